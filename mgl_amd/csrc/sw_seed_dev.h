// sw_seed_dev.h -- the device helpers that the seeding kernels and sw_rank.hip share: the k-mer's code and hash, and the bitonic sort of a
// workgroup of SEED_THREADS.  None of them names LDS (what does is sw_seed_sketch.h's); each translation unit gets its own copy (unnamed
// namespace).
#ifndef MGL_SW_SEED_DEV_H
#define MGL_SW_SEED_DEV_H

#include "sw_seed.h"

namespace mgl_sw_dev {

namespace {

__device__ inline uint32_t seed_hash(uint32_t key)
{
    uint32_t h = key ^ 0x9E3779B9u;
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    return h ^ (h >> 16);
}

__device__ inline uint8_t seed_code(uint8_t b) { return b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : 4; }

// a[0 .. n2), n2 a power of two, ascending; `val` (or null) moves with its key
__device__ __noinline__ void seed_bitonic(uint64_t *a, uint32_t *val, const int n2)
{
    for (int size = 2; size <= n2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = threadIdx.x; i < n2 / 2; i += SEED_THREADS) {
                const int l = 2 * i - (i & (stride - 1)), h = l + stride;
                const bool asc = (l & size) == 0;
                const uint64_t x = a[l], y = a[h];
                if ((x > y) == asc) {
                    a[l] = y;
                    a[h] = x;
                    if (val) {
                        const uint32_t vx = val[l];
                        val[l] = val[h];
                        val[h] = vx;
                    }
                }
            }
            __syncthreads();
        }
}

__device__ inline int seed_pow2(const int n)
{
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

} // namespace

} // namespace mgl_sw_dev

#endif
