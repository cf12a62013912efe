// sw_seed_sketch.h -- what the three seeding kernels share (sw_seed_kernel, sw_seed_strands_kernel, sw_seed_index_kernel; DESIGN.md
// sections 9h - 9j) and, of it, what the index build's sw_index_sketch_kernel uses: the sketch of a block of SEED_BLOCK positions with
// its LDS, the workgroup's prefix sum, the read's sorted table, a window block against a table, and the merge with the row's staging.
// Included by sw_seed.hip, sw_seed_strands.hip and sw_index.hip only: it declares LDS, of which every translation unit gets its own
// (unnamed namespace).  The tables and the hits are the kernels': their sizes differ, and they reach these functions as a pair of
// pointers, `lds` for the place in LDS and `slot` for the one in the workgroup's workspace slot, with the capacity of the first.  Where
// a table or a row's hits live follows from their number alone, so no pointer is carried between the phases.
//
// __noinline__ on the sketch and the probe (and on the sort, sw_seed_dev.h), __forceinline__ on the table and the staging: a kernel with
// all of its phases inlined keeps more wave-uniform values alive than there are scalar registers, and a phase that is inlined is inlined
// once, so only leaves are called (no frame, no scratch).
#ifndef MGL_SW_SEED_SKETCH_H
#define MGL_SW_SEED_SKETCH_H

#include "sw_seed_dev.h"

namespace mgl_sw_dev {

namespace {

constexpr int SEED_ST_BAD_ARG = 1, SEED_ST_NOMEM = 3, SEED_ST_UNSUPPORTED = 5; // mgl_sw_status
constexpr int SEED_SPAN = SEED_BLOCK + 2 * SEED_MAX_W;                        // positions staged for one block (B + 2 w - 2 at most)

struct SeedSketchLds {
    uint32_t key[SEED_SPAN];
    uint32_t hash[SEED_SPAN];
    uint32_t flag[SEED_BLOCK / 4]; // a byte per position of the block
    uint8_t code[SEED_SPAN + SEED_MAX_K];
    uint8_t valid[SEED_SPAN];
    int wave_sum[SEED_THREADS / 64];
};
static_assert(sizeof(SeedSketchLds) % 8 == 0, "a kernel's 8-byte tables follow it without a gap");
__shared__ SeedSketchLds s;

// the inclusive prefix sum of v over the wave
template <typename T>
__device__ __forceinline__ T wave_inclusive_sum(T v)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T up = __shfl_up(v, d);
        if (lane >= d) v += up;
    }
    return v;
}

// the exclusive prefix sum of v over the workgroup of SEED_THREADS, and the sum
__device__ inline int seed_block_scan(const int v, int &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int incl = wave_inclusive_sum(v);
    if (lane == 63) s.wave_sum[wave] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int x = 0; x < SEED_THREADS / 64; ++x) {
        const int ws = s.wave_sum[x];
        before += x < wave ? ws : 0;
        all += ws;
    }
    __syncthreads();
    total = all;
    return before + incl - v;
}

// Positions [p0, p0 + SEED_BLOCK) of a sequence of nk k-mer positions (nk + k - 1 bytes): key, hash and validity of every position a
// window over them can see, from `lo` on (returned), and flag[] set for the selected ones among them.  `rev` sketches the reverse
// complement of seq without making it: byte i of it is read at last - i and its code is 3 - c, and everything behind that load works
// in the ORIENTED sequence's coordinates.
__device__ __noinline__ int64_t seed_sketch_block(const uint8_t *seq, const int64_t nk, const int k, const int w, const int64_t p0, const bool rev)
{
    const int tid = threadIdx.x;
    const int64_t lo = p0 - w + 1 > 0 ? p0 - w + 1 : 0;
    const int64_t hi = p0 + SEED_BLOCK + w - 2 < nk - 1 ? p0 + SEED_BLOCK + w - 2 : nk - 1; // the last position a window sees
    const int npos = (int)(hi - lo + 1), nbytes = npos + k - 1;
    const int64_t last = nk + k - 2; // the sequence's last byte
    for (int i = tid; i < nbytes; i += SEED_THREADS) {
        const uint8_t c = seed_code(seq[rev ? last - (lo + i) : lo + i]); // (lo + i <= hi + k - 1 <= last)
        s.code[i] = rev && c < 4 ? 3 - c : c;
    }
    s.flag[tid] = 0;
    __syncthreads();
    for (int i = tid; i < npos; i += SEED_THREADS) {
        uint32_t key = 0, bad = 0;
        for (int j = 0; j < k; ++j) {
            const uint32_t c = s.code[i + j];
            bad |= c >> 2;
            key = key << 2 | (c & 3);
        }
        s.key[i] = key;
        s.hash[i] = seed_hash(key);
        s.valid[i] = !bad;
    }
    __syncthreads();
    const int64_t last_win = nk - w > 0 ? nk - w : 0;
    const int64_t a_hi = p0 + SEED_BLOCK - 1 < last_win ? p0 + SEED_BLOCK - 1 : last_win;
    uint8_t *const flag = reinterpret_cast<uint8_t *>(s.flag);
    for (int64_t a = lo + tid; a <= a_hi; a += SEED_THREADS) {
        const int from = (int)(a - lo), to = (int)((a + w < nk ? a + w : nk) - lo);
        int best = -1;
        uint32_t best_h = 0;
        for (int i = from; i < to; ++i) {
            const uint32_t h = s.hash[i];
            const bool take = s.valid[i] && (best < 0 || h < best_h); // (strict `<` while the position ascends: ties to the smallest)
            best = take ? i : best;
            best_h = take ? h : best_h;
        }
        const int64_t at = best + lo - p0;
        if (best >= 0 && at >= 0 && at < SEED_BLOCK) flag[at] = 1;
    }
    __syncthreads();
    return lo;
}

// (a) the table of a read in one orientation, (key << 32 | position) sorted, in `lds` or -- above lds_cap entries -- in `slot`.
// -> its entries; 0: no key to meet, no hit; -1: a sketch above SEED_MAX_QUERY_SEEDS, refused
__device__ __forceinline__ int seed_build_table(const uint8_t *Q, const int nkq, const int k, const int w, const bool rev, uint64_t *lds, uint64_t *slot,
                                                const int lds_cap)
{
    const int tid = threadIdx.x;
    const uint8_t *const flag = reinterpret_cast<const uint8_t *>(s.flag);
    int nq = 0;
    for (uint32_t p0 = 0; (int64_t)p0 < nkq; p0 += SEED_BLOCK) { // (unsigned: the step past a sequence of nearly 2^31 bytes)
        const int64_t lo = seed_sketch_block(Q, nkq, k, w, p0, rev);
        const uint32_t f = s.flag[tid];
        int total;
        int at = nq + seed_block_scan(__popc(f), total);
        if (nq + total > SEED_MAX_QUERY_SEEDS) return -1;
        if (nq <= lds_cap && nq + total > lds_cap) // the table leaves LDS
            for (int i = tid; i < nq; i += SEED_THREADS) slot[i] = lds[i];
        uint64_t *const tab = nq + total > lds_cap ? slot : lds;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (flag[tid * 4 + j]) {
                const int64_t pos = p0 + tid * 4 + j;
                tab[at++] = (uint64_t)s.key[pos - lo] << 32 | (uint64_t)pos;
            }
        nq += total;
        __syncthreads();
    }
    if (nq == 0) return 0;
    uint64_t *const tab = nq > lds_cap ? slot : lds;
    const int n2 = seed_pow2(nq);
    for (int i = nq + tid; i < n2; i += SEED_THREADS) tab[i] = ~0ull;
    __syncthreads();
    seed_bitonic(tab, nullptr, n2);
    return nq;
}

// (b) the window's block that seed_sketch_block left in LDS (positions from p0, staged from lo) against a table, never stored: a
// selected position looks its key up (binary search, then the run of equal keys, dropped above max_occ) and a prefix sum over the run
// lengths says where its hits go -- the row's raw hits (t << 32 | q) behind the R it has, ascending by (t, q) without a sort, in `lds` or
// -- above lds_cap -- in `slot`.  -> the new R, or -1 beyond max_cand.  (`inline`: sw_index.hip probes the index instead and does not call it)
__device__ __noinline__ inline int seed_probe_block(const uint64_t *tab, const int nq, uint64_t *lds, uint64_t *slot, const int lds_cap, const int R,
                                                    const uint32_t p0, const int64_t lo, const int max_occ, const int max_cand)
{
    const int tid = threadIdx.x;
    const uint8_t *const flag = reinterpret_cast<const uint8_t *>(s.flag);
    int first[4], cnt[4], sum = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        first[j] = cnt[j] = 0;
        if (flag[tid * 4 + j]) {
            const uint32_t key = s.key[p0 + tid * 4 + j - lo];
            const uint64_t want = (uint64_t)key << 32;
            int b = 0, e = nq; // the first entry not below `want`
            while (b < e) {
                const int m = (b + e) >> 1;
                if (tab[m] < want) b = m + 1;
                else e = m;
            }
            int c = 0;
            while (b + c < nq && c <= max_occ && (uint32_t)(tab[b + c] >> 32) == key) ++c;
            first[j] = b;
            cnt[j] = c <= max_occ ? c : 0;
            sum += cnt[j];
        }
    }
    int total;
    int at = R + seed_block_scan(sum, total);
    if (R + total > max_cand) return -1;
    if (R <= lds_cap && R + total > lds_cap) // the hits leave LDS (max_cand is above lds_cap: the slot has the room)
        for (int i = tid; i < R; i += SEED_THREADS) slot[i] = lds[i];
    uint64_t *const hits = R + total > lds_cap ? slot : lds;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint64_t t = (uint64_t)(p0 + tid * 4 + j) << 32;
        for (int c = 0; c < cnt[j]; ++c) hits[at++] = t | (uint32_t)tab[first[j] + c];
    }
    __syncthreads();
    return R + total;
}

// (c), (d) a row's R raw hits (t << 32 | q) -> its candidates, ascending by (t, q), in its staging (st: t, then q, then l, max_cand
// each).  ORDERED: the hits arrive ascending by (t, q), as seed_probe_block leaves them; otherwise (the index's, in key order) the
// merge = 0 path sorts them first.  The merge: the hits re-keyed (diagonal << 32 | t) and sorted; a hit is a run's head iff it is the
// first of its diagonal or starts beyond the end of the one before it, which says the same as "beyond the end of the run so far"
// because all hits are k long; the r-th head and the r-th tail are one run's, so heads and tails are compacted by one prefix count;
// the runs are sorted back by (t, q) with their lengths.  `run` and `len` hold them meanwhile.  No barrier behind the last loop.
// -> N, the row's candidates
template <bool ORDERED>
__device__ __forceinline__ int seed_stage_row(uint64_t *hits, const int R, uint64_t *run, uint32_t *len, int32_t *st, const int max_cand, const int k,
                                              const int merge)
{
    const int tid = threadIdx.x;
    int32_t *const sq = st + max_cand, *const sl = sq + max_cand;
    if (R == 0) return 0;
    const int n2 = seed_pow2(R);
    if (!merge) {
        if (!ORDERED) {
            for (int i = R + tid; i < n2; i += SEED_THREADS) hits[i] = ~0ull;
            __syncthreads();
            seed_bitonic(hits, nullptr, n2);
        }
        for (int i = tid; i < R; i += SEED_THREADS) {
            const uint64_t h = hits[i];
            st[i] = (int32_t)(h >> 32);
            sq[i] = (int32_t)(uint32_t)h;
            sl[i] = k;
        }
        return R;
    }
    for (int i = tid; i < n2; i += SEED_THREADS) {
        const uint64_t h = i < R ? hits[i] : 0;
        const uint32_t t = (uint32_t)(h >> 32), q = (uint32_t)h;
        hits[i] = i < R ? (uint64_t)(t - q + 0x80000000u) << 32 | t : ~0ull;
    }
    __syncthreads();
    seed_bitonic(hits, nullptr, n2);
    int N = 0;
    for (int base = 0; base < R; base += SEED_THREADS) {
        const int i = base + tid;
        bool head = false, tail = false;
        uint64_t me = 0;
        if (i < R) {
            me = hits[i];
            const uint64_t prev = i > 0 ? hits[i - 1] : 0, next = i + 1 < R ? hits[i + 1] : 0;
            head = i == 0 || (prev >> 32) != (me >> 32) || me > prev + (uint64_t)k; // (the same diagonal: the difference is t's)
            tail = i + 1 == R || (next >> 32) != (me >> 32) || next > me + (uint64_t)k;
        }
        int total;
        const int r = N + seed_block_scan(head ? 1 : 0, total) + (head ? 1 : 0) - 1; // the run this hit belongs to
        const uint32_t t = (uint32_t)me, d = (uint32_t)(me >> 32);
        if (head) run[r] = (uint64_t)t << 32 | (uint32_t)(t - d + 0x80000000u);
        if (tail) len[r] = t + (uint32_t)k; // the run's end; its length once the head is known to all
        N += total;
    }
    __syncthreads();
    const int m2 = seed_pow2(N);
    for (int i = tid; i < m2; i += SEED_THREADS) {
        if (i < N) len[i] -= (uint32_t)(run[i] >> 32);
        else run[i] = ~0ull, len[i] = 0;
    }
    __syncthreads();
    seed_bitonic(run, len, m2);
    for (int i = tid; i < N; i += SEED_THREADS) {
        const uint64_t h = run[i];
        st[i] = (int32_t)(h >> 32);
        sq[i] = (int32_t)(uint32_t)h;
        sl[i] = (int32_t)len[i];
    }
    return N;
}

} // namespace

} // namespace mgl_sw_dev

#endif
