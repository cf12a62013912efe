// sw_pileup.hip -- sw_pileup_kernel, sw_pileup_flag_kernel and sw_pileup_write_kernel (the definition is
// tests/pileup_textbook.py's).
//
// sw_pileup_kernel: one wave per alignment, persistent over the batch, as sw_describe_kernel; the four waves of a workgroup share
// nothing and there is no workgroup barrier.  The alignment's status and select words are read first and nothing else of an alignment
// that is not counted.  Then the check of sw_cigar_wave.h, whole, before the first add: a refused alignment adds nothing.  Then the
// slot is parsed into LDS a chunk at a time and the elements are taken in turn by the whole wave.  An M element goes 64 columns a
// step, clipped to the region beforehand: a lane reads its query byte and adds 1 to the word of that byte's plane at its position.
// A D element adds 1 to 64 consecutive words of plane 5 a step.  An I element is lane 0's: 1 in plane 6 and its length in plane 7 at
// the position in front of the target cursor.  Every add is a relaxed, agent-scope atomic whose result is not used, so the compiler
// emits the form without return; the counts are integers and the adds commute, so the table is the same whatever the order.
// The M step is ONE instruction whose lanes address up to five planes.  The other form -- an exec-masked instruction per channel
// present in the step, each over consecutive words -- was measured and is 3 % slower (docs/history.md).
//
// The sites entry: sw_pileup_flag_kernel, a thread per position, reads the planes (consecutive words of each plane across a wave)
// and the reference byte, writes the call and the flags and counts the sites of its block of PILEUP_SITE_BLOCK positions; rocPRIM's
// device-wide exclusive scan turns the blocks' counts into the blocks' first places (the region is the reference: millions of
// blocks, so no one-block scan); sw_pileup_write_kernel evaluates the positions of the blocks that have sites in front of the
// capacity again and writes their records in position order.
#include "sw_pileup.h"

#include <rocprim/device/device_scan.hpp>

#include "sw_cigar_wave.h"

namespace mgl_sw_dev {

namespace {

using namespace cigar_wave;

// A / a 0, C / c 1, G / g 2, T / t 3, every other byte 4
__device__ __forceinline__ int channel_of(const uint8_t b)
{
    const uint8_t u = b & 0xdf;
    return u == 'A' ? 0 : u == 'C' ? 1 : u == 'G' ? 2 : u == 'T' ? 3 : 4;
}

__device__ __forceinline__ void add_word(uint32_t *const at, const uint32_t v)
{
    (void)__hip_atomic_fetch_add(at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the columns [lo, hi) of an element of `len` columns whose first column stands at `rel` (counted from the region's first position)
// that lie inside the region
__device__ __forceinline__ void clip_columns(const int64_t rel, const int len, const int64_t region_len, int &lo, int &hi)
{
    lo = (int)min(max(-rel, (int64_t)0), (int64_t)len);
    hi = (int)min(max(region_len - rel, (int64_t)0), (int64_t)len);
}

__global__ __launch_bounds__(64 * DESCRIBE_WAVES) void sw_pileup_kernel(const PileupArgs a)
{
    __shared__ WaveLds lds[DESCRIBE_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    WaveLds &L = lds[wave];
    const int64_t waves = (int64_t)gridDim.x * DESCRIBE_WAVES;
    for (int64_t p = (int64_t)blockIdx.x * DESCRIBE_WAVES + wave; p < a.n; p += waves) {
        auto finish = [&](const int status) {
            if (lane == 0 && a.status) a.status[p] = status;
        };
        const int sin = a.status_in ? a.status_in[p] : 0;
        if (sin != 0) { // nothing of the alignment is read
            finish(sin);
            continue;
        }
        if (a.select && a.select[p] == 0) {
            finish(MGL_SW_OK);
            continue;
        }
        const mgl_sw_chain_alignment r = a.aln[p];
        Parser P{};
        if (!check_alignment(P, L, lane, r, a.t_len[p], a.q_len[p], a.cigar_len[p], a.cigar + p * (int64_t)a.cigar_stride, a.cigar_stride, a.binary)) {
            finish(MGL_SW_ERR_BAD_ARG);
            continue;
        }
        // ---- the walk: the first target column stands at rel0, counted from the region's first position
        const int64_t rel0 = a.t_start[p] + r.t_beg - a.region_beg;
        const uint8_t *const Q = a.queries + a.q_start[p] + r.q_beg;
        rewind(P);
        while (P.pos < P.bytes) {
            int count = 0;
            while (P.pos < P.bytes && count + 64 <= DESCRIBE_CHUNK) count += parse_step<true>(P, L, lane, count);
            wave_sync();
            for (int e = 0; e < count; ++e) {
                const int len = L.len[e], op = L.op[e];
                const int64_t rel = rel0 + L.toff[e];
                if (op == OP_M) {
                    const uint8_t *const q = Q + L.qoff[e];
                    int lo, hi;
                    clip_columns(rel, len, a.region_len, lo, hi);
                    for (int64_t c = lo + lane; c < hi; c += 64) {
                        const int ch = channel_of(q[c]);
                        add_word(a.counts + ch * a.region_len + (rel + c), 1u);
                    }
                } else if (op == OP_D) {
                    int lo, hi;
                    clip_columns(rel, len, a.region_len, lo, hi);
                    for (int64_t c = lo + lane; c < hi; c += 64) add_word(a.counts + 5 * a.region_len + (rel + c), 1u);
                } else if (lane == 0 && rel - 1 >= 0 && rel - 1 < a.region_len) { // behind the position in front of the target cursor
                    add_word(a.counts + 6 * a.region_len + (rel - 1), 1u);
                    add_word(a.counts + 7 * a.region_len + (rel - 1), (uint32_t)len);
                }
            }
            wave_sync(); // the chunk is written again
        }
        finish(MGL_SW_OK);
    }
}

// ---- the sites entry

struct Site {
    int flags, ref, call, alt;
    int64_t depth, call_count, alt_count;
};

// position i of the region, all arithmetic in 64 bits
__device__ __forceinline__ Site site_at(const PileupSitesArgs &a, const int64_t i)
{
    int64_t c[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) c[k] = (int64_t)a.counts[k * a.region_len + i];
    Site s;
    s.ref = channel_of(a.ref[i]);
    s.depth = c[0] + c[1] + c[2] + c[3] + c[4] + c[5];
    s.call = 0;
    s.call_count = c[0];
    s.alt = -1;
    s.alt_count = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        if (c[k] > s.call_count) { // (the lowest channel wins a tie)
            s.call = k;
            s.call_count = c[k];
        }
        if (k < 5 && k != s.ref && c[k] > s.alt_count) {
            s.alt = k;
            s.alt_count = c[k];
        }
    }
    auto ok = [&](const int64_t x) { return x >= a.min_alt && x * 256 >= (int64_t)a.min_frac * s.depth; };
    s.flags = 0;
    if (s.depth >= a.min_depth) s.flags = 1 | (ok(s.alt_count) ? 2 : 0) | (ok(c[5]) ? 4 : 0) | (ok(c[6]) ? 8 : 0);
    return s;
}

// -> this thread's place among the block's sites and (in every thread) their number
__device__ __forceinline__ int block_rank(const bool site, int &total)
{
    __shared__ int wave_sites[PILEUP_SITE_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t m = __ballot(site);
    if (lane == 0) wave_sites[wave] = __popcll(m);
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < PILEUP_SITE_BLOCK / 64; ++w) {
        before += w < wave ? wave_sites[w] : 0;
        total += wave_sites[w];
    }
    return before + __popcll(m & (((uint64_t)1 << lane) - 1));
}

__global__ __launch_bounds__(PILEUP_SITE_BLOCK) void sw_pileup_flag_kernel(const PileupSitesArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * PILEUP_SITE_BLOCK + threadIdx.x;
    bool site = false;
    if (i < a.region_len) {
        const Site s = site_at(a, i);
        // "ACGTN*", a byte a channel
        if (a.call) a.call[i] = (s.flags & 1) ? (uint8_t)(0x2a4e54474341ull >> (8 * s.call)) : (uint8_t)'N';
        if (a.flags) a.flags[i] = (uint8_t)s.flags;
        site = (s.flags & 14) != 0;
    }
    int total;
    block_rank(site, total);
    if (threadIdx.x == 0) {
        a.block_count[blockIdx.x] = total;
        if (blockIdx.x == 0) a.block_count[a.blocks] = 0; // the scan's last place is the number of all sites
    }
}

__device__ __forceinline__ int32_t clip31(const int64_t v) { return (int32_t)min(v, (int64_t)0x7fffffff); }

__global__ __launch_bounds__(PILEUP_SITE_BLOCK) void sw_pileup_write_kernel(const PileupSitesArgs a)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) a.n_sites[0] = a.block_start[a.blocks];
    const int64_t first = a.block_start[blockIdx.x];
    if (a.block_count[blockIdx.x] == 0 || first >= a.site_capacity) return; // (the same in every thread)
    const int64_t i = (int64_t)blockIdx.x * PILEUP_SITE_BLOCK + threadIdx.x;
    Site s{};
    if (i < a.region_len) s = site_at(a, i);
    const bool site = (s.flags & 14) != 0;
    int total;
    const int64_t at = first + block_rank(site, total);
    if (site && at < a.site_capacity) {
        mgl_sw_site o;
        o.pos = (int32_t)i;
        o.flags = s.flags;
        o.depth = clip31(s.depth);
        o.ref = s.ref;
        o.call = s.call;
        o.call_count = clip31(s.call_count);
        o.alt = s.alt;
        o.alt_count = clip31(s.alt_count);
        a.sites[at] = o;
    }
}

bool sites_args_good(const PileupSitesArgs &a)
{
    return a.counts && a.ref && a.region_len >= 1 && a.region_len <= PILEUP_MAX_REGION &&
           a.blocks == (a.region_len + PILEUP_SITE_BLOCK - 1) / PILEUP_SITE_BLOCK && a.block_count && a.block_start && a.n_sites &&
           a.site_capacity >= 0 && a.site_capacity <= PILEUP_MAX_SITES && (a.sites || a.site_capacity == 0);
}

} // namespace

hipError_t launch_pileup(const PileupArgs &a, hipStream_t stream)
{
    if (a.n < 1) return hipSuccess;
    if (a.n > DESCRIBE_MAX_CHUNK || a.groups < 1 || a.cigar_stride < 0) return hipErrorInvalidValue;
    if (!a.queries || !a.t_start || !a.q_start || !a.t_len || !a.q_len || !a.aln || !a.cigar || !a.cigar_len || !a.counts) return hipErrorInvalidValue;
    if (a.region_beg < 0 || a.region_len < 1 || a.region_len > PILEUP_MAX_REGION) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_pileup_kernel, dim3((unsigned)a.groups), dim3(64 * DESCRIBE_WAVES), 0, stream, a);
    return hipGetLastError();
}

hipError_t pileup_scan_bytes(const int64_t entries, size_t *bytes)
{
    if (entries < 1 || !bytes) return hipErrorInvalidValue;
    *bytes = 0;
    return rocprim::exclusive_scan(nullptr, *bytes, (const int64_t *)nullptr, (int64_t *)nullptr, (int64_t)0, (size_t)entries, rocprim::plus<int64_t>(), 0);
}

hipError_t launch_pileup_flag(const PileupSitesArgs &a, hipStream_t stream)
{
    if (!sites_args_good(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_pileup_flag_kernel, dim3((unsigned)a.blocks), dim3(PILEUP_SITE_BLOCK), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_pileup_scan(const PileupSitesArgs &a, hipStream_t stream)
{
    if (!sites_args_good(a) || !a.scan_tmp) return hipErrorInvalidValue;
    size_t bytes = a.scan_bytes;
    return rocprim::exclusive_scan(a.scan_tmp, bytes, a.block_count, a.block_start, (int64_t)0, (size_t)(a.blocks + 1), rocprim::plus<int64_t>(), stream);
}

hipError_t launch_pileup_write(const PileupSitesArgs &a, hipStream_t stream)
{
    if (!sites_args_good(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_pileup_write_kernel, dim3((unsigned)a.blocks), dim3(PILEUP_SITE_BLOCK), 0, stream, a);
    return hipGetLastError();
}

} // namespace mgl_sw_dev
