// sw_index.hip -- the kernels of mgl_sw_index_build_device, mgl_sw_seed_index_batch_device and mgl_sw_locate_window_batch_device
// (the function is tests/index_textbook.py's).  sw_index.h describes the index and the workspace.
//
// The build, once per reference and not the hot path: sw_index_sketch_kernel sketches the reference SEED_BLOCK k-mer positions per
// workgroup with the w - 1 positions to either side (sw_seed_kernel's sketch with 64-bit positions), in two passes: the first counts a
// block's selected positions, sw_index_scan_kernel sums the counts (one workgroup, INDEX_SCAN_THREADS blocks a step with a running
// carry), and -- the host having learnt M and allocated exactly that -- the second writes key << 32 | position where the sums say.
// rocPRIM sorts the entries over bits [0, 32 + 2k), sw_index_split_kernel takes keys and positions apart and sw_index_bucket_kernel
// finds every bucket's first entry by a binary search of its own.
//
// sw_seed_index_kernel, the hot path: one workgroup of 256 threads per read, persistent; the rows of a read (Q, then rc(Q) read from Q's
// bytes in place) one after the other, sw_seed_strands_kernel's scheme with the roles swapped:
//   (a) the row's sketch as (key << 32 | q), bitonic-sorted: equal keys are neighbours, the length of their run is occ_Q;
//   (b) the head of every run looks its key up: the bucket's bounds, a lower bound between them and an upper bound no further than
//       max_occ_ref + 1 entries on.  A prefix sum over occ_Q * occ_I of the kept keys places the raw hits (t << 32 | q), in key order,
//       and the workgroup writes them a hit per thread, whoever's key they belong to;
//   (c) the merge as in sw_seed_kernel (re-keyed by (diagonal, t), sorted, heads and tails, sorted back by (t, q)); with merge = 0 one
//       sort by (t, q);
//   (d) N and the candidates go to the row's staging, which sw_seed_scan_kernel and sw_seed_pack_kernel read.
// The table and the hits live in LDS up to SEED_LDS_TAB and SEED_LDS_HITS entries and in the workgroup's slot beyond.
//
// sw_locate_window_kernel: a wave per pair: the checks over the pair's anchors, the window, the anchors' t rebased in 4-byte stores.
//
// The contigs of a reference (the functions are tests/contig_textbook.py's; sw_index.h has the table):
// sw_contig_gap_kernel (the build: a workgroup per gap looks for a base), sw_contig_of_kernel (a thread per anchor: the contig that holds
// it, the table searched in LDS where it fits) and sw_locate_window_contigs_kernel (sw_locate_window_kernel inside the contig of the
// pair's first anchor).
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>

#include "sw_index.h"
#include "sw_seed_sketch.h"

namespace mgl_sw_dev {

namespace {

__shared__ uint64_t s_tab[SEED_LDS_TAB];   // sw_seed_index_kernel's alone, and s_hits
__shared__ uint64_t s_hits[SEED_LDS_HITS];
struct IndexProbeLds { // a probe step, per thread: where its hits start in the step, its key's first entry, occ_I << 8 | occ_Q
    int start[SEED_THREADS];
    uint32_t first[SEED_THREADS];
    int occ[SEED_THREADS];
};
__shared__ IndexProbeLds s_probe;
static_assert(SEED_MAX_OCC < 256, "occ_Q shares a word with occ_I");
static_assert(sizeof(SeedSketchLds) + sizeof(s_tab) + sizeof(s_hits) + sizeof(IndexProbeLds) <= 80 * 1024, "two workgroups share a CU's 160 KiB of LDS");
static_assert(SEED_LDS_TAB * 8 >= SEED_LDS_HITS * 12, "the runs and their lengths fit where the table was");

// ---------------------------------------------------------------------------------------------------------------- the build

// pass 0: block_count; pass 1: the entries, where block_start says
__global__ __launch_bounds__(SEED_THREADS) void sw_index_sketch_kernel(const IndexBuildArgs a, const int pass)
{
    const int tid = threadIdx.x;
    const int64_t nk = a.ref_len - a.k + 1;
    const uint8_t *const flag = reinterpret_cast<const uint8_t *>(s.flag);
    for (int64_t b = blockIdx.x; b < a.blocks; b += gridDim.x) {
        const int64_t p0 = b * SEED_BLOCK;
        const int64_t lo = seed_sketch_block(a.ref, nk, a.k, a.w, p0, false);
        int total;
        const int before = seed_block_scan(__popc(s.flag[tid]), total);
        if (pass == 0) {
            if (tid == 0) a.block_count[b] = (uint32_t)total;
        } else {
            int64_t at = (int64_t)a.block_start[b] + before;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (flag[tid * 4 + j]) {
                    const int64_t pos = p0 + tid * 4 + j;
                    a.entries[at++] = (uint64_t)s.key[pos - lo] << 32 | (uint64_t)pos;
                }
        }
        __syncthreads(); // (the next block's sketch writes what this one still reads)
    }
}

__global__ __launch_bounds__(INDEX_SCAN_THREADS) void sw_index_scan_kernel(const IndexBuildArgs a)
{
    __shared__ uint32_t wave_sum[INDEX_SCAN_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t carry = 0; // (M is below 2^31)
    for (int64_t base = 0; base < a.blocks; base += INDEX_SCAN_THREADS) {
        const int64_t b = base + tid;
        const uint32_t own = b < a.blocks ? a.block_count[b] : 0;
        const uint32_t incl = wave_inclusive_sum(own);
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        uint32_t before = carry, all = 0;
#pragma unroll
        for (int x = 0; x < INDEX_SCAN_THREADS / 64; ++x) {
            const uint32_t sum = wave_sum[x];
            before += x < wave ? sum : 0;
            all += sum;
        }
        __syncthreads();
        if (b < a.blocks) a.block_start[b] = before + incl - own;
        carry += all;
    }
    if (tid == 0) a.block_start[a.blocks] = carry;
}

__global__ __launch_bounds__(256) void sw_index_split_kernel(const uint64_t *sorted, const int64_t m, uint32_t *keys, int32_t *pos)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (int64_t)gridDim.x * 256) {
        const uint64_t e = sorted[i];
        keys[i] = (uint32_t)(e >> 32);
        pos[i] = (int32_t)(uint32_t)e;
    }
}

// bucket[j], j in [0, 2^bucket_bits]: the first entry whose key is not below j << (2k - bucket_bits)
__global__ __launch_bounds__(256) void sw_index_bucket_kernel(const uint32_t *keys, const int64_t m, const int shift, const int64_t buckets, uint32_t *bucket)
{
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j <= buckets; j += (int64_t)gridDim.x * 256) {
        const uint64_t want = (uint64_t)j << shift;
        int64_t b = 0, e = m;
        while (b < e) {
            const int64_t mid = (b + e) >> 1;
            if ((uint64_t)keys[mid] < want) b = mid + 1;
            else e = mid;
        }
        bucket[j] = (uint32_t)b;
    }
}

// ---------------------------------------------------------------------------------------------------------------- the lookup

// the index's entries with `key`: -> their number, 0 where there are more than max_occ_ref, and the first of them
__device__ inline int index_lookup(const IndexView &ix, const uint32_t key, const int max_occ_ref, uint32_t &first)
{
    const uint32_t b = key >> (2 * ix.k - ix.bucket_bits);
    const uint32_t lo = ix.bucket[b], hi = ix.bucket[b + 1];
    uint32_t x = lo, y = hi; // the first entry not below `key` (entries < 2^31: the sums fit)
    while (x < y) {
        const uint32_t m = (x + y) >> 1;
        if (ix.keys[m] < key) x = m + 1;
        else y = m;
    }
    first = x;
    const uint32_t far = x + (uint32_t)max_occ_ref + 1;
    uint32_t u = x, v = hi < far ? hi : far; // the first entry above `key`, no further than one beyond the cap
    while (u < v) {
        const uint32_t m = (u + v) >> 1;
        if (ix.keys[m] <= key) u = m + 1;
        else v = m;
    }
    const int cnt = (int)(u - x);
    return cnt > max_occ_ref ? 0 : cnt;
}

// (b) the sorted table against the index: the row's raw hits (t << 32 | q) in key order, in s_hits or -- above SEED_LDS_HITS -- in `slot`.
// -> R, or -1 beyond max_cand
__device__ __forceinline__ int index_probe(const IndexView &ix, const uint64_t *tab, const int nq, uint64_t *slot, const int max_occ, const int max_occ_ref,
                                           const int max_cand)
{
    const int tid = threadIdx.x;
    int R = 0;
    for (int base = 0; base < nq; base += SEED_THREADS) {
        const int i = base + tid;
        int occ_q = 0, occ_i = 0, mine = 0;
        uint32_t first = 0;
        if (i < nq) {
            const uint32_t key = (uint32_t)(tab[i] >> 32);
            if (i == 0 || (uint32_t)(tab[i - 1] >> 32) != key) { // the head of its run
                int c = 1;
                while (i + c < nq && c <= max_occ && (uint32_t)(tab[i + c] >> 32) == key) ++c;
                if (c <= max_occ) {
                    occ_q = c;
                    occ_i = index_lookup(ix, key, max_occ_ref, first);
                    mine = occ_q * occ_i;                       // (at most 64 * 8192)
                    mine = mine <= max_cand ? mine : max_cand + 1; // (the sum over the workgroup stays an int; the row is refused below)
                }
            }
        }
        int total;
        const int start = seed_block_scan(mine, total); // where this thread's hits begin in the step
        if (R + total > max_cand) return -1;
        if (R <= SEED_LDS_HITS && R + total > SEED_LDS_HITS) // the hits leave LDS (max_cand is above SEED_LDS_HITS: the slot has the room)
            for (int x = tid; x < R; x += SEED_THREADS) slot[x] = s_hits[x];
        uint64_t *const hits = R + total > SEED_LDS_HITS ? slot : s_hits;
        // the step's hits are written by the whole workgroup, not by the heads: a key at both caps is 8 192 hits.  Hit h of the step
        // belongs to the last thread that starts at or before it (a thread without hits starts where its successor does)
        s_probe.start[tid] = start;
        s_probe.first[tid] = first;
        s_probe.occ[tid] = occ_i << 8 | occ_q;
        __syncthreads();
        for (int h = tid; h < total; h += SEED_THREADS) {
            int b = 0, e = SEED_THREADS - 1;
            while (b < e) {
                const int m = (b + e + 1) >> 1;
                if (s_probe.start[m] <= h) b = m;
                else e = m - 1;
            }
            const int j = h - s_probe.start[b], oq = s_probe.occ[b] & 255, x = j / oq, c = j - x * oq; // entry x of the index, position c of the run
            hits[R + h] = (uint64_t)(uint32_t)ix.pos[s_probe.first[b] + x] << 32 | (uint32_t)tab[base + b + c];
        }
        R += total;
        __syncthreads();
    }
    return R;
}

__global__ __launch_bounds__(SEED_THREADS) void sw_seed_index_kernel(const SeedIndexArgs aa)
{
    const SeedStageArgs &a = aa.s;
    const int tid = threadIdx.x;
    const int k = aa.ix.k, w = aa.ix.w;
    const SeedWorkspace sg = seed_workspace(a.n, a.max_cand); // (a.n: the rows)
    int32_t *const count = reinterpret_cast<int32_t *>(a.ws + sg.count), *const stage = reinterpret_cast<int32_t *>(a.ws + sg.stage);
    unsigned char *const slot = a.ws + sg.bytes + (int64_t)blockIdx.x * sg.slot_bytes;
    uint64_t *const slot_tab = reinterpret_cast<uint64_t *>(slot);
    uint64_t *const slot_hits = reinterpret_cast<uint64_t *>(slot + SEED_SLOT_TAB); // (both only where max_cand is above SEED_LDS_HITS)
    uint32_t *const slot_len = reinterpret_cast<uint32_t *>(slot + SEED_SLOT_LEN);
    const int reads = (int)(a.n / aa.strands); // (rows <= 2^30)

    for (int p = blockIdx.x; p < reads; p += a.groups) {
        const int ql = a.q_len[p];
        const uint8_t *const Q = a.queries + a.q_start[p];
#pragma nounroll
        for (int r = 0; r < aa.strands; ++r) {
            __syncthreads(); // (the row before this one is done with LDS)
            const int64_t row = (int64_t)p * aa.strands + r;
            if (tid == 0) {
                if (aa.row_t_len) aa.row_t_len[row] = (int32_t)aa.ix.ref_len;
                if (aa.row_q_len) aa.row_q_len[row] = ql;
            }
            auto finish = [&](const int n_cand, const int status) {
                if (tid != 0) return;
                count[row] = n_cand;
                if (a.status) a.status[row] = status;
            };
            if (ql < 1) {
                finish(0, SEED_ST_BAD_ARG);
                continue;
            }
            // ---- (a) nq < 0: the row is refused; nq = 0: no key to look up, no hit
            const int nq = seed_build_table(Q, ql - k + 1, k, w, r == 1, s_tab, slot_tab, SEED_LDS_TAB);
            if (nq < 0) {
                finish(0, SEED_ST_UNSUPPORTED);
                continue;
            }
            // ---- (b)
            const int R = index_probe(aa.ix, nq > SEED_LDS_TAB ? slot_tab : s_tab, nq, slot_hits, a.max_occ, aa.max_occ_ref, a.max_cand);
            if (R < 0) {
                finish(0, SEED_ST_UNSUPPORTED);
                continue;
            }
            // ---- (c), (d) the runs go where the table was: it is not read again
            const bool in_lds = R <= SEED_LDS_HITS;
            const int N = seed_stage_row<false>(in_lds ? s_hits : slot_hits, R, in_lds ? s_tab : slot_tab,
                                          in_lds ? reinterpret_cast<uint32_t *>(s_tab + SEED_LDS_HITS) : slot_len, stage + row * 3 * a.max_cand, a.max_cand,
                                          k, a.merge);
            finish(N, 0);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- the window

__global__ __launch_bounds__(64) void sw_locate_window_kernel(const LocateArgs a)
{
    const int lane = threadIdx.x;
    for (int64_t p = blockIdx.x; p < a.n; p += gridDim.x) {
        const int64_t ql = a.q_len[p], a0 = a.anchor_start[p], a1 = a.anchor_start[p + 1];
        bool bad = ql < 1 || a0 < 0 || a1 < a0 || a1 > a.total_anchors;
        const int64_t K = bad ? 0 : a1 - a0;
        bool mine = false;
        for (int64_t m = lane; m < K; m += 64) {
            const int64_t t = a.anchor_t[a0 + m], q = a.anchor_q[a0 + m], l = a.anchor_len[a0 + m];
            mine = mine || l < 1 || t < 0 || q < 0 || t + l > a.ref_len || q + l > ql;
        }
        bad = bad || __any(mine);
        int status = bad ? SEED_ST_BAD_ARG : 0;
        int64_t lo = 0, hi = 0;
        if (!bad && K > 0) { // (the first and the last anchor are read before any is rebased: the output may be the input)
            const int64_t t0 = a.anchor_t[a0], q0 = a.anchor_q[a0];
            const int64_t tK = a.anchor_t[a1 - 1], qK = a.anchor_q[a1 - 1], lK = a.anchor_len[a1 - 1];
            lo = t0 - q0 - a.slack;
            lo = lo > 0 ? lo : 0;
            hi = tK + lK + (ql - qK - lK) + a.slack;
            hi = hi < a.ref_len ? hi : a.ref_len;
            if (hi - lo > a.max_tl) status = SEED_ST_UNSUPPORTED;
        }
        const bool kept = status == 0 && K > 0;
        if (kept)
            for (int64_t m = lane; m < K; m += 64) a.anchor_t_out[a0 + m] = (int32_t)(a.anchor_t[a0 + m] - lo);
        if (lane == 0) {
            a.t_start[p] = kept ? lo : 0;
            a.t_len[p] = kept ? (int32_t)(hi - lo) : 0;
            if (a.status) a.status[p] = status;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- the contigs

// the contig that holds [t, t + l): the last c with start[c] <= t, where t + l <= end[c] -- -1 where there is none: t < 0, l < 1, inside
// a gap, or over a contig's end.  n = 0: one contig [0, ref_len), no table read.  `start` and `end`: pointers, or the LDS arrays themselves
template <typename A>
__device__ __forceinline__ int contig_find(const A &start, const A &end, const int n, const int ref_len, const int64_t t, const int64_t l)
{
    if (t < 0 || l < 1) return -1;
    if (n == 0) return t + l <= ref_len ? 0 : -1;
    int b = 0, e = n; // the first contig that starts beyond t
    while (b < e) {
        const int m = (b + e) >> 1;
        if (start[m] <= t) b = m + 1;
        else e = m;
    }
    return b > 0 && t + l <= end[b - 1] ? b - 1 : -1;
}

// a workgroup per gap: gap g lies between contig g and contig g + 1
__global__ __launch_bounds__(256) void sw_contig_gap_kernel(const uint8_t *ref, const ContigView cv, int32_t *flag)
{
    const int g = blockIdx.x;
    bool base = false;
    for (int64_t i = (int64_t)cv.end[g] + threadIdx.x; i < cv.start[g + 1]; i += 256) base |= seed_code(ref[i]) < 4;
    if (base) *flag = 1;
}

// a thread per anchor; the table staged in LDS where it fits
template <bool LDS>
__global__ __launch_bounds__(256) void sw_contig_of_kernel(const ContigOfArgs a)
{
    __shared__ int32_t s_start[LDS ? CONTIG_LDS_MAX : 1], s_end[LDS ? CONTIG_LDS_MAX : 1];
    if constexpr (LDS) {
        for (int i = threadIdx.x; i < a.cv.n; i += 256) s_start[i] = a.cv.start[i], s_end[i] = a.cv.end[i];
        __syncthreads();
    }
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.total; i += (int64_t)gridDim.x * 256) {
        const int64_t t = a.t[i], l = a.len[i];
        if constexpr (LDS) a.group[i] = contig_find(s_start, s_end, a.cv.n, a.cv.ref_len, t, l);
        else a.group[i] = contig_find(a.cv.start, a.cv.end, a.cv.n, a.cv.ref_len, t, l);
    }
}

// sw_locate_window_kernel with the window kept inside the contig of the read's first anchor; every anchor has to lie in that contig
__global__ __launch_bounds__(64) void sw_locate_window_contigs_kernel(const LocateContigsArgs aa)
{
    const LocateArgs &a = aa.l;
    const ContigView &cv = aa.cv;
    const int lane = threadIdx.x;
    for (int64_t p = blockIdx.x; p < a.n; p += gridDim.x) {
        const int64_t ql = a.q_len[p], a0 = a.anchor_start[p], a1 = a.anchor_start[p + 1];
        bool bad = ql < 1 || a0 < 0 || a1 < a0 || a1 > a.total_anchors;
        const int64_t K = bad ? 0 : a1 - a0;
        const int c = K > 0 ? contig_find(cv.start, cv.end, cv.n, cv.ref_len, a.anchor_t[a0], a.anchor_len[a0]) : -1; // (the same in every lane)
        bool mine = false;
        for (int64_t m = lane; m < K; m += 64) {
            const int64_t t = a.anchor_t[a0 + m], q = a.anchor_q[a0 + m], l = a.anchor_len[a0 + m];
            mine = mine || q < 0 || q + l > ql || contig_find(cv.start, cv.end, cv.n, cv.ref_len, t, l) != c;
        }
        bad = bad || (K > 0 && c < 0) || __any(mine);
        int status = bad ? SEED_ST_BAD_ARG : 0;
        int64_t lo = 0, hi = 0;
        if (!bad && K > 0) { // (the first and the last anchor are read before any is rebased: the output may be the input)
            const int64_t t0 = a.anchor_t[a0], q0 = a.anchor_q[a0];
            const int64_t tK = a.anchor_t[a1 - 1], qK = a.anchor_q[a1 - 1], lK = a.anchor_len[a1 - 1];
            const int64_t cs = cv.n ? cv.start[c] : 0, ce = cv.n ? cv.end[c] : cv.ref_len;
            lo = t0 - q0 - a.slack;
            lo = lo > cs ? lo : cs;
            hi = tK + lK + (ql - qK - lK) + a.slack;
            hi = hi < ce ? hi : ce;
            if (hi - lo > a.max_tl) status = SEED_ST_UNSUPPORTED;
        }
        const bool kept = status == 0 && K > 0;
        if (kept)
            for (int64_t m = lane; m < K; m += 64) a.anchor_t_out[a0 + m] = (int32_t)(a.anchor_t[a0 + m] - lo);
        if (lane == 0) {
            a.t_start[p] = kept ? lo : 0;
            a.t_len[p] = kept ? (int32_t)(hi - lo) : 0;
            aa.rid[p] = kept ? c : -1;
            if (a.status) a.status[p] = status;
        }
    }
}

int index_grid(const int64_t items, const int per_block)
{
    const int64_t blocks = (items + per_block - 1) / per_block;
    return (int)(blocks < 1 ? 1 : blocks < 65536 ? blocks : 65536);
}

} // namespace

static hipError_t launch_index_sketch(const IndexBuildArgs &a, const int pass, hipStream_t stream)
{
    if (a.blocks < 1) return hipSuccess;
    if (!a.ref || a.ref_len < 1 || a.ref_len > INDEX_MAX_REF || a.k < SEED_MIN_K || a.k > SEED_MAX_K || a.w < 1 || a.w > SEED_MAX_W) return hipErrorInvalidValue;
    if (a.blocks != (a.ref_len - a.k + 1 + SEED_BLOCK - 1) / SEED_BLOCK || !a.block_count || !a.block_start || (pass && !a.entries)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_index_sketch_kernel, dim3((unsigned)index_grid(a.blocks, 1)), dim3(SEED_THREADS), 0, stream, a, pass);
    return hipGetLastError();
}

hipError_t launch_index_count(const IndexBuildArgs &a, hipStream_t stream) { return launch_index_sketch(a, 0, stream); }
hipError_t launch_index_write(const IndexBuildArgs &a, hipStream_t stream) { return launch_index_sketch(a, 1, stream); }

hipError_t launch_index_scan(const IndexBuildArgs &a, hipStream_t stream)
{
    if (a.blocks < 0 || !a.block_start || (a.blocks > 0 && !a.block_count)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_index_scan_kernel, dim3(1), dim3(INDEX_SCAN_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t index_sort_entries(uint64_t *entries, uint64_t *sorted, const int64_t m, const int k, hipStream_t stream)
{
    if (m < 1) return hipSuccess;
    if (!entries || !sorted || m > INDEX_MAX_REF) return hipErrorInvalidValue;
    size_t bytes = 0;
    hipError_t he = rocprim::radix_sort_keys(nullptr, bytes, entries, sorted, (size_t)m, 0u, (unsigned)(32 + 2 * k), stream);
    if (he != hipSuccess) return he;
    void *tmp = nullptr;
    he = hipMalloc(&tmp, bytes > 0 ? bytes : 256);
    if (he != hipSuccess) return he;
    he = rocprim::radix_sort_keys(tmp, bytes, entries, sorted, (size_t)m, 0u, (unsigned)(32 + 2 * k), stream);
    const hipError_t se = hipStreamSynchronize(stream); // (the storage is in use until the sort is done)
    (void)hipFree(tmp);
    return he != hipSuccess ? he : se;
}

hipError_t launch_index_split(const uint64_t *sorted, const int64_t m, uint32_t *keys, int32_t *pos, hipStream_t stream)
{
    if (m < 1) return hipSuccess;
    if (!sorted || !keys || !pos) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_index_split_kernel, dim3((unsigned)index_grid(m, 256)), dim3(256), 0, stream, sorted, m, keys, pos);
    return hipGetLastError();
}

hipError_t launch_index_buckets(const uint32_t *keys, const int64_t m, const int k, const int bucket_bits, uint32_t *bucket, hipStream_t stream)
{
    if (m < 0 || (m > 0 && !keys) || !bucket || bucket_bits < 1 || bucket_bits > INDEX_MAX_BUCKET_BITS || bucket_bits > 2 * k) return hipErrorInvalidValue;
    const int64_t buckets = (int64_t)1 << bucket_bits;
    hipLaunchKernelGGL(sw_index_bucket_kernel, dim3((unsigned)index_grid(buckets + 1, 256)), dim3(256), 0, stream, keys, m, 2 * k - bucket_bits, buckets, bucket);
    return hipGetLastError();
}

hipError_t launch_seed_index(const SeedIndexArgs &aa, hipStream_t stream)
{
    const SeedStageArgs &a = aa.s;
    if (a.n < 1) return hipSuccess;
    if ((aa.strands != 1 && aa.strands != 2) || a.n > SEED_MAX_PAIRS || a.n % aa.strands || a.groups < 1) return hipErrorInvalidValue;
    if (aa.ix.k < SEED_MIN_K || aa.ix.k > SEED_MAX_K || aa.ix.w < 1 || aa.ix.w > SEED_MAX_W || !aa.ix.bucket || (aa.ix.entries > 0 && (!aa.ix.keys || !aa.ix.pos)))
        return hipErrorInvalidValue;
    if (a.max_occ < 1 || a.max_occ > SEED_MAX_OCC || aa.max_occ_ref < 1 || aa.max_occ_ref > INDEX_MAX_OCC_REF || a.max_cand < 1 || a.max_cand > SEED_MAX_CAND)
        return hipErrorInvalidValue;
    if (!a.ws) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_seed_index_kernel, dim3((unsigned)a.groups), dim3(SEED_THREADS), 0, stream, aa);
    return hipGetLastError();
}

hipError_t launch_locate_window(const LocateArgs &a, hipStream_t stream)
{
    if (a.n < 1) return hipSuccess;
    if (!a.q_len || !a.anchor_start || !a.anchor_t || !a.anchor_q || !a.anchor_len || !a.t_start || !a.t_len || !a.anchor_t_out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_locate_window_kernel, dim3((unsigned)index_grid(a.n, 1)), dim3(64), 0, stream, a);
    return hipGetLastError();
}

static bool contig_view_ok(const ContigView &cv)
{
    return cv.ref_len >= 1 && cv.n >= 0 && cv.n <= CONTIG_MAX && (cv.n == 0 || (cv.start && cv.end));
}

hipError_t launch_contig_gaps(const uint8_t *ref, const ContigView &cv, int32_t *flag, hipStream_t stream)
{
    if (cv.n < 2) return hipSuccess;
    if (!ref || !flag || !contig_view_ok(cv)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_contig_gap_kernel, dim3((unsigned)(cv.n - 1)), dim3(256), 0, stream, ref, cv, flag);
    return hipGetLastError();
}

hipError_t launch_contig_of(const ContigOfArgs &a, hipStream_t stream)
{
    if (a.total < 1) return hipSuccess;
    if (a.total > SEED_MAX_PAIRS || !a.t || !a.len || !a.group || !contig_view_ok(a.cv)) return hipErrorInvalidValue;
    // a workgroup stages the table once and then strides over the anchors: no more workgroups than keep the device busy
    const int64_t blocks = (a.total + 255) / 256;
    const dim3 grid((unsigned)(blocks < 4096 ? blocks : 4096));
    if (a.cv.n <= CONTIG_LDS_MAX) hipLaunchKernelGGL(sw_contig_of_kernel<true>, grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(sw_contig_of_kernel<false>, grid, dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_locate_window_contigs(const LocateContigsArgs &aa, hipStream_t stream)
{
    const LocateArgs &a = aa.l;
    if (a.n < 1) return hipSuccess;
    if (!a.q_len || !a.anchor_start || !a.anchor_t || !a.anchor_q || !a.anchor_len || !a.t_start || !a.t_len || !a.anchor_t_out || !aa.rid) return hipErrorInvalidValue;
    if (!contig_view_ok(aa.cv)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_locate_window_contigs_kernel, dim3((unsigned)index_grid(a.n, 1)), dim3(64), 0, stream, aa);
    return hipGetLastError();
}

} // namespace mgl_sw_dev
