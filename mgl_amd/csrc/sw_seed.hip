// sw_seed.hip -- the three kernels of mgl_sw_seed_batch_device (the function is tests/seed_textbook.py's).
// sw_seed.h describes the workspace they share with the host side.
//
// sw_seed_kernel, the hot path: one workgroup of 256 threads per pair, persistent over the pairs.  A sequence is sketched SEED_BLOCK
// k-mer positions at a time: the bytes of the block and of the w - 1 positions to either side go to LDS as 2-bit codes, a thread forms key
// and hash of a position from its k codes, a thread per window takes the window's minimum from LDS (strict `<` while the position
// ascends: ties to the smallest position) and flags it, and the flagged positions of the block are compacted in order by a prefix count
// (a thread owns four neighbouring positions).  The phases are sw_seed_sketch.h's, shared with sw_seed_strands.hip and sw_index.hip:
//   (a) the query's sketch, as (key << 32 | position), bitonic-sorted (seed_build_table);
//   (b) the window's sketch, never stored, against the table: the raw hits (t << 32 | q), ascending (seed_probe_block);
//   (c) the merge of the hits on one diagonal into maximal runs, and (d) N_p and the candidates to the pair's staging (seed_stage_row).
// The table and the hits live in LDS while they fit (SEED_LDS_TAB, SEED_LDS_HITS) and in the workgroup's workspace slot when a pair
// outgrows that.
//
// sw_seed_scan_kernel: one block, the exclusive prefix sum of the counts into d_cand_start_out with a running carry, 1024 pairs a step,
// cut at the capacity.  sw_seed_pack_kernel: one wave per pair, the staging into the pair's CSR place.
#include "sw_seed_sketch.h"

namespace mgl_sw_dev {

namespace {

__shared__ uint64_t s_tab[SEED_LDS_TAB]; // sw_seed_kernel's alone, and s_hits: the other two kernels reach nothing that names them
__shared__ uint64_t s_hits[SEED_LDS_HITS];
static_assert(sizeof(SeedSketchLds) + sizeof(s_tab) + sizeof(s_hits) <= 64 * 1024, "a workgroup's LDS");
static_assert(SEED_LDS_TAB * 8 >= SEED_LDS_HITS * 12, "the runs and their lengths fit where the table was");

__global__ __launch_bounds__(SEED_THREADS) void sw_seed_kernel(const SeedStageArgs a)
{
    const int tid = threadIdx.x;
    const int k = a.k, w = a.w;
    const SeedWorkspace sg = seed_workspace(a.n, a.max_cand);
    int32_t *const count = reinterpret_cast<int32_t *>(a.ws + sg.count), *const stage = reinterpret_cast<int32_t *>(a.ws + sg.stage);
    unsigned char *const slot = a.ws + sg.bytes + (int64_t)blockIdx.x * sg.slot_bytes;
    uint64_t *const slot_tab = reinterpret_cast<uint64_t *>(slot);
    uint64_t *const slot_hits = reinterpret_cast<uint64_t *>(slot + SEED_SLOT_TAB); // (both only where max_cand is above SEED_LDS_HITS)
    uint32_t *const slot_len = reinterpret_cast<uint32_t *>(slot + SEED_SLOT_LEN);

    for (int p = blockIdx.x; p < (int)a.n; p += a.groups) { // (n <= 2^30)
        __syncthreads(); // (the pair before this one is done with LDS)
        const int tl = a.t_len[p], ql = a.q_len[p];
        auto finish = [&](const int n_cand, const int status) {
            if (tid != 0) return;
            count[p] = n_cand;
            if (a.status) a.status[p] = status;
        };
        if (tl < 1 || ql < 1) {
            finish(0, SEED_ST_BAD_ARG);
            continue;
        }
        const uint8_t *const T = a.targets + a.t_start[p], *const Q = a.queries + a.q_start[p];
        const int nkt = tl - k + 1;

        // ---- (a) nq < 0: the pair is refused; nq = 0: no key to meet, no hit
        const int nq = seed_build_table(Q, ql - k + 1, k, w, false, s_tab, slot_tab, SEED_LDS_TAB);
        if (nq <= 0) {
            finish(0, nq < 0 ? SEED_ST_UNSUPPORTED : 0);
            continue;
        }
        // ---- (b) R < 0: the pair is refused
        const uint64_t *const tab = nq > SEED_LDS_TAB ? slot_tab : s_tab;
        int R = 0;
        for (uint32_t p0 = 0; (int64_t)p0 < nkt && R >= 0; p0 += SEED_BLOCK) { // (unsigned: the step past a sequence of nearly 2^31 bytes)
            const int64_t lo = seed_sketch_block(T, nkt, k, w, p0, false);
            R = seed_probe_block(tab, nq, s_hits, slot_hits, SEED_LDS_HITS, R, p0, lo, a.max_occ, a.max_cand);
        }
        if (R < 0) {
            finish(0, SEED_ST_UNSUPPORTED);
            continue;
        }
        // ---- (c), (d) the runs go where the table was: it is not read again
        const bool in_lds = R <= SEED_LDS_HITS;
        const int N = seed_stage_row<true>(in_lds ? s_hits : slot_hits, R, in_lds ? s_tab : slot_tab,
                                           in_lds ? reinterpret_cast<uint32_t *>(s_tab + SEED_LDS_HITS) : slot_len, stage + (int64_t)p * 3 * a.max_cand,
                                           a.max_cand, k, a.merge);
        finish(N, 0);
    }
}

__global__ __launch_bounds__(1024) void sw_seed_scan_kernel(const SeedStageArgs a)
{
    __shared__ int64_t wave_sum[16];
    __shared__ int64_t cut_at; // S_(P*), or -1 while every pair fits
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int32_t *const count = reinterpret_cast<int32_t *>(a.ws + seed_workspace(a.n, a.max_cand).count);
    if (tid == 0) cut_at = -1;
    __syncthreads();
    int64_t carry = 0;
    for (int64_t base = 0; base < a.n; base += 1024) {
        const int64_t p = base + tid;
        const int64_t own = p < a.n ? count[p] : 0;
        const int64_t incl = wave_inclusive_sum(own);
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        int64_t before = carry, all = 0;
        for (int x = 0; x < 16; ++x) {
            const int64_t sum = wave_sum[x];
            before += x < wave ? sum : 0;
            all += sum;
        }
        const int64_t excl = before + incl - own, end = excl + own;
        // the sums ascend: P* is the one pair that begins inside the capacity and ends beyond it
        if (p < a.n && end > a.cand_capacity && excl <= a.cand_capacity) cut_at = excl;
        __syncthreads();
        if (p < a.n) {
            if (end <= a.cand_capacity) a.cand_start[p] = excl;
            else {
                a.cand_start[p] = cut_at;
                count[p] = 0;
                if (a.status && a.status[p] == 0) a.status[p] = SEED_ST_NOMEM;
            }
        }
        carry += all;
    }
    if (tid == 0) a.cand_start[a.n] = carry <= a.cand_capacity ? carry : cut_at;
}

__global__ __launch_bounds__(64) void sw_seed_pack_kernel(const SeedStageArgs a)
{
    const int lane = threadIdx.x;
    const SeedWorkspace sg = seed_workspace(a.n, a.max_cand);
    const int32_t *const count = reinterpret_cast<const int32_t *>(a.ws + sg.count), *const stage = reinterpret_cast<const int32_t *>(a.ws + sg.stage);
    for (int64_t p = blockIdx.x; p < a.n; p += gridDim.x) {
        const int cnt = count[p];
        if (cnt == 0) continue;
        const int64_t at = a.cand_start[p];
        const int32_t *const st = stage + p * 3 * a.max_cand, *const sq = st + a.max_cand, *const sl = sq + a.max_cand;
        if (at < 0 || at + cnt > a.cand_capacity) continue; // (the scan kept the pair: this holds)
        for (int m = lane; m < cnt; m += 64) {
            a.cand_t[at + m] = st[m];
            a.cand_q[at + m] = sq[m];
            a.cand_len[at + m] = sl[m];
        }
    }
}

} // namespace

hipError_t launch_seed(const SeedStageArgs &a, hipStream_t stream)
{
    if (a.n < 1) return hipSuccess;
    if (a.n > SEED_MAX_PAIRS || a.groups < 1 || a.k < SEED_MIN_K || a.k > SEED_MAX_K || a.w < 1 || a.w > SEED_MAX_W) return hipErrorInvalidValue;
    if (a.max_occ < 1 || a.max_occ > SEED_MAX_OCC || a.max_cand < 1 || a.max_cand > SEED_MAX_CAND) return hipErrorInvalidValue;
    if (!a.ws) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_seed_kernel, dim3((unsigned)a.groups), dim3(SEED_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_seed_scan(const SeedStageArgs &a, hipStream_t stream)
{
    if (a.n < 0 || a.n > SEED_MAX_PAIRS || !a.cand_start || (a.n > 0 && !a.ws)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_seed_scan_kernel, dim3(1), dim3(1024), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_seed_pack(const SeedStageArgs &a, hipStream_t stream)
{
    if (a.n < 1 || a.cand_capacity < 1) return hipSuccess;
    if (!a.ws || !a.cand_start || !a.cand_t || !a.cand_q || !a.cand_len) return hipErrorInvalidValue;
    const int64_t grid = a.n < 65536 ? a.n : 65536;
    hipLaunchKernelGGL(sw_seed_pack_kernel, dim3((unsigned)grid), dim3(64), 0, stream, a);
    return hipGetLastError();
}

} // namespace mgl_sw_dev
