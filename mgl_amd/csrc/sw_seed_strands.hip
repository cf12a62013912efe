// sw_seed_strands.hip -- the kernels of mgl_sw_seed_strands_batch_device and mgl_sw_select_strand_batch_device (DESIGN.md section 9i;
// the function is tests/strand_textbook.py's).  sw_seed_strands.h describes the workspaces they share with the host side.
//
// sw_seed_strands_kernel: sw_seed_kernel's scheme (sw_seed.hip: a workgroup of 256 threads per pair, persistent; a sequence sketched
// SEED_BLOCK positions at a time) over the two ROWS of a pair, (T, Q) and (T, rc(Q)):
//   (a) two tables, one per orientation of the read, each as (key << 32 | position) and bitonic-sorted.  The reverse one is sketched from
//       the read's bytes where they lie: byte i of rc(Q) is read at ql - 1 - i and its code is 3 - c.  Everything behind that load works
//       in the oriented read's coordinates, so the tie rule "smallest position" and the block seams are the oriented read's by
//       construction;
//   (b) the window is read and sketched ONCE: a block's selected positions stay in LDS (flag, key) while they are probed against the
//       forward table and then against the reverse one, each row with its own hits, its own count and its own refusal;
//   (c), (d) per row as in sw_seed_kernel: the merge and the row's staging.  Both tables are dead by then: the runs of either row go
//       where the two tables were.
// A table lives in LDS up to STRAND_LDS_TAB entries and a row's hits up to STRAND_LDS_HITS; beyond that in the row's half of the
// workgroup's slot.  Where each lives follows from its size alone, so no pointer is carried between the phases.
// The rows' counts, staging and statuses are laid out as sw_seed_scan_kernel and sw_seed_pack_kernel read them: the host side runs
// those two over the 2n rows.
//
// sw_select_strand_kernel (a thread per pair: the checks, the strand, K_p), sw_select_strand_scan_kernel (one block, the prefix sum of
// K_p with a running carry, 1024 pairs a step) and sw_select_strand_pack_kernel (a wave per pair: the chosen row's anchors and the
// oriented read, in 4-byte stores between the unaligned ends).
#include "sw_seed_sketch.h"
#include "sw_seed_strands.h"

namespace mgl_sw_dev {

namespace {

__shared__ uint64_t s_tab[2][STRAND_LDS_TAB];   // sw_seed_strands_kernel's alone, and s_hits.  By orientation; (c) reuses both as one area
__shared__ uint64_t s_hits[2][STRAND_LDS_HITS]; // by row
static_assert(sizeof(SeedSketchLds) + sizeof(s_tab) + sizeof(s_hits) <= 80 * 1024, "two workgroups share a CU's 160 KiB of LDS");
static_assert(2 * STRAND_LDS_TAB * 8 >= STRAND_LDS_HITS * 12, "the runs and their lengths fit where the two tables were");

__global__ __launch_bounds__(SEED_THREADS) void sw_seed_strands_kernel(const SeedStrandsArgs aa)
{
    const SeedStageArgs &a = aa.s;
    const int tid = threadIdx.x;
    const int k = a.k, w = a.w;
    const SeedWorkspace sg = seed_workspace(a.n, a.max_cand); // (a.n: the rows)
    int32_t *const count = reinterpret_cast<int32_t *>(a.ws + sg.count), *const stage = reinterpret_cast<int32_t *>(a.ws + sg.stage);
    unsigned char *const slot = a.ws + sg.bytes + (int64_t)blockIdx.x * 2 * sg.slot_bytes;
    const int pairs = (int)(a.n >> 1);

    for (int p = blockIdx.x; p < pairs; p += a.groups) {
        __syncthreads(); // (the pair before this one is done with LDS)
        const int tl = a.t_len[p], ql = a.q_len[p];
        const int64_t row = 2 * (int64_t)p;
        if (tid < 2) {
            if (aa.row_t_len) aa.row_t_len[row + tid] = tl;
            if (aa.row_q_len) aa.row_q_len[row + tid] = ql;
        }
        auto finish = [&](const int r, const int n_cand, const int status) {
            if (tid != 0) return;
            count[row + r] = n_cand;
            if (a.status) a.status[row + r] = status;
        };
        if (tl < 1 || ql < 1) {
            finish(0, 0, SEED_ST_BAD_ARG);
            finish(1, 0, SEED_ST_BAD_ARG);
            continue;
        }
        const uint8_t *const T = a.targets + a.t_start[p], *const Q = a.queries + a.q_start[p];
        const int nkq = ql - k + 1, nkt = tl - k + 1;

        // ---- (a) the two tables.  nq < 0: the row is refused; nq = 0: no key to meet, no hit.  The loops over the two rows stay loops, and a
        // row's state is picked by hand: the phases are inlined once each, and only leaves are called (no frame, no scratch)
        int nq0 = 0, nq1 = 0, R0 = 0, R1 = 0;
#pragma nounroll
        for (int r = 0; r < 2; ++r) {
            const int nq = seed_build_table(Q, nkq, k, w, r == 1, s_tab[r], reinterpret_cast<uint64_t *>(slot + r * sg.slot_bytes), STRAND_LDS_TAB);
            if (r) nq1 = nq;
            else nq0 = nq;
        }

        // ---- (b) the window's sketch, once, against both.  R < 0: the row is refused
        if (nq0 > 0 || nq1 > 0)
            for (uint32_t p0 = 0; (int64_t)p0 < nkt; p0 += SEED_BLOCK) {
                const int64_t lo = seed_sketch_block(T, nkt, k, w, p0, false);
#pragma nounroll
                for (int r = 0; r < 2; ++r) {
                    const int nq = r ? nq1 : nq0, R = r ? R1 : R0;
                    if (nq <= 0 || R < 0) continue;
                    unsigned char *const half = slot + r * sg.slot_bytes;
                    const uint64_t *const tab = nq > STRAND_LDS_TAB ? reinterpret_cast<const uint64_t *>(half) : s_tab[r];
                    const int Rn = seed_probe_block(tab, nq, s_hits[r], reinterpret_cast<uint64_t *>(half + SEED_SLOT_TAB), STRAND_LDS_HITS, R, p0, lo, a.max_occ,
                                                    a.max_cand);
                    if (r) R1 = Rn;
                    else R0 = Rn;
                }
                if ((nq0 <= 0 || R0 < 0) && (nq1 <= 0 || R1 < 0)) break;
            }

        // ---- (c), (d) per row
#pragma nounroll
        for (int r = 0; r < 2; ++r) {
            const int nq = r ? nq1 : nq0, R = r ? R1 : R0;
            if (nq < 0 || R < 0) {
                finish(r, 0, SEED_ST_UNSUPPORTED);
                continue;
            }
            unsigned char *const half = slot + r * sg.slot_bytes;
            const bool in_lds = R <= STRAND_LDS_HITS;
            uint64_t *const hits = in_lds ? s_hits[r] : reinterpret_cast<uint64_t *>(half + SEED_SLOT_TAB);
            uint64_t *const run = in_lds ? &s_tab[0][0] : reinterpret_cast<uint64_t *>(half);
            uint32_t *const len = in_lds ? reinterpret_cast<uint32_t *>(&s_tab[0][0] + STRAND_LDS_HITS) : reinterpret_cast<uint32_t *>(half + SEED_SLOT_LEN);
            const int N = seed_stage_row<true>(hits, R, run, len, stage + (row + r) * 3 * a.max_cand, a.max_cand, k, a.merge);
            __syncthreads(); // (the next row's runs go to the same place)
            finish(r, N, 0);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- the choice

__global__ __launch_bounds__(256) void sw_select_strand_kernel(const SelectStrandArgs a)
{
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < a.n; p += (int64_t)gridDim.x * 256) {
        const int64_t ql = a.q_len[p], qs = a.q_start[p];
        const int64_t c0 = a.chain_start[2 * p], c1 = a.chain_start[2 * p + 1], c2 = a.chain_start[2 * p + 2];
        const bool bad = ql < 1 || qs < 0 || qs > a.query_bytes - ql || c0 < 0 || c1 < c0 || c2 < c1 || c2 > a.total_chain;
        const int K0 = (int)(c1 - c0), K1 = (int)(c2 - c1); // (total_chain <= 2^30)
        const int s0 = !bad && K0 > 0 ? a.chain_score[2 * p] : 0, s1 = !bad && K1 > 0 ? a.chain_score[2 * p + 1] : 0;
        const int strand = s1 > s0 ? 1 : 0;
        a.count[p] = bad ? -1 : strand ? K1 : K0;
        a.strand[p] = strand;
        if (a.score) a.score[p] = strand ? s1 : s0;
        if (a.status) a.status[p] = bad ? SEED_ST_BAD_ARG : 0;
    }
}

__global__ __launch_bounds__(1024) void sw_select_strand_scan_kernel(const SelectStrandArgs a)
{
    __shared__ int64_t wave_sum[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t carry = 0;
    for (int64_t base = 0; base < a.n; base += 1024) {
        const int64_t p = base + tid;
        const int cnt = p < a.n ? a.count[p] : 0;
        const int64_t own = cnt > 0 ? cnt : 0;
        const int64_t incl = wave_inclusive_sum(own);
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        int64_t before = carry, all = 0;
        for (int x = 0; x < 16; ++x) {
            const int64_t sum = wave_sum[x];
            before += x < wave ? sum : 0;
            all += sum;
        }
        __syncthreads();
        if (p < a.n) a.anchor_start[p] = before + incl - own;
        carry += all;
    }
    if (tid == 0) a.anchor_start[a.n] = carry;
}

__device__ inline uint8_t strand_comp(const uint8_t b) { return b == 'A' ? 'T' : b == 'T' ? 'A' : b == 'C' ? 'G' : b == 'G' ? 'C' : b; }

__global__ __launch_bounds__(64) void sw_select_strand_pack_kernel(const SelectStrandArgs a)
{
    const int lane = threadIdx.x;
    for (int64_t p = blockIdx.x; p < a.n; p += gridDim.x) {
        const int cnt = a.count[p];
        if (cnt < 0) continue; // a refused pair: neither anchors nor bytes
        const int strand = a.strand[p];
        const int64_t from = a.chain_start[2 * p + strand], at = a.anchor_start[p];
        // (sw_select_strand_kernel checked `from`; ranges that are valid one by one but overlap can add up to more than the capacity)
        if (at + cnt <= a.total_chain)
            for (int m = lane; m < cnt; m += 64) {
                a.anchor_t[at + m] = a.chain_t[from + m];
                a.anchor_q[at + m] = a.chain_q[from + m];
                a.anchor_len[at + m] = a.chain_len[from + m];
            }
        // the oriented read: single bytes up to the first 4-aligned address of the output, whole words, single bytes behind the last
        const int ql = a.q_len[p];
        const uint8_t *const src = a.queries + a.q_start[p];
        uint8_t *const dst = a.queries_out + a.q_start[p];
        auto oriented = [&](const int i) -> uint32_t { return strand ? strand_comp(src[ql - 1 - i]) : src[i]; };
        const int to_aligned = (int)(-reinterpret_cast<uintptr_t>(dst) & 3);
        const int head = to_aligned < ql ? to_aligned : ql, words = (ql - head) >> 2, tail = head + 4 * words;
        if (lane < head) dst[lane] = (uint8_t)oriented(lane);
        uint32_t *const dst4 = reinterpret_cast<uint32_t *>(dst + head);
        for (int x = lane; x < words; x += 64) {
            const int i = head + 4 * x;
            dst4[x] = oriented(i) | oriented(i + 1) << 8 | oriented(i + 2) << 16 | oriented(i + 3) << 24;
        }
        if (lane < ql - tail) dst[tail + lane] = (uint8_t)oriented(tail + lane);
    }
}

} // namespace

hipError_t launch_seed_strands(const SeedStrandsArgs &aa, hipStream_t stream)
{
    const SeedStageArgs &a = aa.s;
    if (a.n < 1) return hipSuccess;
    if (a.n > 2 * STRAND_MAX_PAIRS || (a.n & 1) || a.groups < 1 || a.k < SEED_MIN_K || a.k > SEED_MAX_K || a.w < 1 || a.w > SEED_MAX_W) return hipErrorInvalidValue;
    if (a.max_occ < 1 || a.max_occ > SEED_MAX_OCC || a.max_cand < 1 || a.max_cand > SEED_MAX_CAND) return hipErrorInvalidValue;
    if (!a.ws) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_seed_strands_kernel, dim3((unsigned)a.groups), dim3(SEED_THREADS), 0, stream, aa);
    return hipGetLastError();
}

hipError_t launch_select_strand(const SelectStrandArgs &a, hipStream_t stream)
{
    if (a.n < 1) return hipSuccess;
    if (a.n > STRAND_MAX_PAIRS || !a.count || !a.strand) return hipErrorInvalidValue;
    const int64_t blocks = (a.n + 255) / 256;
    hipLaunchKernelGGL(sw_select_strand_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_select_strand_scan(const SelectStrandArgs &a, hipStream_t stream)
{
    if (a.n < 0 || a.n > STRAND_MAX_PAIRS || !a.anchor_start || (a.n > 0 && !a.count)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_select_strand_scan_kernel, dim3(1), dim3(1024), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_select_strand_pack(const SelectStrandArgs &a, hipStream_t stream)
{
    if (a.n < 1) return hipSuccess;
    if (!a.count || !a.strand || !a.anchor_start || !a.queries_out) return hipErrorInvalidValue;
    const int64_t grid = a.n < 65536 ? a.n : 65536;
    hipLaunchKernelGGL(sw_select_strand_pack_kernel, dim3((unsigned)grid), dim3(64), 0, stream, a);
    return hipGetLastError();
}

} // namespace mgl_sw_dev
