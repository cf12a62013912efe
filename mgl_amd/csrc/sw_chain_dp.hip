// sw_chain_dp.hip -- the three kernels of mgl_sw_chain_anchors_batch_device and of its grouped form (DESIGN.md sections 9g and 9m; the
// functions are tests/chain_dp_textbook.py's and tests/contig_textbook.py's chain_dp_grouped).  sw_chain_dp.h describes the workspace they share with the host side.
//
// sw_chain_dp_kernel, the hot path: one wave per read, persistent over the reads.  The FORWARD form of the DP: the 64 lanes are a
// ring, lane i mod 64 owns candidate i while its predecessors j = i - 64 .. i - 1 go by.  Step j: f(j) is final in lane j mod 64 --
// every j' < j has gone by -- and f(j), t_j + l_j and q_j + l_j are read from that lane at a wave-uniform index.  The lane keeps
// (f(j), pred(j)) aside, takes candidate j + 64 with f = l and pred = -1, and then every lane offers j to the candidate it owns: the
// lanes own j + 1 .. j + 64 now, so the distance i - j is 1 .. 64 and max_pred = 64 needs no second ring.  A lane replaces on `>=`
// while j ascends, which is "ties to the largest j, no predecessor counts as -1".  There is no reduction and no memory access inside
// a block of 64 steps: the candidates of the next block were loaded (coalesced, 64 at once) one block earlier, those of the block
// after it are requested at the block's start, and what the 64 lanes kept aside is stored (coalesced) at the block's end: f and pred to
// the caller's arrays, i - pred as a byte where the trace-back chases it -- LDS, or the wave's workspace slot where max_cand is above
// CHAIN_DP_LDS_PRED.  Each lane keeps the arg-max of the f it finalised (first wins: its indices ascend); one reduction at the read's
// end picks the largest f and, among equals, the smallest index.  The same wave then walks pred back and writes the chain, last
// anchor first, into the read's staging.  All candidates of a read are checked, 64 at a time, before the DP starts: a refused read
// writes nothing but its status, count and score.
//
// sw_chain_dp_scan_kernel: one block, the exclusive prefix sum of the counts into d_chain_start_out, 1024 reads a step.
// sw_chain_dp_pack_kernel: one wave per read, 64 anchors a step from the staging (reversed) into the read's CSR place.
#include "sw_band_wave.h"
#include "sw_chain_dp.h"

namespace mgl_sw_dev {

namespace {

// GROUPED (mgl_sw_chain_anchors_grouped_batch_device): j may precede i only where both have the same group >= 0.  A lane carries its
// candidate's group beside t, q and l, and the groups of the next two blocks beside nt and mt; a step reads j's from its lane.
template <bool GROUPED>
__global__ __launch_bounds__(64) void sw_chain_dp_kernel(const ChainDpArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_pred[];
    const int lane = threadIdx.x;
    const bool in_lds = a.slot_bytes == 0;
    unsigned char *const slot = in_lds ? nullptr : a.ws + (int64_t)blockIdx.x * a.slot_bytes;
    const int max_pred = a.max_pred, mdt = a.max_dist_t, mdq = a.max_dist_q, bw = a.bw;
    const uint32_t pen_gap = (uint32_t)a.pen_gap, pen_skip = (uint32_t)a.pen_skip;

    for (int64_t p = blockIdx.x; p < a.n; p += a.waves) {
        const int tl = a.t_len[p], ql = a.q_len[p];
        const int64_t c0 = a.cand_start[p], c1 = a.cand_start[p + 1];
        auto refuse = [&](const int status) {
            if (lane != 0) return;
            a.count[p] = 0;
            a.chain_score[p] = 0;
            if (a.status) a.status[p] = status;
        };
        if (c0 < 0 || c1 < c0 || c1 > a.total_cand || tl < 1 || ql < 1) {
            refuse(ST_BAD_ARG);
            continue;
        }
        const int64_t cnt = c1 - c0;
        bool bad = false;
        for (int64_t i = c0 + lane; i < c1; i += 64) {
            const int t = a.cand_t[i], q = a.cand_q[i], l = a.cand_len[i];
            bad |= !(l >= 1 && t >= 0 && q >= 0 && (int64_t)t + l <= tl && (int64_t)q + l <= ql);
        }
        if (__ballot(bad)) {
            refuse(ST_BAD_ARG);
            continue;
        }
        if (cnt > a.max_cand) {
            refuse(ST_UNSUPPORTED);
            continue;
        }
        const int N = (int)cnt;
        if (N == 0) {
            refuse(0);
            continue;
        }
        const int32_t *const ct = a.cand_t + c0, *const cq = a.cand_q + c0, *const cl = a.cand_len + c0;
        [[maybe_unused]] const int32_t *const cg = GROUPED ? a.cand_group + c0 : nullptr;
        __threadfence_block(); // (the trace-back of the wave's last read is done with the pred bytes)
        __builtin_amdgcn_wave_barrier();

        // the candidate the lane owns (idx, its f and pred so far), the one it takes next (n*) and the one after that (m*)
        int idx = lane;
        int t = 0, q = 0, l = 0, nt = 0, nq = 0, nl = 0;
        if (idx < N) t = ct[idx], q = cq[idx], l = cl[idx];
        if (idx + 64 < N) nt = ct[idx + 64], nq = cq[idx + 64], nl = cl[idx + 64];
        [[maybe_unused]] int g = -1, ng = -1;
        if constexpr (GROUPED) {
            if (idx < N) g = cg[idx];
            if (idx + 64 < N) ng = cg[idx + 64];
        }
        int f = l, pred = -1;
        int best_f = 0, best_i = 0;
        for (int base = 0; base < N; base += 64) {
            int mt = 0, mq = 0, ml = 0;
            if (base + 128 + lane < N) mt = ct[base + 128 + lane], mq = cq[base + 128 + lane], ml = cl[base + 128 + lane];
            [[maybe_unused]] int mg = -1;
            if constexpr (GROUPED)
                if (base + 128 + lane < N) mg = cg[base + 128 + lane];
            int fin_f = 0, fin_p = -1;
            const int steps = min(64, N - base);
            for (int s = 0; s < steps; ++s) {
                const int j = base + s;
                const int fj = __builtin_amdgcn_readlane(f, s);
                const int lj = __builtin_amdgcn_readlane(l, s);
                const int te = __builtin_amdgcn_readlane(t, s) + lj, qe = __builtin_amdgcn_readlane(q, s) + lj;
                [[maybe_unused]] int gj = 0;
                if constexpr (GROUPED) gj = __builtin_amdgcn_readlane(g, s);
                if (lane == s) { // f(j) is final: kept aside, and the lane takes candidate j + 64
                    fin_f = f;
                    fin_p = pred;
                    const bool up = f > best_f;
                    best_f = up ? f : best_f;
                    best_i = up ? j : best_i;
                    t = nt;
                    q = nq;
                    l = nl;
                    if constexpr (GROUPED) g = ng;
                    f = nl;
                    pred = -1;
                    idx += 64;
                }
                // j offered to the lane's candidate; unsigned where a lane that fails the mask may wrap
                const int dt = (int)((uint32_t)t - (uint32_t)te), dq = (int)((uint32_t)q - (uint32_t)qe);
                const int diff = (int)((uint32_t)dt - (uint32_t)dq);
                const uint32_t dd = (uint32_t)(diff < 0 ? -diff : diff);
                bool ok = idx < N && idx - j <= max_pred && dt >= 0 && dq >= 0 && dt <= mdt && dq <= mdq && dd <= (uint32_t)bw;
                if constexpr (GROUPED) ok = ok && g == gj && g >= 0;
                const uint32_t dg = (uint32_t)(dt < dq ? dt : dq);
                const int pen = (int)((pen_gap * dd + pen_skip * dg) >> 8) + ((31 - __clz((int)(dd + 1u))) >> 1);
                const int cand = (int)((uint32_t)fj + (uint32_t)l - (uint32_t)pen);
                const bool take = ok && cand >= f;
                f = take ? cand : f;
                pred = take ? j : pred;
            }
            // the block's 64 results, coalesced
            if (base + lane < N) {
                const unsigned char back = (unsigned char)(fin_p < 0 ? 0 : base + lane - fin_p);
                if (in_lds) lds_pred[base + lane] = back;
                else slot[base + lane] = back;
                if (a.f_out) a.f_out[c0 + base + lane] = fin_f;
                if (a.pred_out) a.pred_out[c0 + base + lane] = fin_p;
            }
            nt = mt;
            nq = mq;
            nl = ml;
            if constexpr (GROUPED) ng = mg;
        }

        // ---- the chain's end: the largest f, then the smallest index
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const int of = __shfl_xor(best_f, m), oi = __shfl_xor(best_i, m);
            const bool up = of > best_f || (of == best_f && oi < best_i);
            best_f = up ? of : best_f;
            best_i = up ? oi : best_i;
        }
        if (in_lds) __threadfence_block(); // the pred bytes before the walk reads them
        else __threadfence();
        __builtin_amdgcn_wave_barrier();

        // ---- the walk, the same in every lane; lane 0 writes
        int32_t *const stage = a.stage + c0;
        int k = 0;
        for (int i = best_i; k < N;) {
            if (lane == 0) stage[k] = i;
            ++k;
            const int back = in_lds ? lds_pred[i] : __hip_atomic_load(slot + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (back == 0 || back > i) break; // (back <= i: pred >= 0)
            i -= back;
        }
        if (lane == 0) {
            a.count[p] = k;
            a.chain_score[p] = best_f;
            if (a.status) a.status[p] = 0;
        }
    }
}

__global__ __launch_bounds__(1024) void sw_chain_dp_scan_kernel(const ChainDpArgs a)
{
    __shared__ int64_t wave_sum[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t carry = 0;
    for (int64_t base = 0; base < a.n; base += 1024) {
        const int64_t p = base + tid;
        const int64_t own = p < a.n ? a.count[p] : 0;
        int64_t incl = own;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        int64_t before = carry, all = 0;
        for (int w = 0; w < 16; ++w) {
            const int64_t s = wave_sum[w];
            before += w < wave ? s : 0;
            all += s;
        }
        if (p < a.n) a.chain_start[p] = before + incl - own;
        carry += all;
        __syncthreads();
    }
    if (tid == 0) a.chain_start[a.n] = carry;
}

__global__ __launch_bounds__(64) void sw_chain_dp_pack_kernel(const ChainDpArgs a)
{
    const int lane = threadIdx.x;
    for (int64_t p = blockIdx.x; p < a.n; p += gridDim.x) {
        const int64_t at = a.chain_start[p];
        const int k = a.count[p];
        if (k == 0) continue;
        const int64_t c0 = a.cand_start[p]; // (a read with a chain passed the range check)
        const int32_t *const stage = a.stage + c0;
        for (int m = lane; m < k; m += 64) {
            const int64_t src = c0 + stage[k - 1 - m], dst = at + m;
            if (src < 0 || src >= a.total_cand || dst >= a.total_cand) continue; // (ranges that overlap: sw_chain_dp.h)
            a.chain_t[dst] = a.cand_t[src];
            a.chain_q[dst] = a.cand_q[src];
            a.chain_len[dst] = a.cand_len[src];
        }
    }
}

} // namespace

hipError_t launch_chain_dp(const ChainDpArgs &a, hipStream_t stream)
{
    if (a.n < 1) return hipSuccess;
    if (a.n > CHAIN_DP_MAX_CHUNK || a.total_cand > CHAIN_DP_MAX_CHUNK || a.waves < 1 || a.max_pred < 1 || a.max_pred > CHAIN_DP_MAX_PRED) return hipErrorInvalidValue;
    if (!a.count || !a.stage || !a.chain_score || !a.cand_start) return hipErrorInvalidValue;
    // where pred lives: LDS that holds max_cand bytes, or a slot that does
    if (a.slot_bytes == 0 ? (a.lds_bytes < a.max_cand || a.lds_bytes > CHAIN_DP_LDS_PRED) : (!a.ws || a.slot_bytes < a.max_cand)) return hipErrorInvalidValue;
    if (a.cand_group) hipLaunchKernelGGL(sw_chain_dp_kernel<true>, dim3((unsigned)a.waves), dim3(64), (size_t)a.lds_bytes, stream, a);
    else hipLaunchKernelGGL(sw_chain_dp_kernel<false>, dim3((unsigned)a.waves), dim3(64), (size_t)a.lds_bytes, stream, a);
    return hipGetLastError();
}

hipError_t launch_chain_dp_scan(const ChainDpArgs &a, hipStream_t stream)
{
    if (a.n < 0 || a.n > CHAIN_DP_MAX_CHUNK || !a.chain_start || (a.n > 0 && !a.count)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_chain_dp_scan_kernel, dim3(1), dim3(1024), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_chain_dp_pack(const ChainDpArgs &a, hipStream_t stream)
{
    if (a.n < 1 || a.total_cand < 1) return hipSuccess;
    if (!a.count || !a.stage || !a.chain_start || !a.chain_t || !a.chain_q || !a.chain_len) return hipErrorInvalidValue;
    const int64_t grid = a.n < 65536 ? a.n : 65536;
    hipLaunchKernelGGL(sw_chain_dp_pack_kernel, dim3((unsigned)grid), dim3(64), 0, stream, a);
    return hipGetLastError();
}

} // namespace mgl_sw_dev
