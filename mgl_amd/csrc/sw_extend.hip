// sw_extend.hip -- sw_extend_kernel, the kernel of mgl_sw_extend_batch_device: extension from an anchored start (0, 0) to a free end
// over the band -band <= j - i <= band, with the Z-drop rule (the function is tests/extend_textbook.py's, which
// the tests compare with).
//
// The mapping is sw_banded.hip's, and the sweep, the decision bits, the walk and the CIGAR output are the same code: sw_band_wave.h,
// which both files include and which describes them.
//
// What is new: a lane owns one row of the strip, so it keeps that row's running maximum and the step at which it first appeared (the
// border column seeds it where that is in the band), and the lane on column ql keeps H(i, ql).  After a strip the wave takes an
// inclusive prefix of (H, i, j) over the lanes in row order -- strict, so that earlier rows win --, lane 0's element folded with the
// running best of the strips above; every lane tests the drop predicate of its row against the exclusive prefix, and one ballot finds
// the first dropping row.  Lanes from there on, and rows past tl, stay out of the best cell and of score_qend, and the wave leaves the
// pair's remaining strips undone.
#include "sw_band_wave.h"
#include "sw_extend.h"

namespace mgl_sw_dev {

namespace {

__global__ __launch_bounds__(64) void sw_extend_kernel(const ExtendArgs a)
{
    const int lane = threadIdx.x;
    const int o = a.gopen, e = a.gext;
    unsigned char *const slot = a.ws + (int64_t)blockIdx.x * a.slot_bytes;

    for (int64_t p = blockIdx.x; p < a.n; p += a.slots) {
        const int tl = a.t.len[p], ql = a.q.len[p];
        Extension ex{0, 0, 0, 0, 0, 0, 0, 0};
        auto finish = [&](const int status, const int cigar_len) {
            if (lane != 0) return;
            a.ext[p] = status ? Extension{0, 0, 0, 0, 0, 0, 0, 0} : ex;
            if (a.status) a.status[p] = status;
            if (a.cigar_len) a.cigar_len[p] = cigar_len;
        };
        if (tl < 1 || ql < 1 || tl > a.max_tl || ql > a.max_ql) {
            finish(ST_BAD_ARG, 0);
            continue;
        }
        if (!banded_range_ok(tl, ql, a.match, a.mismatch, o, e) || extend_pair_bytes(tl, ql, a.band, a.score_only != 0) > a.slot_bytes) {
            finish(ST_UNSUPPORTED, 0);
            continue;
        }
        const int lo = -a.band, hi = a.band;
        int2 *const carry = reinterpret_cast<int2 *>(slot);
        uint32_t *const elems = reinterpret_cast<uint32_t *>(slot + banded_carry_bytes(ql));
        uint32_t *const dir = reinterpret_cast<uint32_t *>(slot + banded_carry_bytes(ql) + banded_elem_bytes(tl, ql));
        const int64_t strip_words = (int64_t)extend_strip_steps(ql, a.band) * 8;
        const int64_t ts = a.t.off[p];
        const unsigned char *const tq = a.q.data + a.q.off[p];

        // row 0: the border's H and the E that enters row 1, minus infinity beyond the band
        for (int j = lane; j <= ql; j += 64) {
            const int b = border(j, o, e, true); // the anchored start: always a gap penalty
            carry[j] = j <= hi ? make_int2(b, b - o) : make_int2(NEG, NEG);
        }
        __threadfence_block();
        __builtin_amdgcn_wave_barrier();

        const int rows = min(tl, ql + hi); // rows beyond have no cell in the band
        int bh = 0, bi = 0, bj = 0;        // best(i) of the rows done so far: (0, 0) is the empty extension
        int mq = EXTEND_NO_QEND, mqt = -1; // the lane's last-column best: later rows win ties
        int rows_done = tl, dropped = 0;
        const int strips = (rows + 63) / 64;
        for (int k = 0; k < strips; ++k) {
            // the strip as strip_setup() of sw_band_wave.h fills it (borders always gap penalties), plus s_span, written out: called
            // as a function here, the setup reaches the compiler with other wrap flags, and this kernel, allocated anew, takes a
            // 163rd VGPR and 2 to 10 more instructions per unrolled sweep body (docs/history.md C.000000)
            const int i = 64 * k + lane + 1;
            const bool rowv = i <= rows, last = k + 1 == strips;
            Strip st;
            st.c0 = max(1, 64 * k + 1 + lo);
            const int c1 = min(ql, 64 * k + 64 + hi);
            st.steps = (c1 - st.c0 + 64 + 7) & ~7;
            st.tc = rowv ? a.t.data[ts + i - 1] : 0x100;
            const int jlo = max(1, i + lo);
            st.s_first = jlo - st.c0 + lane;
            st.s_first0 = jlo == 1 ? st.s_first : NEVER;
            st.s_top = i + hi - st.c0 + lane;
            st.s_span = min(i + hi, ql) - jlo; // (a row past `rows` may get any window, a negative span read as unsigned included: rowv keeps it out of every result)
            st.s_last = rowv && i + hi >= ql ? ql - st.c0 + lane : NEVER;
            st.f_init = i + lo <= 0 ? border(i, o, e, true) - o : NEG; // (i, 0) is in the band: F[i][1] = H[i][0] - o
            st.p_init = border(i - 1, o, e, true);
            st.w_lane = last ? (rows - 1) & 63 : 63;
            st.w_first = __builtin_amdgcn_readlane(st.s_first, st.w_lane);
            st.w_last = min(__builtin_amdgcn_readlane(st.s_top, st.w_lane), ql - st.c0 + st.w_lane);
            st.carry = carry;
            st.q = tq;
            st.ql = ql;
            st.dir = dir + (int64_t)k * strip_words + lane;
            st.col0 = st.c0 == 1;
            st.lastcol = 64 * k + 64 + hi >= ql;
            // the row's maximum starts from the border column where that is in the band (step s_first - 1), or from minus infinity
            Swept sw;
            sw.rmax = i + lo <= 0 ? border(i, o, e, true) : NEG;
            sw.rs = st.s_first - 1;
            sweep_strip<true>(st, lane, a.match, a.mismatch, o, e, !a.score_only, sw);
            __threadfence_block(); // the carry row before the next strip reads it, the decisions before the walk does
            __builtin_amdgcn_wave_barrier();

            // ---- best(i) per row: an inclusive prefix of (H, i, j) over the lanes; lane 0's element is folded with the running best
            // of the strips above first (which is earlier: it stays on a tie)
            const int rcol = st.c0 + sw.rs - lane;
            int ph = rowv ? sw.rmax : NEG, pi = i, pj = rcol;
            if (lane == 0 && !(ph > bh)) {
                ph = bh;
                pi = bi;
                pj = bj;
            }
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int oh = __shfl_up(ph, d), oi = __shfl_up(pi, d), oj = __shfl_up(pj, d);
                const bool keep = lane < d || ph > oh; // strict: the earlier rows win a tie
                ph = keep ? ph : oh;
                pi = keep ? pi : oi;
                pj = keep ? pj : oj;
            }
            // the exclusive prefix: best(i - 1) as row i sees it
            int xh = __shfl_up(ph, 1), xi = __shfl_up(pi, 1), xj = __shfl_up(pj, 1);
            if (lane == 0) {
                xh = bh;
                xi = bi;
                xj = bj;
            }
            const bool drop = rowv && a.zdrop >= 0 &&
                              (int64_t)xh - (int64_t)sw.rmax > (int64_t)a.zdrop + (int64_t)e * (int64_t)abs((i - xi) - (rcol - xj));
            const unsigned long long dm = __ballot(drop);
            const int live = dm ? __builtin_ctzll(dm) : min(64, rows - 64 * k); // the strip's rows that exist for the outputs
            if (live > 0) {
                bh = __shfl(ph, live - 1);
                bi = __shfl(pi, live - 1);
                bj = __shfl(pj, live - 1);
            }
            if (lane < live && st.s_last != NEVER && sw.h_last >= mq) {
                mq = sw.h_last;
                mqt = i;
            }
            if (dm) {
                rows_done = 64 * k + live;
                dropped = 1;
                break;
            }
        }
        if (!dropped && rows < tl && a.zdrop >= 0) { // row rows + 1 has no cell in the band: it drops whenever the rule is on
            rows_done = rows;
            dropped = 1;
        }
        // ---- the last column: the largest H, the later row among equals
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const int oq = __shfl_xor(mq, m), ot = __shfl_xor(mqt, m);
            const bool take = oq > mq || (oq == mq && ot > mqt);
            mq = take ? oq : mq;
            mqt = take ? ot : mqt;
        }
        ex.score = bh;
        ex.t_end = bi;
        ex.q_end = bj;
        ex.score_qend = mq;
        ex.t_end_qend = mqt;
        ex.rows_done = rows_done;
        ex.dropped = dropped;
        ex.cigar_from = (a.to_query_end && mqt >= 1) ? 1 : 0;
        int I = ex.cigar_from ? mqt : bi, J = ex.cigar_from ? ql : bj;
        if (a.score_only || I == 0) { // (the best cell on the border is (0, 0): the empty extension)
            finish(0, 0);
            __threadfence_block(); // (the next pair reuses the slot)
            __builtin_amdgcn_wave_barrier();
            continue;
        }

        // ---- the walk from (I, J) back to row 0 or column 0, which one closing run then leaves for (0, 0)
        const Dirs dv{dir, lo, hi, strip_words};
        Elems el{elems, lane, a.binary_cigar, 0, 0};
        const Walked w = walk(dv, lane, I, J, 0, el);
        el.push(w.state, w.seg);
        if (w.I > 0) el.push(OP_D, w.I);
        else if (w.J > 0) el.push(OP_I, w.J);
        const int cap = a.binary_cigar ? a.cigar_stride & ~3 : a.cigar_stride;
        if (el.size > cap) {
            finish(ST_CIGAR_OVERFLOW, 0);
            continue;
        }
        el.write<false>(a.cigar + p * (int64_t)a.cigar_stride);
        finish(0, el.size);
        __threadfence_block(); // (the next pair reuses the slot)
        __builtin_amdgcn_wave_barrier();
    }
}

} // namespace

// pairs 0 .. n - 1 on a.slots waves, wave w in workspace slot w
hipError_t launch_extend(const ExtendArgs &a, hipStream_t stream)
{
    if (a.n < 1) return hipSuccess;
    if (!a.ext || !a.ws || a.slots < 1 || a.slot_bytes < 256 || (!a.score_only && (!a.cigar || !a.cigar_len))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_extend_kernel, dim3((unsigned)a.slots), dim3(64), 0, stream, a);
    return hipGetLastError();
}

} // namespace mgl_sw_dev
