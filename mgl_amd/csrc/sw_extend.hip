// sw_extend.hip -- sw_extend_kernel, the kernel of mgl_sw_extend_batch_device: extension from an anchored start (0, 0) to a free end
// over the band -band <= j - i <= band, with the Z-drop rule (the function is tests/extend_textbook.py's, which
// the tests compare with).
//
// The mapping is sw_banded.hip's, and the sweep, the decision bits, the walk and the CIGAR output below are that file's restated
// (a copy rather than a shared header: sw_banded_kernel's code object stays what it was): one wave per pair, int32, the 64 lanes on
// 64 consecutive target rows (a strip) on an anti-diagonal, H / E of the row above and the query byte arriving from lane l - 1 by
// wave_shr:1, lane 0 fed from the carry row in the pair's workspace slot, four decision bits per cell.
//
// What is new: a lane owns one row of the strip, so it keeps that row's running maximum and the step at which it first appeared (the
// border column seeds it where that is in the band), and the lane on column ql keeps H(i, ql).  After a strip the wave takes an
// inclusive prefix of (H, i, j) over the lanes in row order -- strict, so that earlier rows win --, lane 0's element folded with the
// running best of the strips above; every lane tests the drop predicate of its row against the exclusive prefix, and one ballot finds
// the first dropping row.  Lanes from there on, and rows past tl, stay out of the best cell and of score_qend, and the wave leaves the
// pair's remaining strips undone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sw_extend.h"

namespace mgl_sw_dev {

namespace {

constexpr int ST_BAD_ARG = 1, ST_CIGAR_OVERFLOW = 2, ST_UNSUPPORTED = 5; // mgl_sw_status
constexpr int NEG = BANDED_NEG;
constexpr int NEVER = -1; // a step number no step has

__device__ __forceinline__ int dpp_shr1(int lane0_value, int src) { return __builtin_amdgcn_update_dpp(lane0_value, src, 0x138, 0xf, 0xf, false); } // wave_shr:1, lane 0 keeps lane0_value
// wrapping arithmetic: the lanes outside the band compute on whatever they hold
__device__ __forceinline__ int wadd(int a, int b) { return (int)((unsigned)a + (unsigned)b); }
__device__ __forceinline__ int wsub(int a, int b) { return (int)((unsigned)a - (unsigned)b); }
__device__ __forceinline__ unsigned shift_in_sign(unsigned acc, int v) { return __builtin_amdgcn_alignbit(acc, (unsigned)v, 31); } // acc << 1 | v < 0

__device__ __forceinline__ int border(int k, int o, int e) { return k > 0 ? -o - (k - 1) * e : 0; } // the anchored start: always a gap penalty

__device__ __forceinline__ int digits(int v)
{
    int d = 1;
    while (v >= 10) {
        v /= 10;
        ++d;
    }
    return d;
}

// what a strip's sweep needs beside the lane's registers
struct Strip {
    int c0, steps;                 // first column, steps (a multiple of 8)
    int tc;                        // the lane's target byte
    int s_first, s_first0, s_top, s_last; // the lane's step at its first in-band column / the same where that column is 1 / on the band's upper edge / at column ql
    int s_span;                    // the lane's in-band steps are s_first .. s_first + s_span
    int f_init, p_init;            // F entering the first in-band column; H[i - 1][0]
    int w_first, w_last, w_lane;   // the writing lane and its steps in the band
    int2 *carry;
    const unsigned char *q;
    int ql;
    uint32_t *dir;                 // the strip's decisions + lane
};

// COL0: the strip has rows whose band starts at column 1 (their diagonal there is the border column's H); LASTCOL: rows that reach
// column ql (H there is kept); STORE: decisions are kept.  rmax / rs: the row's largest in-band H and the step of its first
// appearance, seeded by the caller with the border column's (step s_first - 1) or minus infinity
template <bool COL0, bool LASTCOL, bool STORE>
__device__ __forceinline__ void sweep(const Strip &st, const int lane, const int match, const int mismatch, const int o, const int e, int prev_up, int &h_last,
                                      int &rmax, int &rs)
{
    int out_h = 0, out_e = NEG, f = NEG, qc = 0;
    unsigned acc = 0;
    int2 *const wcarry = st.carry + (st.c0 - st.w_lane);
    for (int sb = 0; sb < st.steps; sb += 64) {
        // the next 64 columns of the row above the strip and of the query: lane x holds what lane 0 needs at step sb + x
        const int jb = st.c0 + sb + lane;
        int2 cb = make_int2(NEG, NEG);
        int qb = 0;
        if (jb <= st.ql) {
            cb = st.carry[jb];
            qb = st.q[jb - 1];
        }
        const int blocks = min(8, (st.steps - sb) >> 3);
        for (int b = 0; b < blocks; ++b) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int x = b * 8 + u, s = sb + x;
                const int up_h = dpp_shr1(__builtin_amdgcn_readlane(cb.x, x), out_h);
                int up_e = dpp_shr1(__builtin_amdgcn_readlane(cb.y, x), out_e);
                qc = dpp_shr1(__builtin_amdgcn_readlane(qb, x), qc);
                up_e = s == st.s_top ? NEG : up_e;
                f = s == st.s_first ? st.f_init : f;
                if (COL0) prev_up = s == st.s_first0 ? st.p_init : prev_up;
                const int diag = wadd(prev_up, qc == st.tc ? match : mismatch);
                const int h = max(max(diag, up_e), f);
                const int eo = wsub(h, o), ee = wsub(up_e, e), fe = wsub(f, e);
                acc = shift_in_sign(acc, wsub(diag, h)); // H is not the diagonal (which wins ties)
                acc = shift_in_sign(acc, wsub(f, h));    // ... nor F (which wins ties against E)
                acc = shift_in_sign(acc, wsub(ee, eo));  // E opens here: only when strictly better than extending
                acc = shift_in_sign(acc, wsub(fe, eo));  // F opens here
                out_e = max(eo, ee);
                f = max(eo, fe);
                out_h = h;
                prev_up = up_h;
                if (LASTCOL) h_last = s == st.s_last ? h : h_last;
                // the row's maximum, left to right: a later column takes over only when strictly larger; in-band steps only
                const bool rtake = h > rmax && (unsigned)(s - st.s_first) <= (unsigned)st.s_span;
                rmax = rtake ? h : rmax;
                rs = rtake ? s : rs;
                if (s >= st.w_first && s <= st.w_last) {
                    if (lane == st.w_lane) wcarry[s] = make_int2(h, out_e);
                }
            }
            if (STORE) st.dir[(int64_t)((sb >> 3) + b) * 64] = acc;
        }
    }
}

// the decisions of one pair as the walk reads them
struct Dirs {
    const uint32_t *dir;
    int lo;
    int64_t strip_words;
    __device__ __forceinline__ unsigned at(const int i, const int j) const
    {
        const int r = i - 1, k = r >> 6, l = r & 63;
        const int c0 = max(1, 64 * k + 1 + lo), s = j - c0 + l;
        return (dir[(int64_t)k * strip_words + (int64_t)(s >> 3) * 64 + l] >> (4 * (7 - (s & 7)))) & 15u;
    }
};
constexpr unsigned D_NOT_DIAG = 8, D_NOT_F = 4, D_E_OPEN = 2, D_F_OPEN = 1;

__device__ __forceinline__ int trailing_ones(const unsigned long long m) { return m == ~0ull ? 64 : __builtin_ctzll(~m); }

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
            const int b = border(j, o, e);
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
            st.f_init = i + lo <= 0 ? border(i, o, e) - o : NEG; // (i, 0) is in the band: F[i][1] = H[i][0] - o
            st.p_init = border(i - 1, o, e);
            st.w_lane = last ? (rows - 1) & 63 : 63;
            st.w_first = __builtin_amdgcn_readlane(st.s_first, st.w_lane);
            st.w_last = min(__builtin_amdgcn_readlane(st.s_top, st.w_lane), ql - st.c0 + st.w_lane);
            st.carry = carry;
            st.q = tq;
            st.ql = ql;
            st.dir = dir + (int64_t)k * strip_words + lane;
            const bool col0 = st.c0 == 1, lastcol = 64 * k + 64 + hi >= ql, store = !a.score_only;
            // lane 0's first diagonal: H[64k][c0 - 1] (with column 0 in the band the sweep sets it from the border)
            const int prev_up = (lane == 0 && !col0) ? carry[st.c0 - 1].x : 0;
            int h_last = NEG;
            int rmax = i + lo <= 0 ? border(i, o, e) : NEG, rs = st.s_first - 1; // the border column where it is in the band
            if (store) {
                if (col0 && lastcol) sweep<true, true, true>(st, lane, a.match, a.mismatch, o, e, prev_up, h_last, rmax, rs);
                else if (col0) sweep<true, false, true>(st, lane, a.match, a.mismatch, o, e, prev_up, h_last, rmax, rs);
                else if (lastcol) sweep<false, true, true>(st, lane, a.match, a.mismatch, o, e, prev_up, h_last, rmax, rs);
                else sweep<false, false, true>(st, lane, a.match, a.mismatch, o, e, prev_up, h_last, rmax, rs);
            } else {
                if (col0 || lastcol) sweep<true, true, false>(st, lane, a.match, a.mismatch, o, e, prev_up, h_last, rmax, rs);
                else sweep<false, false, false>(st, lane, a.match, a.mismatch, o, e, prev_up, h_last, rmax, rs);
            }
            __threadfence_block(); // the carry row before the next strip reads it, the decisions before the walk does
            __builtin_amdgcn_wave_barrier();

            // ---- best(i) per row: an inclusive prefix of (H, i, j) over the lanes; lane 0's element is folded with the running best
            // of the strips above first (which is earlier: it stays on a tie)
            const int rcol = st.c0 + rs - lane;
            int ph = rowv ? rmax : NEG, pi = i, pj = rcol;
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
                              (int64_t)xh - (int64_t)rmax > (int64_t)a.zdrop + (int64_t)e * (int64_t)abs((i - xi) - (rcol - xj));
            const unsigned long long dm = __ballot(drop);
            const int live = dm ? __builtin_ctzll(dm) : min(64, rows - 64 * k); // the strip's rows that exist for the outputs
            if (live > 0) {
                bh = __shfl(ph, live - 1);
                bi = __shfl(pi, live - 1);
                bj = __shfl(pj, live - 1);
            }
            if (lane < live && st.s_last != NEVER && h_last >= mq) {
                mq = h_last;
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

        // ---- the walk of sw_banded.hip from (I, J) back to (0, 0), the whole wave on one path
        const Dirs dv{dir, lo, strip_words};
        int seg = 0, ne = 0, size = 0;
        auto push = [&](const unsigned op, const int len) { // (last element first; zero lengths are skipped)
            if (len <= 0) return;
            if (lane == 0) elems[ne] = (uint32_t)len << 4 | op;
            ++ne;
            size += a.binary_cigar ? 4 : digits(len) + 1;
        };
        constexpr unsigned OP_M = 0, OP_I = 1, OP_D = 2;
        unsigned state = OP_M;
        do {
            // the next 64 cells of the diagonal: how many of them are diagonal moves
            const int di = I - lane, dj = J - lane;
            const bool dvalid = di >= 1 && dj >= 1;
            const unsigned nib = dvalid ? dv.at(di, dj) : D_NOT_DIAG;
            const int run = trailing_ones(__ballot(dvalid && !(nib & D_NOT_DIAG)));
            unsigned next;
            int step;
            if (run > 0) {
                next = OP_M;
                step = run;
                I -= run;
                J -= run;
            } else if (!(__builtin_amdgcn_readfirstlane(nib) & D_NOT_F)) {
                // F: one column, and one more for every cell to the left whose F went on extending
                next = OP_I;
                step = 1;
                for (;;) {
                    const int jj = J - step - lane;
                    const bool v = jj >= 1 && jj >= I + lo;
                    const int r = trailing_ones(__ballot(v && !(dv.at(I, v ? jj : J) & D_F_OPEN)));
                    step += r;
                    if (r < 64) break;
                }
                J -= step;
            } else {
                next = OP_D;
                step = 1;
                for (;;) {
                    const int ii = I - step - lane;
                    const bool v = ii >= 1 && J <= ii + hi;
                    const int r = trailing_ones(__ballot(v && !(dv.at(v ? ii : I, J) & D_E_OPEN)));
                    step += r;
                    if (r < 64) break;
                }
                I -= step;
            }
            if (next == state) {
                seg += step;
            } else {
                push(state, seg);
                seg = step;
                state = next;
            }
        } while (I > 0 && J > 0);
        push(state, seg);
        if (I > 0) push(OP_D, I); // a walk that reaches column 0 or row 0 finishes with one run
        else if (J > 0) push(OP_I, J);
        const int cap = a.binary_cigar ? a.cigar_stride & ~3 : a.cigar_stride;
        if (size > cap) {
            finish(ST_CIGAR_OVERFLOW, 0);
            continue;
        }
        __threadfence_block(); // lane 0's elements before the wave reads them
        __builtin_amdgcn_wave_barrier();
        // ---- the elements front to back, 64 at a time: a prefix sum of their widths places each lane's
        char *const out = a.cigar + p * (int64_t)a.cigar_stride;
        for (int base = 0, at = 0; base < ne; base += 64) {
            const int m = base + lane;
            const uint32_t v = m < ne ? elems[ne - 1 - m] : 0;
            const int len = (int)(v >> 4);
            const int w = m < ne ? (a.binary_cigar ? 4 : digits(len) + 1) : 0;
            int incl = w;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int up = __shfl_up(incl, d);
                if (lane >= d) incl += up;
            }
            int pos = at + incl;
            if (m < ne) {
                if (a.binary_cigar) {
                    out[pos - 4] = (char)(v & 0xff);
                    out[pos - 3] = (char)((v >> 8) & 0xff);
                    out[pos - 2] = (char)((v >> 16) & 0xff);
                    out[pos - 1] = (char)(v >> 24);
                } else {
                    const unsigned op = v & 15u;
                    out[--pos] = op == OP_M ? 'M' : op == OP_I ? 'I' : 'D';
                    for (int x = len; x > 0; x /= 10) out[--pos] = (char)('0' + x % 10);
                }
            }
            at += __shfl(incl, 63);
        }
        finish(0, size);
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
