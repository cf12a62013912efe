// sw_banded.hip -- sw_banded_kernel, the kernel of mgl_sw_align_batch_device_banded: the GATK function (DESIGN.md section 2's
// recurrence, priorities, tie rules, end-cell scans and walk) over the cells of a diagonal band only (the
// function is tests/banded_textbook.py's, which the tests compare with).
//
// One wave per pair, int32.  The 64 lanes hold 64 consecutive target rows (a strip) on an anti-diagonal: at step s lane l of strip k
// is at column c0 + s - l, c0 = max(1, 64k + 1 + lo) the first column any row of the strip has in the band.  E of the cell above and H
// of the diagonal come from lane l - 1's previous step (wave_shr:1), the query byte travels the same way; lane 0 takes all three from
// registers that the wave loads 64 columns at a time: the carry row {H, E} that the strip above left in the pair's workspace slot,
// and the query.  The strip's last row (the pair's last row in the last strip) writes the carry row for the next.
//
// The lanes never branch on the band.  A lane computes at every step, in the band or not; what keeps the out-of-band values out is
// three per-lane step numbers: at its first in-band column a lane's F (and, where that column is 1, its diagonal) is set to what the
// definition says enters there -- the border's, or minus infinity --, at the column on the band's upper edge the E from above is
// minus infinity, and whatever a lane computes after its last in-band column is read by nobody (the lane below is then on its own
// upper edge, or past it).  Minus infinity is BANDED_NEG (sw_banded.h: the range guard makes it lose every comparison).
//
// Every cell leaves four bits -- H is not the diagonal / H is not F / E opened / F opened -- shifted into a dword per lane, stored
// every eighth step: [strip][step / 8][lane].  The wave then scans the last column's and last row's in-band cells, and walks the path
// together: 64 lanes look at the next 64 cells of a diagonal (or of a gap run) at once and a ballot gives the run's length.  Lane 0
// keeps the elements, last first, in the slot; the wave writes them out front to back.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sw_banded.h"

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

__device__ __forceinline__ int border(int k, int o, int e, bool indel) { return (indel && k > 0) ? -o - (k - 1) * e : 0; }

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
    int f_init, p_init;            // F entering the first in-band column; H[i - 1][0]
    int w_first, w_last, w_lane;   // the writing lane and its steps in the band
    int2 *carry;
    const unsigned char *q;
    int ql;
    uint32_t *dir;                 // the strip's decisions + lane
};

// COL0: the strip has rows whose band starts at column 1 (their diagonal there is the border column's H); LASTCOL: rows that reach
// column ql (H there is kept for the last-column scan); STORE: decisions are kept
template <bool COL0, bool LASTCOL, bool STORE>
__device__ __forceinline__ void sweep(const Strip &st, const int lane, const int match, const int mismatch, const int o, const int e, int prev_up, int &h_last)
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

__global__ __launch_bounds__(64) void sw_banded_kernel(const BandedArgs a)
{
    const int lane = threadIdx.x;
    const int o = a.gopen, e = a.gext;
    const bool indel = (a.strategy & (OS_INDEL | OS_LEAD_ID)) != 0;
    unsigned char *const slot = a.ws + (int64_t)blockIdx.x * a.slot_bytes;

    for (int64_t p = blockIdx.x; p < a.n; p += a.slots) {
        const int tl = a.t.len[p], ql = a.q.len[p];
        Score sc{0, 0, 0, 0, 0, 0};
        auto finish = [&](const int status, const int offset, const int cigar_len) {
            if (lane != 0) return;
            a.offset[p] = offset;
            if (a.score) a.score[p] = sc;
            if (a.status) a.status[p] = status;
            if (a.cigar_len) a.cigar_len[p] = cigar_len;
        };
        if (tl < 1 || ql < 1 || tl > a.max_tl || ql > a.max_ql) {
            finish(ST_BAD_ARG, 0, 0);
            continue;
        }
        if (!banded_range_ok(tl, ql, a.match, a.mismatch, o, e) || banded_pair_bytes(tl, ql, a.band, a.score_only != 0) > a.slot_bytes) {
            finish(ST_UNSUPPORTED, 0, 0);
            continue;
        }
        const int lo = banded_lo(tl, ql, a.band), hi = banded_hi(tl, ql, a.band);
        int2 *const carry = reinterpret_cast<int2 *>(slot);
        uint32_t *const elems = reinterpret_cast<uint32_t *>(slot + banded_carry_bytes(ql));
        uint32_t *const dir = reinterpret_cast<uint32_t *>(slot + banded_carry_bytes(ql) + banded_elem_bytes(tl, ql));
        const int64_t strip_words = (int64_t)banded_strip_steps(tl, ql, a.band) * 8;
        const int64_t ts = a.t.off[p];
        const unsigned char *const tq = a.q.data + a.q.off[p];

        // row 0: the border's H and the E that enters row 1, minus infinity beyond the band
        for (int j = lane; j <= ql; j += 64) {
            const int b = border(j, o, e, indel);
            carry[j] = j <= hi ? make_int2(b, b - o) : make_int2(NEG, NEG);
        }
        __threadfence_block();
        __builtin_amdgcn_wave_barrier();

        int mq = NEG, mqt = -1; // the lane's last-column best: later rows win ties
        const int strips = (tl + 63) / 64;
        for (int k = 0; k < strips; ++k) {
            const int i = 64 * k + lane + 1;
            const bool rowv = i <= tl, last = k + 1 == strips;
            Strip st;
            st.c0 = max(1, 64 * k + 1 + lo);
            const int c1 = min(ql, 64 * k + 64 + hi);
            st.steps = (c1 - st.c0 + 64 + 7) & ~7;
            st.tc = rowv ? a.t.data[ts + i - 1] : 0x100;
            const int jlo = max(1, i + lo);
            st.s_first = jlo - st.c0 + lane;
            st.s_first0 = jlo == 1 ? st.s_first : NEVER;
            st.s_top = i + hi - st.c0 + lane;
            st.s_last = rowv && i + hi >= ql ? ql - st.c0 + lane : NEVER;
            st.f_init = i + lo <= 0 ? border(i, o, e, indel) - o : NEG; // (i, 0) is in the band: F[i][1] = H[i][0] - o
            st.p_init = border(i - 1, o, e, indel);
            st.w_lane = last ? (tl - 1) & 63 : 63;
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
            if (store) {
                if (col0 && lastcol) sweep<true, true, true>(st, lane, a.match, a.mismatch, o, e, prev_up, h_last);
                else if (col0) sweep<true, false, true>(st, lane, a.match, a.mismatch, o, e, prev_up, h_last);
                else if (lastcol) sweep<false, true, true>(st, lane, a.match, a.mismatch, o, e, prev_up, h_last);
                else sweep<false, false, true>(st, lane, a.match, a.mismatch, o, e, prev_up, h_last);
            } else {
                if (col0 || lastcol) sweep<true, true, false>(st, lane, a.match, a.mismatch, o, e, prev_up, h_last);
                else sweep<false, false, false>(st, lane, a.match, a.mismatch, o, e, prev_up, h_last);
            }
            if (st.s_last != NEVER && h_last >= mq) {
                mq = h_last;
                mqt = i;
            }
            __threadfence_block(); // the carry row before the next strip (or the last-row scan) reads it
            __builtin_amdgcn_wave_barrier();
        }
        // ---- the last column: the largest H, the later row among equals
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const int oq = __shfl_xor(mq, m), ot = __shfl_xor(mqt, m);
            const bool take = oq > mq || (oq == mq && ot > mqt);
            mq = take ? oq : mq;
            mqt = take ? ot : mqt;
        }
        // ---- the last row's in-band cells in column order: a larger H takes over, an equal one only when strictly nearer the
        // diagonal -- so the winner is the first of the nearest among the largest
        int rb = NEG, rj = 0x7fffffff;
        for (int j = max(1, tl + lo) + lane; j <= ql; j += 64) {
            const int h = carry[j].x;
            const int d = abs(tl - j), bd = abs(tl - rj);
            if (h > rb || (h == rb && d < bd)) { // (a lane's columns ascend: among equals at equal distance the first stays)
                rb = h;
                rj = j;
            }
        }
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const int ob = __shfl_xor(rb, m), oj = __shfl_xor(rj, m);
            const int d = abs(tl - rj), od = abs(tl - oj);
            const bool take = ob > rb || (ob == rb && (od < d || (od == d && oj < rj)));
            rb = take ? ob : rb;
            rj = take ? oj : rj;
        }
        sc.mqe = mq;
        sc.mqe_t = mqt;
        sc.max = mq;
        sc.max_t = mqt;
        sc.max_q = ql;
        sc.seg_length = 0;
        if (rb > mq || (rb == mq && abs(tl - rj) < abs(mqt - ql))) {
            sc.max = rb;
            sc.max_t = tl;
            sc.max_q = rj;
            sc.seg_length = ql - rj;
        }
        if (a.score_only) {
            finish(0, 0, 0);
            continue;
        }

        // ---- the walk (calculateCigar, sw.cpp:149-255, as walk_and_write() in sw_traceback.h restates it), the whole wave on one path
        const Dirs dv{dir, lo, strip_words};
        int I, J, seg = 0;
        if (a.strategy == OS_INDEL) {
            I = tl;
            J = ql;
        } else if (a.strategy != OS_LEAD_ID) {
            I = sc.max_t;
            J = sc.max_q;
            seg = sc.seg_length;
        } else {
            I = sc.mqe_t;
            J = ql;
        }
        int ne = 0, size = 0;
        auto push = [&](const unsigned op, const int len) { // (last element first; zero lengths are skipped)
            if (len <= 0) return;
            if (lane == 0) elems[ne] = (uint32_t)len << 4 | op;
            ++ne;
            size += a.binary_cigar ? 4 : digits(len) + 1;
        };
        constexpr unsigned OP_M = 0, OP_I = 1, OP_D = 2, OP_S = 4;
        if (seg > 0 && a.strategy == OS_SOFTCLIP) {
            push(OP_S, seg);
            seg = 0;
        }
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
        int off;
        if (a.strategy == OS_SOFTCLIP) {
            push(state, seg);
            if (J > 0) push(OP_S, J);
            off = I;
        } else if (a.strategy == OS_IGNORE) {
            push(state, seg + J);
            off = I - J;
        } else {
            push(state, seg);
            if (I > 0) push(OP_D, I);
            else if (J > 0) push(OP_I, J);
            off = 0;
        }
        const int cap = a.binary_cigar ? a.cigar_stride & ~3 : a.cigar_stride;
        if (size > cap) {
            finish(ST_CIGAR_OVERFLOW, 0, size);
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
                    out[--pos] = op == OP_M ? 'M' : op == OP_I ? 'I' : op == OP_D ? 'D' : 'S';
                    for (int x = len; x > 0; x /= 10) out[--pos] = (char)('0' + x % 10);
                }
            }
            at += __shfl(incl, 63);
        }
        finish(0, off, size);
        __threadfence_block(); // (the next pair reuses the slot)
        __builtin_amdgcn_wave_barrier();
    }
}

} // namespace

// pairs 0 .. n - 1 on a.slots waves, wave w in workspace slot w
hipError_t launch_banded(const BandedArgs &a, hipStream_t stream)
{
    if (a.n < 1) return hipSuccess;
    if (!a.offset || !a.ws || a.slots < 1 || a.slot_bytes < 256 || (!a.score_only && (!a.cigar || !a.cigar_len)) || (a.score_only && !a.score)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_banded_kernel, dim3((unsigned)a.slots), dim3(64), 0, stream, a);
    return hipGetLastError();
}

} // namespace mgl_sw_dev
