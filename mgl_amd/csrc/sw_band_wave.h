// sw_band_wave.h -- what sw_banded_kernel (sw_banded.hip), sw_extend_kernel (sw_extend.hip) and sw_extend_adaptive_kernel
// (sw_extend_adaptive.hip) share: one wave per pair over the cells of a diagonal band, int32 (DESIGN.md sections 9b to 9d).  Device code,
// included by those three files only; every function is inlined
// into its kernel (docs/history.md C.000000 compares the code objects with those of the kernels that held a copy each).
//
// The 64 lanes hold 64 consecutive target rows (a strip) on an anti-diagonal: at step s lane l of strip k is at column c0 + s - l,
// c0 = max(1, 64k + 1 + lo) the first column any row of the strip has in the band.  E of the cell above and H of the diagonal come
// from lane l - 1's previous step (wave_shr:1), the query byte travels the same way; lane 0 takes all three from registers that the
// wave loads 64 columns at a time: the carry row {H, E} that the strip above left in the pair's workspace slot, and the query.  The
// strip's last row (the pair's last row in the last strip) writes the carry row for the next.
//
// The lanes never branch on the band.  A lane computes at every step, in the band or not; what keeps the out-of-band values out is
// three per-lane step numbers: at its first in-band column a lane's F (and, where that column is 1, its diagonal) is set to what the
// definition says enters there -- the border's, or minus infinity --, at the column on the band's upper edge the E from above is
// minus infinity, and whatever a lane computes after its last in-band column is read by nobody (the lane below is then on its own
// upper edge, or past it).  Minus infinity is BANDED_NEG (sw_banded.h: the range guard makes it lose every comparison).
//
// Every cell leaves four bits -- H is not the diagonal / H is not F / E opened / F opened -- shifted into a dword per lane, stored
// every eighth step: [strip][step / 8][lane].  The wave walks the path together: 64 lanes look at the next 64 cells of a diagonal (or
// of a gap run) at once and a ballot gives the run's length.  Lane 0 keeps the elements, last first, in the slot; the wave writes
// them out front to back.
#ifndef MGL_SW_BAND_WAVE_H
#define MGL_SW_BAND_WAVE_H

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

// H of border cell k of row 0 or column 0: a gap's penalty where the borders carry one (`gaps`), otherwise zero
__device__ __forceinline__ int border(int k, int o, int e, bool gaps) { return (gaps && k > 0) ? -o - (k - 1) * e : 0; }

__device__ __forceinline__ int digits(int v)
{
    int d = 1;
    while (v >= 10) {
        v /= 10;
        ++d;
    }
    return d;
}

__device__ __forceinline__ int trailing_ones(const unsigned long long m) { return m == ~0ull ? 64 : __builtin_ctzll(~m); }

// what a strip's sweep needs beside the lane's registers
struct Strip {
    int c0, steps;                 // first column, steps (a multiple of 8)
    bool col0, lastcol;            // the strip has rows whose band starts at column 1 / that reach column ql
    int tc;                        // the lane's target byte
    int s_first, s_first0, s_top, s_last; // the lane's step at its first in-band column / the same where that column is 1 / on the band's upper edge / at column ql
    int s_span;                    // the lane's in-band steps are s_first .. s_first + s_span (ROWMAX sweeps only: their caller sets it)
    int f_init, p_init;            // F entering the first in-band column; H[i - 1][0]
    int w_first, w_last, w_lane;   // the writing lane and its steps in the band
    int2 *carry;
    const unsigned char *q;
    int ql;
    uint32_t *dir;                 // the strip's decisions + lane
};

// strip k of a pair whose rows 1 .. rows have cells in the band lo <= j - i <= hi; t, q: the pair's sequences; dir: the strip's decisions
// (sw_extend.hip writes the same out: see there)
__device__ __forceinline__ Strip strip_setup(const int k, const int lane, const int rows, const int ql, const int lo, const int hi, const int o, const int e,
                                             const bool gaps, const unsigned char *const t, const unsigned char *const q, int2 *const carry, uint32_t *const dir)
{
    const int i = 64 * k + lane + 1;
    const bool rowv = i <= rows, last = k + 1 == (rows + 63) / 64;
    Strip st;
    st.c0 = max(1, 64 * k + 1 + lo);
    const int c1 = min(ql, 64 * k + 64 + hi);
    st.steps = (c1 - st.c0 + 64 + 7) & ~7;
    st.tc = rowv ? t[(int64_t)i - 1] : 0x100;
    const int jlo = max(1, i + lo);
    st.s_first = jlo - st.c0 + lane;
    st.s_first0 = jlo == 1 ? st.s_first : NEVER;
    st.s_top = i + hi - st.c0 + lane;
    st.s_last = rowv && i + hi >= ql ? ql - st.c0 + lane : NEVER;
    st.f_init = i + lo <= 0 ? border(i, o, e, gaps) - o : NEG; // (i, 0) is in the band: F[i][1] = H[i][0] - o
    st.p_init = border(i - 1, o, e, gaps);
    st.w_lane = last ? (rows - 1) & 63 : 63;
    st.w_first = __builtin_amdgcn_readlane(st.s_first, st.w_lane);
    st.w_last = min(__builtin_amdgcn_readlane(st.s_top, st.w_lane), ql - st.c0 + st.w_lane);
    st.carry = carry;
    st.q = q;
    st.ql = ql;
    st.dir = dir + lane;
    st.col0 = st.c0 == 1;
    st.lastcol = 64 * k + 64 + hi >= ql;
    return st;
}

// what a sweep leaves in a lane beside the carry row and the decisions
struct Swept {
    int h_last;   // H at column ql (the lanes with s_last)
    int rmax, rs; // ROWMAX sweeps only: the row's largest in-band H and the step of its first appearance, seeded by the caller
};

// COL0, LASTCOL: Strip's col0, lastcol (the diagonal at column 1 is the border column's H; H at column ql is kept); STORE: decisions
// are kept; ROWMAX: the row's maximum is kept
template <bool COL0, bool LASTCOL, bool STORE, bool ROWMAX>
__device__ __forceinline__ void sweep(const Strip &st, const int lane, const int match, const int mismatch, const int o, const int e, int prev_up, Swept &sw)
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
                if (LASTCOL) sw.h_last = s == st.s_last ? h : sw.h_last;
                if (ROWMAX) {
                    // the row's maximum, left to right: a later column takes over only when strictly larger; in-band steps only
                    const bool rtake = h > sw.rmax && (unsigned)(s - st.s_first) <= (unsigned)st.s_span;
                    sw.rmax = rtake ? h : sw.rmax;
                    sw.rs = rtake ? s : sw.rs;
                }
                if (s >= st.w_first && s <= st.w_last) {
                    if (lane == st.w_lane) wcarry[s] = make_int2(h, out_e);
                }
            }
            if (STORE) st.dir[(int64_t)((sb >> 3) + b) * 64] = acc;
        }
    }
}

// the sweep of one strip, specialised by what the strip needs
template <bool ROWMAX>
__device__ __forceinline__ void sweep_strip(const Strip &st, const int lane, const int match, const int mismatch, const int o, const int e, const bool store, Swept &sw)
{
    // lane 0's first diagonal: H[64k][c0 - 1] (with column 0 in the band the sweep sets it from the border)
    const int prev_up = (lane == 0 && !st.col0) ? st.carry[st.c0 - 1].x : 0;
    sw.h_last = NEG;
    if (store) {
        if (st.col0 && st.lastcol) sweep<true, true, true, ROWMAX>(st, lane, match, mismatch, o, e, prev_up, sw);
        else if (st.col0) sweep<true, false, true, ROWMAX>(st, lane, match, mismatch, o, e, prev_up, sw);
        else if (st.lastcol) sweep<false, true, true, ROWMAX>(st, lane, match, mismatch, o, e, prev_up, sw);
        else sweep<false, false, true, ROWMAX>(st, lane, match, mismatch, o, e, prev_up, sw);
    } else {
        if (st.col0 || st.lastcol) sweep<true, true, false, ROWMAX>(st, lane, match, mismatch, o, e, prev_up, sw);
        else sweep<false, false, false, ROWMAX>(st, lane, match, mismatch, o, e, prev_up, sw);
    }
}

// the decisions of one pair as the walk reads them
struct Dirs {
    const uint32_t *dir;
    int lo, hi;
    int64_t strip_words;
    __device__ __forceinline__ unsigned at(const int i, const int j) const
    {
        const int r = i - 1, k = r >> 6, l = r & 63;
        const int c0 = max(1, 64 * k + 1 + lo), s = j - c0 + l;
        return (dir[(int64_t)k * strip_words + (int64_t)(s >> 3) * 64 + l] >> (4 * (7 - (s & 7)))) & 15u;
    }
};
constexpr unsigned D_NOT_DIAG = 8, D_NOT_F = 4, D_E_OPEN = 2, D_F_OPEN = 1;
constexpr unsigned OP_M = 0, OP_I = 1, OP_D = 2, OP_S = 4;

// the walk's elements in the pair's slot: lane 0 keeps them, last first; every lane counts them and the bytes they will take
struct Elems {
    uint32_t *elems;
    int lane, binary;
    int ne, size;
    __device__ __forceinline__ void push(const unsigned op, const int len) // (zero lengths are skipped)
    {
        if (len <= 0) return;
        if (lane == 0) elems[ne] = (uint32_t)len << 4 | op;
        ++ne;
        size += binary ? 4 : digits(len) + 1;
    }

    // the elements front to back into `out`, 64 at a time: a prefix sum of their widths places each lane's.  CLIPS: there may be 'S'
    template <bool CLIPS>
    __device__ __forceinline__ void write(char *const out) const
    {
        __threadfence_block(); // lane 0's elements before the wave reads them
        __builtin_amdgcn_wave_barrier();
        for (int base = 0, at = 0; base < ne; base += 64) {
            const int m = base + lane;
            const uint32_t v = m < ne ? elems[ne - 1 - m] : 0;
            const int len = (int)(v >> 4);
            const int w = m < ne ? (binary ? 4 : digits(len) + 1) : 0;
            int incl = w;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int up = __shfl_up(incl, d);
                if (lane >= d) incl += up;
            }
            int pos = at + incl;
            if (m < ne) {
                if (binary) {
                    out[pos - 4] = (char)(v & 0xff);
                    out[pos - 3] = (char)((v >> 8) & 0xff);
                    out[pos - 2] = (char)((v >> 16) & 0xff);
                    out[pos - 1] = (char)(v >> 24);
                } else {
                    const unsigned op = v & 15u;
                    out[--pos] = op == OP_M ? 'M' : op == OP_I ? 'I' : (!CLIPS || op == OP_D) ? 'D' : 'S';
                    for (int x = len; x > 0; x /= 10) out[--pos] = (char)('0' + x % 10);
                }
            }
            at += __shfl(incl, 63);
        }
    }
};

// The walk (calculateCigar, sw.cpp:149-255, as walk_and_write() in sw_traceback.h restates it), the whole wave on one path: from
// (I, J), inside a run of `seg` cells of `state`, back to row 0 or column 0.  Finished runs are pushed; where it ended and the last run, which
// the caller closes, are returned
struct Walked {
    int I, J, seg;
    unsigned state;
};
__device__ __forceinline__ Walked walk(const Dirs &dv, const int lane, int I, int J, int seg, Elems &el)
{
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
                const bool v = jj >= 1 && jj >= I + dv.lo;
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
                const bool v = ii >= 1 && J <= ii + dv.hi;
                const int r = trailing_ones(__ballot(v && !(dv.at(v ? ii : I, J) & D_E_OPEN)));
                step += r;
                if (r < 64) break;
            }
            I -= step;
        }
        if (next == state) {
            seg += step;
        } else {
            el.push(state, seg);
            seg = step;
            state = next;
        }
    } while (I > 0 && J > 0);
    return Walked{I, J, seg, state};
}

} // namespace

} // namespace mgl_sw_dev

#endif
