// sw_extend_adaptive.hip -- sw_extend_adaptive_kernel, the kernel of mgl_sw_extend_batch_device with MGL_SW_FLAG_EXTEND_ADAPTIVE_BAND:
// sw_extend.hip's extension with a band that is re-centred once per strip of 64 rows on the diagonal of the cell that holds the
// maximum of the strip's last row (the function is tests/extend_adaptive_textbook.py's, which the tests compare
// with).
//
// The mapping, the sweep, the decision bits, the prefix over rows, the Z-drop test and the CIGAR output are sw_extend.hip's and
// sw_band_wave.h's; sweep() is called as there.  What is new:
//
// Strip k has its own band lo_k = d_k - band <= j - i <= hi_k = d_k + band, d_0 = 0, and every entry of Strip is filled from lo_k,
// hi_k.  d_(k+1) is lane 63's column of the row maximum minus 64 (k + 1), read out of the lane after a sweep that did not drop.
// |d_(k+1) - d_k| <= band, because that column lies in row 64 (k + 1)'s band.
//
// The seam.  The sweep writes the carry row over the writing lane's in-band columns only, and lane 0 of the next strip reads the
// columns of ITS band (and the one to the left of it, its first diagonal).  After a shift these are up to `band` columns more on one
// side, which hold what an earlier strip or row 0 left there: the wave stores minus infinity over them before the next strip starts.
// Where row 64 (k + 1) did not have the border column in its band and row 64 (k + 1) + 1 has, lane 0's first diagonal is minus infinity
// too (p_init); where the band moved left, the cell above lane 0's upper edge is in the band of its own row and its E is read (s_top).
//
// A band that moved left holds cells that no path reaches: every input of such a cell is minus infinity or derived from it, so it holds
// BANDED_NEG plus at most match x (diagonal steps since), which is below -2^29 under the range guard (match x (min(tl, ql) - 1) < 2^29)
// and above INT_MIN (the fall is at most 2 gopen + |mismatch| min(tl, ql) + gext max(tl, ql) <= 2^29): it loses every comparison with a
// finite value strictly, as the sentinel itself does.  A row that has a cell has a finite one (the diagonal of the new centre, or column
// ql below it; the textbook asserts it), so no such value becomes a row maximum, and (i, ql) is finite where it is in the band.
//
// The walk reads a strip's decisions with that strip's c0, so lane 0 keeps d_k per strip behind the decisions; AdaptiveDirs::at()
// reads it back and answers "not a diagonal, a gap opened" for a cell outside its row's band, which ends every run there (the
// diagonal look-ahead of 64 cells may cross a seam into cells the strip above did not hold).  walk_adaptive() is walk() of
// sw_band_wave.h with that view; as a template over the view walk() changed the code objects of the two kernels that share it
// (docs/history.md), so the 45 lines stand twice.
//
// Geometry in int32: banded_range_ok() is unchanged, |d_k| <= max(tl, ql) <= 2^28 (0 <= rj <= ql, 64 k <= tl), the host clamps band at
// 2^29, so every 64 k + 64 + d_k + band is at most 2^30 + 64 and every d_k - band at least -(2^28 + 2^29).
#include "sw_band_wave.h"
#include "sw_extend.h"

namespace mgl_sw_dev {

namespace {

// the decisions of one pair as the walk reads them: a strip's first column comes from its own centre
struct AdaptiveDirs {
    const uint32_t *dir;
    const int *centre;
    int band;
    int64_t strip_words;
    __device__ __forceinline__ unsigned at(const int i, const int j) const // i >= 1
    {
        const int r = i - 1, k = r >> 6, l = r & 63;
        const int d = centre[k], off = j - i - d;
        if (off < -band || off > band) return D_NOT_DIAG | D_NOT_F | D_E_OPEN | D_F_OPEN;
        const int c0 = max(1, 64 * k + 1 + d - band), s = j - c0 + l;
        return (dir[(int64_t)k * strip_words + (int64_t)(s >> 3) * 64 + l] >> (4 * (7 - (s & 7)))) & 15u;
    }
};

// walk() of sw_band_wave.h over AdaptiveDirs: a run ends where at() says so, which covers the band of every row it looks at
__device__ __forceinline__ Walked walk_adaptive(const AdaptiveDirs &dv, const int lane, int I, int J, int seg, Elems &el)
{
    unsigned state = OP_M;
    do {
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
            next = OP_I;
            step = 1;
            for (;;) {
                const int jj = J - step - lane;
                const bool v = jj >= 1;
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
                const bool v = ii >= 1;
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

__global__ __launch_bounds__(64) void sw_extend_adaptive_kernel(const ExtendArgs a)
{
    const int lane = threadIdx.x;
    const int o = a.gopen, e = a.gext, band = a.band;
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
        if (!banded_range_ok(tl, ql, a.match, a.mismatch, o, e) || extend_adaptive_pair_bytes(tl, ql, band, a.score_only != 0) > a.slot_bytes) {
            finish(ST_UNSUPPORTED, 0);
            continue;
        }
        int2 *const carry = reinterpret_cast<int2 *>(slot);
        uint32_t *const elems = reinterpret_cast<uint32_t *>(slot + banded_carry_bytes(ql));
        uint32_t *const dir = reinterpret_cast<uint32_t *>(slot + banded_carry_bytes(ql) + banded_elem_bytes(tl, ql));
        const int64_t strip_words = (int64_t)extend_strip_steps(ql, band) * 8;
        int *const centre = reinterpret_cast<int *>(dir + (int64_t)((tl + 63) / 64) * strip_words); // (not score-only: the slot ends before it otherwise)
        const int64_t ts = a.t.off[p];
        const unsigned char *const tq = a.q.data + a.q.off[p];

        // row 0: the border's H and the E that enters row 1, minus infinity beyond the band (d_0 = 0)
        for (int j = lane; j <= ql; j += 64) {
            const int b = border(j, o, e, true); // the anchored start: always a gap penalty
            carry[j] = j <= band ? make_int2(b, b - o) : make_int2(NEG, NEG);
        }
        __threadfence_block();
        __builtin_amdgcn_wave_barrier();

        int d = 0, lo_above = -band, hi_above = band; // the strip's centre; lo and hi of the strip above (of row 64 k)
        int rows = 0;                      // rows 1 .. rows have a cell in their band, as far as the strips went
        int bh = 0, bi = 0, bj = 0;        // best(i) of the rows done so far: (0, 0) is the empty extension
        int mq = EXTEND_NO_QEND, mqt = -1; // the lane's last-column best: later rows win ties
        int rows_done = tl, dropped = 0;
        for (int k = 0; 64 * k < tl; ++k) {
            const int lo = d - band, hi = d + band;
            if (64 * k + 1 + lo > ql) break;         // row 64 k + 1 has no cell in this band, nor has any row below it
            const int srows = min(tl, ql - lo);      // the rows that have a cell in this strip's band end here
            // ... inside this strip, or the target does: there is no next one.  (Where they end with the strip's last row, the next centre may bring
            // row 64 k + 65 back into the matrix: the loop's test decides)
            const bool last = srows < 64 * k + 64 || 64 * k + 64 >= tl;
            rows = min(srows, 64 * k + 64);
            if (lane == 0 && !a.score_only) centre[k] = d;
            // the strip as sw_extend.hip fills it, from this strip's lo and hi
            const int i = 64 * k + lane + 1;
            const bool rowv = i <= srows;
            Strip st;
            st.c0 = max(1, 64 * k + 1 + lo);
            const int c1 = min(ql, 64 * k + 64 + hi);
            st.steps = (c1 - st.c0 + 64 + 7) & ~7;
            st.tc = rowv ? a.t.data[ts + i - 1] : 0x100;
            const int jlo = max(1, i + lo);
            st.s_first = jlo - st.c0 + lane;
            st.s_first0 = jlo == 1 ? st.s_first : NEVER;
            st.s_top = i + hi - st.c0 + lane;
            st.s_span = min(i + hi, ql) - jlo; // (a row past `srows` may get any window, a negative span read as unsigned included: rowv keeps it out of every result)
            st.s_last = rowv && i + hi >= ql ? ql - st.c0 + lane : NEVER;
            st.f_init = i + lo <= 0 ? border(i, o, e, true) - o : NEG; // (i, 0) is in the band: F[i][1] = H[i][0] - o
            // H[i - 1][0]: for lane 0 it belongs to the strip above, whose band may have left the border column already
            st.p_init = (lane == 0 && 64 * k + lo_above > 0) ? NEG : border(i - 1, o, e, true);
            st.w_lane = last ? (srows - 1) & 63 : 63;
            st.w_first = __builtin_amdgcn_readlane(st.s_first, st.w_lane);
            st.w_last = min(__builtin_amdgcn_readlane(st.s_top, st.w_lane), ql - st.c0 + st.w_lane);
            // the cell above lane 0's upper edge belongs to the strip above: where the band moved left it is in that strip's band and its E counts
            if (lane == 0 && hi < hi_above) st.s_top = NEVER;
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
            __threadfence_block(); // the carry row before the next strip reads it, the decisions and the centre before the walk does
            __builtin_amdgcn_wave_barrier();

            // ---- best(i) per row, the drop test, the last column: sw_extend.hip's
            const int rcol = st.c0 + sw.rs - lane;
            int ph = rowv ? sw.rmax : NEG, pi = i, pj = rcol;
            if (lane == 0 && !(ph > bh)) {
                ph = bh;
                pi = bi;
                pj = bj;
            }
#pragma unroll
            for (int dd = 1; dd < 64; dd <<= 1) {
                const int oh = __shfl_up(ph, dd), oi = __shfl_up(pi, dd), oj = __shfl_up(pj, dd);
                const bool keep = lane < dd || ph > oh; // strict: the earlier rows win a tie
                ph = keep ? ph : oh;
                pi = keep ? pi : oi;
                pj = keep ? pj : oj;
            }
            int xh = __shfl_up(ph, 1), xi = __shfl_up(pi, 1), xj = __shfl_up(pj, 1);
            if (lane == 0) {
                xh = bh;
                xi = bi;
                xj = bj;
            }
            const bool drop = rowv && a.zdrop >= 0 &&
                              (int64_t)xh - (int64_t)sw.rmax > (int64_t)a.zdrop + (int64_t)e * (int64_t)abs((i - xi) - (rcol - xj));
            const unsigned long long dm = __ballot(drop);
            const int live = dm ? __builtin_ctzll(dm) : min(64, srows - 64 * k); // the strip's rows that exist for the outputs
            if (live > 0) {
                bh = __shfl(ph, live - 1);
                bi = __shfl(pi, live - 1);
                bj = __shfl(pj, live - 1);
            }
            // (i, ql) in the band is finite: it is the row's rightmost cell, and F carries a finite value to it from the finite cell every row
            // with a cell has (file header) -- so no unreachable NEG + x, which would beat EXTEND_NO_QEND == NEG here, gets in
            if (lane < live && st.s_last != NEVER && sw.h_last >= mq) {
                mq = sw.h_last;
                mqt = i;
            }
            if (dm) {
                rows_done = 64 * k + live;
                dropped = 1;
                break;
            }
            if (last) break;

            // ---- the next strip's centre: the diagonal of the maximum of row 64 (k + 1), which lane 63 holds; the columns of that row
            // that the next strip's lane 0 reads (its band, and the column left of it) and lane 63 did not write become minus infinity
            const int rn = 64 * (k + 1);
            const int dn = __builtin_amdgcn_readlane(rcol, 63) - rn;
            const int wa = max(1, rn + lo), wb = min(ql, rn + hi);                   // written: row rn's band
            const int ra = max(1, rn + dn - band), rb = min(ql, rn + dn + band);     // read
            for (int j = ra + lane; j <= min(rb, wa - 1); j += 64) carry[j] = make_int2(NEG, NEG);
            for (int j = max(ra, wb + 1) + lane; j <= rb; j += 64) carry[j] = make_int2(NEG, NEG);
            __threadfence_block();
            __builtin_amdgcn_wave_barrier();
            lo_above = lo;
            hi_above = hi;
            d = dn;
        }
        if (!dropped && rows < tl && a.zdrop >= 0) { // row rows + 1 has no cell in its band: it drops whenever the rule is on
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
        const AdaptiveDirs dv{dir, centre, band, strip_words};
        Elems el{elems, lane, a.binary_cigar, 0, 0};
        const Walked w = walk_adaptive(dv, lane, I, J, 0, el);
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
hipError_t launch_extend_adaptive(const ExtendArgs &a, hipStream_t stream)
{
    if (a.n < 1) return hipSuccess;
    if (!a.ext || !a.ws || a.slots < 1 || a.slot_bytes < 256 || (!a.score_only && (!a.cigar || !a.cigar_len))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_extend_adaptive_kernel, dim3((unsigned)a.slots), dim3(64), 0, stream, a);
    return hipGetLastError();
}

} // namespace mgl_sw_dev
