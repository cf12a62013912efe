// sw_dp16_lane_ck.hip -- the two-pairs-per-lane kernel (sw_dp16_lane.hip) in its CHECKPOINTED form: the fill keeps no traceback
// flags at all.  Of the 17 VALU instructions the full fill spends per two cells, 8 build the four flags of sw_lane_cell.h -- for
// 38 400 cells of a 256 x 150 pair of which the path visits ~300, nearly all of them in a way that needs no flag to be known.
//
//   pass 1  runs the score-only column code (8 instructions per two cells with base codes, sw_lane_cell.h) over the whole matrix
//           and keeps what is needed to START AGAIN anywhere on a coarse grid: {H, E} of every 16th target row per column -- the
//           carry row entering every 32-row strip (the reference's score[] / step[], sw_avx.cpp:36-47,196-197; kept for all strips
//           instead of being updated in place) and the row in a strip's middle -- and, every LANE_CK_COLS query columns, the lane's
//           register state (H of the previous column and the horizontal-gap value of its 32 rows).  All of it time-major,
//           [..][lane], stored straight from the registers in whole 256- / 512-byte rows: a lane only ever reads back its own.
//   pass 2  walks the path (sw.cpp:149-255).  The walk knows H of the cell it stands at, so a diagonal stretch up to the next
//           kept row is CHECKED instead of recomputed: if H drops by exactly the sum of the stretch's substitution scores, every
//           cell of it took the diagonal (PathWalk::verify_apply: the proof).  Only where that fails -- a gap, or a tie taken
//           elsewhere -- the walk first checks the shorter stretch to the LEFT EDGE of its block where that comes before the
//           kept row (the column checkpoints are kept columns: PathWalk::edge_len), so that a gap beyond the edge does not cost a
//           block on this side of it.  Then -- 2.78 rounds per wave on Illumina-style reads, 3.50 before the edge check
//           (docs/history.md C.000a) -- the lane recomputes the 16 x LANE_CK_COLS block the walk stands in: the SAME column
//           code with the flags switched on, started from the block's kept row and checkpoint, so every flag is bit for bit the
//           one the full fill would have stored, into a small private buffer; it walks as far as the block reaches and goes on.
//           Both pairs of a lane do this in lock step (one packed recomputation serves pair A's block and pair B's, different
//           blocks in general).
//
// Same arithmetic, same range guard (dp16_range_ok), same results as sw_dp16_lane_kernel.
//
// Per-wave region (a.tb + wave * a.tb_stride_words, lane_ck_words()): WaveMem below.  The wave's scratch (a.scratch,
// lane_ck_scratch_bytes()) holds both sequences of every lane, staged once as [4-base block][A | B][lane] dwords.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "sw_device.h"
#include "sw_lane_cell.h"
#include "sw_traceback.h"

// Timing-only experiment builds (scripts/build_variant.sh; results are WRONG with bits 1, 2, 4 or 16): parts of the kernel switched off
#ifndef MGL_CK_ABLATE
#define MGL_CK_ABLATE 0
#endif
#if (MGL_CK_ABLATE != 0 || defined(MGL_CK_PHASES) || defined(MGL_CK_TRACE)) && !defined(MGL_VARIANT_BUILD)
#error "MGL_CK_ABLATE / MGL_CK_PHASES are measurement builds (scripts/build_variant.sh defines MGL_VARIANT_BUILD): never the shipped library"
#endif

// -DMGL_CK_PHASES (scripts/build_variant.sh): every wave adds the shader-clock ticks it spent in each part of the kernel to a
// device array; mgl_ck_phases_dump() (exported by that build only) prints and clears it
#ifdef MGL_CK_PHASES
__device__ unsigned long long mgl_ck_phase_ticks[16];
#define CK_PHASE(k)                                                                                    \
    do {                                                                                               \
        const unsigned long long now_ = __builtin_amdgcn_s_memtime();                                  \
        if (lane == 0) atomicAdd(&mgl_ck_phase_ticks[k], now_ - phase_t0);                             \
        phase_t0 = __builtin_amdgcn_s_memtime();                                                       \
    } while (0)
#else
#define CK_PHASE(k) do { } while (0)
#endif

// -DMGL_CK_TRACE (scripts/build_variant.sh): every tile leaves {slot, hardware id, start, end (100 MHz ticks)}; mgl_ck_trace_dump(path)
// (exported by that build only) writes the array out -- scripts/ck_trace.py draws the launch's timeline from it
#ifdef MGL_CK_TRACE
__device__ unsigned long long mgl_ck_trace[4 << 17];
#endif

namespace mgl_sw_dev {

namespace {

constexpr int R = 32;            // target rows per strip
constexpr int RB = 16;           // rows per recomputed block
constexpr int CK = LANE_CK_COLS; // query columns per block

// the halves of two packed registers: {a.low, b.high}
__device__ __forceinline__ unsigned lo_hi(unsigned a, unsigned b) { return __builtin_amdgcn_perm(b, a, 0x07060100u); }

// what pass 2 needs to know about the wave's geometry and scoring
struct BlockGeom {
    int tl, ql, nb, match, mismatch, gopen, gext, base;
    bool indel;
    bool codes;  // the walks' windows hold base codes (the staged sequences do, and the walks read those)
    bool direct; // the walks' windows come from the caller's arrays (SeqBlocks): raw bytes
};

// ---- a pair's sequence where the CALLER keeps it (ASCII input), as pass 2's walks read it: whole aligned 16-byte blocks, the same
// bytes the reference compares (sw.cpp:55) whatever the wave staged.  A walk's window is 64 (16) consecutive bases that end at the
// cell it stands at: at most five (two) blocks, one load instruction each -- the staged copy is [4-base block][A | B][lane], every
// dword of a window a load of its own that uses 4 bytes of each 64-byte sector it touches (17 + 17 per pair against 5 + 5).
// Block 0 is the block that holds the sequence's first byte, block `last` the one that holds its last: an index outside 0 .. last
// is clamped (SeqWords::word does the same for dwords), so every block that is loaded holds at least one byte of the pair's own
// sequence and no load leaves the pages the caller's bytes lie in, wherever in a block the sequence starts and ends.  What a clamped
// block puts into the window are bytes in front of the sequence (never counted: a stretch is at most min(I, J) cells long) or behind
// the window's last base (shifted out).
struct SeqBlocks {
    const uint4 *base; // block 0
    int lo;            // where in block 0 the sequence's first byte stands
    __device__ __forceinline__ void init(const uint8_t *p)
    {
        lo = (int)(reinterpret_cast<uintptr_t>(p) & 15);
        base = reinterpret_cast<const uint4 *>(p - lo); // (pointer arithmetic, not a rounded integer: the loads stay global loads)
    }
    // bases end - W .. end - 1 (0-based; 1 <= end <= len) as W / 4 + 1 dwords that start at the window's first base rounded down to
    // a dword: the window's dword k is alignbyte(w[k + 1], w[k], return value), the form the staged windows have.  The funnel shift
    // by the low four bits of the window's address is two rounds of selects for its dword part (by 2, by 1); the byte part is the
    // alignbyte the compare does anyway.
    template <int W>
    __device__ __forceinline__ unsigned window(const int end, const int len, unsigned (&w)[W / 4 + 1]) const
    {
        const int w0 = lo + end - W; // the window's first byte counted from block 0's first (negative: in front of the sequence)
        const int b0 = w0 >> 4, last = max(lo + len - 1, 0) >> 4;
        const unsigned s = (unsigned)w0 & 15u;
        unsigned d[W / 4 + 4];
#pragma unroll
        for (int g = 0; g <= W / 16; ++g) {
            // (the byte offset in 32 bits, as WaveMem::at32)
            const uint4 v = *reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(base) + 16u * (unsigned)min(max(b0 + g, 0), last));
            d[4 * g] = v.x;
            d[4 * g + 1] = v.y;
            d[4 * g + 2] = v.z;
            d[4 * g + 3] = v.w;
        }
        // (bit selects, v_bfi_b32, not ?: -- two loads of d[] behind a condition become ONE load at a selected address while d[] is
        // still an array in memory, and then it stays one: the window went through scratch, 80 accesses per verify iteration)
        const unsigned by2 = 0u - ((s >> 3) & 1u), by1 = 0u - ((s >> 2) & 1u);
        unsigned e[W / 4 + 2];
#pragma unroll
        for (int k = 0; k < W / 4 + 2; ++k) e[k] = (d[k + 2] & by2) | (d[k] & ~by2);
#pragma unroll
        for (int k = 0; k < W / 4 + 1; ++k) w[k] = (e[k + 1] & by1) | (e[k] & ~by1);
        return s & 3u;
    }
};

// the wave's arrays (every pointer includes the lane): what pass 1 keeps, time-major -- a lane only ever reads what it wrote itself
struct WaveMem {
    uint2 *bnd;    // [row 32 k, k = 0 .. strips][column 0 .. ql][lane] {H, E} packed A | B: the carry row entering strip k (row 0: the border)
    uint2 *mid;    // [strip][column 1 .. ql][lane]: the row in the strip's middle (row 32 k + 16)   (bnd, mid, ck: the WIDE form; NARROW: below)
    unsigned *ck;  // [strip][block 1 .. nb - 1][2 r | 2 r + 1][lane]: H[.][32 b] and the horizontal-gap value of the strip's row r entering column 32 b + 1
    uint4 *blk;    // [column of the block][lane]: the recomputed flags of 16 rows
    // the same arrays as pass 2 addresses them: wave-uniform bases (SGPRs) and 32-bit indices that include the lane -- one address
    // register per load instead of two, no 64-bit arithmetic in the walk
    const uint2 *rows;     // the region: bnd at 0, mid at mid_off (entries)
    const unsigned *cku;   // ck without the lane
    const uint32_t *blku;  // blk without the lane, as dwords
    const unsigned *seq;   // the wave's staged sequences: the queries' blocks at 0, the targets' at t_off (dwords)
    unsigned mid_off, t_off, lane;
    // (the BYTE offset is what is computed in 32 bits: an element index leaves its scaling to 64-bit arithmetic and the load to a
    // 64-bit address in two registers -- pass 2 holds dozens of these at once)
    template <class T>
    __device__ __forceinline__ static T at32(const void *base, unsigned byte_off) { return *reinterpret_cast<const T *>(static_cast<const char *>(base) + byte_off); }
    __device__ __forceinline__ uint2 row16(int m, int ql, int j) const // {H, E} of row 16 m (m >= 0) at column j
    {
        return at32<uint2>(rows, 8u * ((m & 1) ? mid_off + (unsigned)(((m >> 1) * ql + j - 1) * 64) + lane : (unsigned)(((m >> 1) * (ql + 1) + j) * 64) + lane));
    }
    // ---- the NARROW records (NARROW = true below; launch_dp16_lane_ck says when).  In column<> eo = max(hn - (o-e), e) with hn >= e and
    // fo = max(hn - (o-e), fr) with hn >= fr, so H - E of a kept row and H - (gap value) of a checkpoint lie in [0, o-e] in every cell
    // that does not wrap: where o - e <= 255 the second value of a record is H minus ONE BYTE, and a lane keeps the H of four columns
    // (rows) as one 16-byte vector.  Same region, same bases of bnd / mid / ck / blk; the records use less of the parts they replace:
    //   rows  EVERY kept row -- the carry row entering strip k (row 32 k; row 0: the border) and the row in a strip's middle (row
    //         32 k + 16) -- has one format and keeps its place: carry row k starts at entry k (ql + 1) 64 of `bnd` (512 (ql + 1) bytes),
    //         the middle row of strip k at entry k ql 64 of `mid` (512 ql bytes): kept_row_off.  Column 0 is not stored (a formula).  The
    //         columns go in groups of four, group g = columns 4 g + 1 .. 4 g + 4, 1 536 bytes each: [lane] uint4 H of the four columns |
    //         [lane] uint2 the differences H - E, byte 2 u of the uint2 pair A's of column 4 g + 1 + u, byte 2 u + 1 pair B's.  A last
    //         group of one to three columns is written the same way (its other columns hold nothing anybody reads) wherever whole
    //         groups fit a middle row's bytes, 3 ceil(ql / 4) <= ql: every ql but 1, 2 and 5.  For those three the last group keeps
    //         the wide records, [column][lane] uint2 {H, E}, where the group starts (tail_wide: ql is the wave's, so this is a
    //         property of the WAVE).  The narrow kernels never store the last row.
    //   ck    checkpoint (strip, block) still starts at dword ((strip (nb - 1) + block - 1) 64) 64 of `ck` (16 KB each) and is twelve
    //         [lane] uint4: 0 .. 7 = H of rows 4 x .. 4 x + 3, 8 .. 11 = the differences H - (gap value) of rows 8 x .. 8 x + 7, two bytes
    //         per row (A, B): 12 KB of the 16.
    __device__ __forceinline__ static bool tail_wide(int ql) { return 3 * ((ql + 3) >> 2) > ql; } // ql = 1, 2, 5
    // where kept row 16 m starts (bytes from `rows`): ONE formula for carry rows (m even) and middle rows (m odd)
    __device__ __forceinline__ unsigned kept_row_off(int m, int ql) const { return (unsigned)((m >> 1) * ((ql + 1 - (m & 1)) * 512)) + (unsigned)(m & 1) * (8u * mid_off); }
    // H of column j (>= 1) of kept row 16 m; `wide`: the column stands in a last group of wide records
    __device__ __forceinline__ unsigned kept_h_off(int m, int ql, int j, bool &wide) const
    {
        const int c = j - 1;
        const unsigned group = kept_row_off(m, ql) + (unsigned)((c >> 2) * 1536);
        wide = tail_wide(ql) && (c >> 2) == ((ql - 1) >> 2);
        return group + (wide ? (unsigned)((c & 3) * 512) + 8u * lane : (unsigned)((c & 3) * 4) + 16u * lane);
    }
    template <bool NARROW>
    __device__ __forceinline__ unsigned row16_h(int m, int ql, int j) const // H alone of row 16 m at column j (>= 1), both pairs
    {
        if (!NARROW) return row16(m, ql, j).x; // (the wide kernels: the code they had before there were two forms)
        bool wide;
        return at32<unsigned>(rows, kept_h_off(m, ql, j, wide));
    }
    // {H, E} of row 16 m at column j (>= 1), one column at a time (NARROW: what ck_block falls back to where the wave has a wide tail)
    template <bool NARROW>
    __device__ __forceinline__ uint2 row16_n(int m, int ql, int j) const
    {
        if (!NARROW) return row16(m, ql, j);
        const int c = j - 1;
        bool wide;
        const unsigned hoff = kept_h_off(m, ql, j, wide);
        const unsigned soff = wide ? hoff + 4u : kept_row_off(m, ql) + (unsigned)((c >> 2) * 1536 + 1024 + ((c >> 1) & 1) * 4) + 8u * lane;
        const unsigned hv = at32<unsigned>(rows, hoff), sv = at32<unsigned>(rows, soff);
        const unsigned d = __builtin_amdgcn_perm(0u, sv, (c & 1) ? 0x0c030c02u : 0x0c010c00u); // ZERO-extended: a difference reaches 255
        return make_uint2(hv, wide ? sv : pk_sub(hv, d));
    }
    __device__ __forceinline__ unsigned qblock(int blk4, int half) const { return at32<unsigned>(seq, 4u * ((unsigned)((2 * blk4 + half) * 64) + lane)); }
    __device__ __forceinline__ unsigned tblock(int blk4, int half) const { return at32<unsigned>(seq, 4u * (t_off + (unsigned)((2 * blk4 + half) * 64) + lane)); }
    __device__ __forceinline__ unsigned flags(int cc, int r4) const { return at32<unsigned>(blku, 4u * ((unsigned)(cc * 256 + r4) + 4u * lane)); } // the block's flags: column cc, rows 4 r4 ..
};

// ---- pass 2: the walk of one pair (calculateCigar, sw.cpp:149-255) as a machine that can stop at a block's edge and go on in
// the next block.  (pi, pj) is the cell whose flags it needs next: the current cell, or the cell a gap run is counting through
// (TbView::vrun / hrun taken apart).
struct WinShift { // what alignbyte takes for the dwords of a walk's two windows (PathWalk::win_load, win64_load)
    unsigned t, q;
};
struct PathWalk {
    int I, J, pi, pj, n, seg;
    int hc;     // mode 0: H[I][J], the score of the cell the walk stands at
    int mode;   // 0: at a cell; 1: counting a vertical run (sw.cpp:73-82); 2: a horizontal one (sw.cpp:84-93)
    char state;
    bool done;
    bool stuck; // the stretch above (I, J) does not add up: the walk needs this block's flags
    SeqBlocks ts, qs; // BlockGeom::direct: the pair's target and query in the caller's arrays
    CigarWriter cw;

    __device__ __forceinline__ void take(char next, int step)
    {
        if (next == state) {
            seg += step;
        } else {
            cw.push_front(state, seg);
            seg = step;
            state = next;
        }
    }
    // h_corner: H[tl][ql], where the walk of SW_OS_INDEL starts
    __device__ __forceinline__ void start(const TbArgs &a, const DpRecord &r, int64_t o, int tl, int ql, bool ok, int h_corner)
    {
        cw.slot = a.cigar + (size_t)o * a.cigar_stride;
        cw.binary = a.binary_cigar;
        cw.cap = a.binary_cigar ? (a.cigar_stride & ~3) : a.cigar_stride;
        cw.pos = cw.cap;
        cw.need = 0;
        seg = 0;
        if (a.strategy == OS_INDEL) { // sw.cpp:155-170
            I = tl;
            J = ql;
            hc = h_corner;
        } else if (a.strategy != OS_LEAD_ID) {
            I = r.max_t;
            J = r.max_q;
            seg = r.seg;
            hc = r.max;
        } else {
            I = r.mqe_t;
            J = ql;
            hc = r.mqe;
        }
        done = !ok;
        stuck = false;
        if (ok && seg > 0 && a.strategy == OS_SOFTCLIP) { // sw.cpp:173-176
            cw.push_front('S', seg);
            seg = 0;
        }
        state = 'M';
        mode = 0;
        n = 0;
        pi = I;
        pj = J;
    }
    // One ROUND of the walk inside block (k, b) = rows 16 k + 1 .. 16 k + 16, columns CK b + 1 .. CK b + CK: the flags of the next
    // LOOK cells along the walk's current direction -- the diagonal (mode 0), up the column (a vertical run), left along the row (a
    // horizontal one) -- are fetched at once (load()), then taken as far as they allow (apply()).  The addresses do not depend on
    // what the cells hold, so a round costs one memory latency however long the run; the caller issues the loads of both pairs of
    // the lane before it applies either.  Flag bits of row t of a dword (sw_lane_cell.h): byte h = {E > max(diag, F): bit 2t+1,
    // F opened: 2t}, byte 2 + h = {F > diag: 2t+1, E opened: 2t}.
    static constexpr int LOOK = 16;
    __device__ __forceinline__ bool can_load(int k, int b) const
    {
        return !done && pi >= 1 && pj >= 1 && ((pi - 1) >> 4) == k && (pj - 1) / CK == b;
    }
    __device__ __forceinline__ void load(const WaveMem &wm, unsigned (&w)[LOOK]) const
    {
        const int rr = (pi - 1) & (RB - 1), cl = (pj - 1) & (CK - 1);
        const int di = mode != 2, dj = mode != 1;
#pragma unroll
        for (int u = 0; u < LOOK; ++u) { // (cells past the block's edge: some valid address, masked in apply())
            const int r = max(rr - u * di, 0), cc = max(cl - u * dj, 0);
            w[u] = wm.flags(cc, r >> 2);
        }
    }
    // returns false when the walk cannot go on inside this block (finished, or the cell it needs next is in another block)
    // (tw, qw: win_load() of the cell the walk stands at -- mode 0 only: the scores of the diagonal steps it takes)
    __device__ __forceinline__ bool apply(const unsigned (&w)[LOOK], const unsigned (&tw)[5], const unsigned (&qw)[5], const WinShift sh, int half,
                                          int k, int b, const BlockGeom &g)
    {
        char op = 0; // the CIGAR element this round completes, if any: taken in ONE place (take() is a large piece of code)
        int len = 0;
        const bool more = moves(w, tw, qw, sh, half, k, b, g, op, len);
        if (len > 0) take(op, len);
        return more;
    }
    __device__ __forceinline__ bool moves(const unsigned (&w)[LOOK], const unsigned (&tw)[5], const unsigned (&qw)[5], const WinShift sh, int half,
                                          int k, int b, const BlockGeom &g, char &op, int &len)
    {
        if (done) return false;
        if (mode == 1 && pi < 1) { // the run reached the matrix's top (TbView::vrun: r >= 1)
            op = 'D';
            len = n;
            I -= n;
        } else if (mode == 2 && pj < 1) {
            op = 'I';
            len = n;
            J -= n;
        } else {
            if (((pi - 1) >> 4) != k || (pj - 1) / CK != b) return false;
            const int rr = (pi - 1) & (RB - 1), cl = (pj - 1) & (CK - 1);
            const int di = mode != 2;
            const int room = mode == 0 ? min(rr, cl) : mode == 1 ? rr : cl; // cells beyond the first that lie inside the block
            // what stops the run: a cell that is not a diagonal move / opens the vertical gap / opens the horizontal gap
            const unsigned stop = (mode == 0 ? 0x00020002u : mode == 1 ? 0x00010000u : 0x00000001u) << (8 * half);
            int cnt = 0;
            unsigned at_stop = 0; // mode 0: is the cell that ended the diagonal run a vertical move (E > max(diag, F))?
#pragma unroll
            for (int u = 0; u < LOOK; ++u) {
                const int t2 = ((rr - u * di) & 3) * 2;
                if (cnt == u && u <= room) {
                    if ((w[u] & (stop << t2)) == 0u)
                        cnt = u + 1;
                    else
                        at_stop = w[u] & ((0x2u << (8 * half)) << t2);
                }
            }
            if (mode == 0) {
                if (cnt > 0) {
                    hc -= cnt * g.match + mismatches(tw, qw, sh, cnt, g.codes) * (g.mismatch - g.match);
                    op = 'M';
                    len = cnt;
                    I -= cnt;
                    J -= cnt;
                }
                if (cnt <= room) { // the run ended at a gap cell of this block (BitsMoves::at: the vertical move first)
                    const bool vertical = at_stop != 0u;
                    mode = vertical ? 1 : 2;
                    n = 1;
                    pi = vertical ? I - 1 : I;
                    pj = vertical ? J : J - 1;
                    return true; // (an edge of the matrix or of the block right behind it: the next round sees that)
                }
            } else if (mode == 1) {
                n += cnt;
                pi -= cnt;
                if (cnt == LOOK && cnt <= room) return true; // more of the run in this block than one round looks at
                if (cnt > room && pi >= 1) return false; // every cell up to the block's edge extends the gap: goes on in the block above
                hc += g.gopen + (n - 1) * g.gext; // H[I][J] = E = H[I - n][J] - o - (n - 1) e (sw.cpp:73-82)
                op = 'D';
                len = n;
                I -= n;
            } else {
                n += cnt;
                pj -= cnt;
                if (cnt == LOOK && cnt <= room) return true;
                if (cnt > room && pj >= 1) return false;
                hc += g.gopen + (n - 1) * g.gext; // sw.cpp:84-93
                op = 'I';
                len = n;
                J -= n;
            }
        }
        mode = 0;
        pi = I;
        pj = J;
        done = !(I > 0 && J > 0); // sw.cpp:214
        return !done && ((pi - 1) >> 4) == k && (pj - 1) / CK == b;
    }
    // ---- cells that need no flags: a diagonal stretch whose scores add up.  Along any diagonal stretch c0, c1 .. cL the diagonal
    // candidate of sw.cpp:51-55 gives H[ck] >= H[ck-1] + s(ck) (s = match or mismatch by the two bases); if H[cL] - H[c0] EQUALS
    // the sum of the L substitution scores, every one of these inequalities is tight, so in every cell of the stretch the diagonal
    // candidate is the maximum, sw.cpp:60-62 records btr = 0 (the diagonal wins ties), and the walk of sw.cpp:182-214 takes L
    // diagonal steps -- whatever the stretch contains (substitutions included) and whatever the penalties are.  The walk knows H of
    // the cell it stands at (hc: the start cell's score is in the record, a diagonal step subtracts s, a gap run of n adds
    // o + (n-1) e: sw.cpp:73-93), pass 1 kept H of every 16th row (WaveMem) and the borders are formulas, so one round
    // checks the stretch from the walk's cell up to the next recorded row (or the matrix's edge) with one look at that row's H and
    // at most 16 bases of both sequences (their staged copies: [4-base block][A | B][lane] dwords).  Only where the sum does NOT
    // fit -- a gap, or a tie taken elsewhere -- does the walk need the flags of the block.
    __device__ __forceinline__ bool can_verify() const { return !done && mode == 0 && !stuck; }
    // bases I - 16 .. I - 1 (0-based) of the target and J - 16 .. J - 1 of the query: byte 15 of the window belongs to cell (I, J).
    // Returns what alignbyte takes to bring dwords k, k + 1 of either window to its bases 4 k .. 4 k + 3.  g.direct (wave-uniform,
    // one value per launch): out of the caller's arrays, two 16-byte loads per sequence -- else the staged dwords, five per sequence.
    __device__ __forceinline__ WinShift win_load(const WaveMem &wm, int half, int tblocks, int qblocks, const BlockGeom &g, unsigned (&tw)[5], unsigned (&qw)[5]) const
    {
        WinShift sh;
        if (g.direct) {
            sh.t = ts.window<16>(I, g.tl, tw);
            sh.q = qs.window<16>(J, g.ql, qw);
            return sh;
        }
        const int dt = (I - 16) >> 2, dq = (J - 16) >> 2;
#pragma unroll
        for (int k = 0; k < 5; ++k) { // (blocks before the sequence: block 0 again -- those bytes are never counted)
            tw[k] = wm.tblock(min(max(dt + k, 0), tblocks - 1), half);
            qw[k] = wm.qblock(min(max(dq + k, 0), qblocks - 1), half);
        }
        sh.t = (unsigned)(I - 16) & 3u;
        sh.q = (unsigned)(J - 16) & 3u;
        return sh;
    }
    // how many of the cells (I, J), (I-1, J-1) .. (I-L+1, J-L+1) hold different bases (raw byte compare, sw.cpp:55); L <= 16, I, J
    // (codes: the staged target holds codes 0 .. 3, the staged query 8 x code or 32 -- sw_lane_cell.h; sh: win_load()'s)
    __device__ __forceinline__ int mismatches(const unsigned (&tw)[5], const unsigned (&qw)[5], const WinShift sh, int L, bool codes) const
    {
        const unsigned st = sh.t, sq = sh.q;
        const int drop = 16 - L, dq = drop >> 2, cut = (drop & 3) * 8; // the window's low `drop` bytes are not part of the stretch
        int n = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned tt = __builtin_amdgcn_alignbyte(tw[k + 1], tw[k], st);
            const unsigned nz = nonzero_bytes((codes ? tt << 3 : tt) ^ __builtin_amdgcn_alignbyte(qw[k + 1], qw[k], sq));
            n += __popc(k > dq ? nz : k == dq ? nz >> cut : 0u);
        }
        return n;
    }
    // One round checks up to VB stretches at once -- from the walk's cell to each of the next VB kept rows: 64 bases of both
    // sequences and the VB rows' H are fetched together, their addresses depend on nothing the round computes -- and takes the
    // longest one that adds up (if the stretch to a row adds up, so does the stretch to every row before it).
    static constexpr int VB = 4;
    // (g.direct: five 16-byte loads per sequence out of the caller's arrays; else seventeen staged dwords)
    __device__ __forceinline__ WinShift win64_load(const WaveMem &wm, int half, int tblocks, int qblocks, const BlockGeom &g, unsigned (&tw)[17], unsigned (&qw)[17]) const
    {
        WinShift sh;
        if (g.direct) {
            sh.t = ts.window<64>(I, g.tl, tw);
            sh.q = qs.window<64>(J, g.ql, qw);
            return sh;
        }
        const int dt = (I - 64) >> 2, dq = (J - 64) >> 2;
#pragma unroll
        for (int k = 0; k < 17; ++k) {
            tw[k] = wm.tblock(min(max(dt + k, 0), tblocks - 1), half);
            qw[k] = wm.qblock(min(max(dq + k, 0), qblocks - 1), half);
        }
        sh.t = (unsigned)(I - 64) & 3u;
        sh.q = (unsigned)(J - 64) & 3u;
        return sh;
    }
    // the stretch to the m-th kept row above the walk's cell (m = 0: the next one), cut where the diagonal leaves the matrix
    __device__ __forceinline__ int stretch_to(int m) const { return min(I - max((((I - 1) >> 4) - m) << 4, 0), J); }
    // H of those rows in stored form (both pairs of the lane)
    template <bool NARROW>
    __device__ __forceinline__ void grid_load(const WaveMem &wm, int ql, unsigned (&w)[VB]) const
    {
#pragma unroll
        for (int m = 0; m < VB; ++m) {
            const int L = stretch_to(m), ie = I - L, je = J - L;
            w[m] = wm.row16_h<NARROW>(ie >> 4, ql, max(je, 1)); // (a stretch that ends on a border: some valid entry, not used)
        }
    }
    // returns true when all VB stretches were taken and the walk can try the next ones
    __device__ __forceinline__ bool verify_apply(const unsigned (&tw)[17], const unsigned (&qw)[17], const WinShift sh, const unsigned (&w)[VB], int half,
                                                 const BlockGeom &g)
    {
        if (!can_verify()) return false;
        // bit u of `differ`: the bases of cell (I - u, J - u) differ (byte 63 - u of the window)
        const unsigned st = sh.t, sq = sh.q;
        unsigned long long differ = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const unsigned tt = __builtin_amdgcn_alignbyte(tw[k + 1], tw[k], st);
            const unsigned nz = nonzero_bytes((g.codes ? tt << 3 : tt) ^ __builtin_amdgcn_alignbyte(qw[k + 1], qw[k], sq)) >> 7;
            const unsigned nib = ((nz * 0x08040201u) >> 24) & 0xfu; // byte 3 -> bit 0 .. byte 0 -> bit 3
            differ |= (unsigned long long)nib << (4 * (15 - k));
        }
        int took = 0, h_at = hc;
        bool all = true;
#pragma unroll
        for (int m = 0; m < VB; ++m) {
            const int L = stretch_to(m), ie = I - L, je = J - L;
            const int he = ie == 0 ? border(je, g.gopen, g.gext, g.indel)
                         : je == 0 ? border(ie, g.gopen, g.gext, g.indel)
                                   : (half ? hi16(w[m]) : lo16(w[m])) - (ie + je) * g.gext - g.base;
            const unsigned long long in = L >= 64 ? ~0ull : (1ull << L) - 1ull;
            const bool ok = hc - he == L * g.match + __popcll(differ & in) * (g.mismatch - g.match);
            took = ok ? L : took; // (the stretches that add up are the first ones: each contains the one before)
            h_at = ok ? he : h_at;
            all = all && ok;
        }
        stuck = !all; // the first stretch that does not add up holds a gap (or a tie taken elsewhere): this block's flags, then
        if (took > 0) {
            take('M', took);
            I -= took;
            J -= took;
            hc = h_at;
            pi = I;
            pj = J;
            done = !(I > 0 && J > 0); // sw.cpp:214
        }
        return all && !done;
    }
    // ---- the kept COLUMN.  A stuck walk is about to have the block it stands in recomputed -- but the stretch that failed is up to
    // 16 cells long and a block only CK columns wide: where the diagonal leaves the block through its left edge before it reaches the
    // kept row, the gap may lie beyond that edge, the recomputed block holds nothing but diagonal moves, and the block behind the
    // edge is recomputed for the same gap.  The left edge of block b is a kept column just as row 16 m is a kept row: pass 1's
    // checkpoints hold H[row][CK b] of every row (h[r] of ck_strip's save(), what ck_block starts from), and the proof above holds
    // for any end cell whose H is known.  So before the block round a stuck walk checks the stretch to the EDGE (I - Lc, CK b),
    // Lc = J - CK b, where that is the nearer one (b >= 1: column 0 is a formula the row check knows; Lc < stretch_to(0): equal
    // lengths end in the cell the row check has just failed).  If it adds up the walk takes it and stands at the right edge of
    // block (k, b - 1) -- still stuck: the rest of the failed stretch, at most 15 cells, lies inside that block -- and the block
    // round picks that block from (pi, pj) by itself.  The edge cell's row is >= 1 and in the walk's own 16-row band.
    __device__ __forceinline__ int edge_len() const // 0: no such stretch
    {
        if (done || mode != 0 || !stuck) return 0;
        const int lc = J - ((J - 1) & ~(CK - 1));
        return J > CK && lc < stretch_to(0) ? lc : 0;
    }
    // H[I - lc][CK b] in stored form, both pairs of the lane (the indexing of ck_block's ia / ib)
    template <bool NARROW>
    __device__ __forceinline__ unsigned edge_load(const WaveMem &wm, int nb, int lc) const
    {
        const int r0 = I - lc - 1, b = (J - 1) / CK;
        if (NARROW) // (WaveMem: the checkpoint's uint4 (r0 & 31) / 4, its dword r0 & 3)
            return WaveMem::at32<unsigned>(wm.cku, (unsigned)(((r0 >> 5) * (nb - 1) + (b - 1)) * 16384 + ((r0 & (R - 1)) >> 2) * 1024 + (r0 & 3) * 4) + 16u * wm.lane);
        return WaveMem::at32<unsigned>(wm.cku, 4u * ((unsigned)((((r0 >> 5) * (nb - 1) + (b - 1)) * 64 + 2 * (r0 & (R - 1))) * 64) + wm.lane));
    }
    // (tw, qw, sh: win_load() of the walk's cell.)  Returns true when the stretch was taken.
    __device__ __forceinline__ bool edge_apply(const unsigned w, const unsigned (&tw)[5], const unsigned (&qw)[5], const WinShift sh, int lc, int half,
                                               const BlockGeom &g)
    {
        if (lc == 0) return false;
        const int ie = I - lc, je = J - lc;
        const int he = (half ? hi16(w) : lo16(w)) - (ie + je) * g.gext - g.base;
        if (hc - he != lc * g.match + mismatches(tw, qw, sh, lc, g.codes) * (g.mismatch - g.match)) return false;
        take('M', lc);
        I = ie;
        J = je;
        hc = he;
        pi = I;
        pj = J; // (I >= 1 and J = CK b >= CK: not done)
        return true;
    }
    // overhangs, text, per-pair results (walk_and_write's tail + traceback_one_pair)
    // (rp: the pair's record where pass 1 left it in memory -- read back here, by the lane that wrote it, rather than carried in a dozen
    // registers through the whole of pass 2)
    __device__ __forceinline__ void finish(const TbArgs &a, const DpRecord *rp, int64_t o)
    {
        int off;
        if (a.strategy == OS_SOFTCLIP) { // sw.cpp:225-229
            cw.push_front(state, seg);
            if (J > 0) cw.push_front('S', J);
            off = I;
        } else if (a.strategy == OS_IGNORE) { // sw.cpp:230-233
            cw.push_front(state, seg + J);
            off = I - J;
        } else { // sw.cpp:234-248
            cw.push_front(state, seg);
            if (I > 0)
                cw.push_front('D', I);
            else if (J > 0)
                cw.push_front('I', J);
            off = 0;
        }
        const int status = finish_cigar(cw);
        for (int x = cw.cap; x < a.cigar_stride; ++x) cw.slot[x] = 0;
        a.offset[o] = off;
        if (a.cigar_len) a.cigar_len[o] = cw.need;
        if (a.status) a.status[o] = status;
        if (a.status_any && status != 0) atomicMax(a.status_any, status);
        if (a.score) {
            const DpRecord r = *rp;
            Score sc;
            sc.mqe = r.mqe;
            sc.mqe_t = r.mqe_t;
            sc.max = r.max;
            sc.max_t = r.max_t;
            sc.max_q = r.max_q;
            sc.seg_length = r.seg;
            a.score[o] = sc;
        }
    }
};

// ---- the last row (sw.cpp:116-127) as ONE running key per lane half.  The reference scans H[tl][1 .. ql] for the largest score, among
// equal scores the smallest |tl - j|, among those the earlier column.  The last strip keeps that running best while it sweeps the
// columns, so the row is neither stored nor read back:
//   frame   a stored H[tl][j] is X + (tl + j) e + base (X the score).  w = stored + (ql - j) e = X + (tl + ql) e + base does not depend
//           on the column, so two columns' w compare as their scores do.  Range: base = 32767 - match min(tl, ql) - e (tl + ql)
//           (dp16_base) makes w = X + 32767 - match min(tl, ql), and X <= match min(i, j) <= match min(tl, ql): w <= 32767, no
//           overflow; (ql - j) e >= 0 and every stored value of the matrix is >= -32768 (dp16_range_ok): w >= stored, no underflow.
//           So the wrapping packed add is exact in both halves.
//   pref    row_pref(j) = ql - 1 - (the number of columns the reference prefers to j at equal score): a wave-uniform number in
//           [0, ql - 1], one value per column (the preference is a strict total order), larger = preferred.
//   key     (w << 16) | pref as a signed 32-bit integer: the larger key is the column the reference keeps, two columns never have
//           equal keys, and the winner's w and j are read back from it once, after the strip (row_col).
// pref fits the key's low half for ql <= ROW_KEY_MAX_QL whatever tl is.  The kernel also accepts longer queries (gext = 0 leaves the
// longer side of a pair unbounded, dp16_range_ok): those launches store the row and scan it after pass 1 as before (LAST_ROW_STORED).
constexpr int ROW_KEY_MAX_QL = 65536;
// columns of 1 .. ql that come before j in the reference's order at equal score: those strictly nearer to tl, and j's mirror image on
// the left of tl where j lies on the right and the mirror is a column
__device__ __forceinline__ int row_pref(const int tl, const int ql, const int j)
{
    const int d = abs(tl - j);
    const int nearer = max(min(ql, tl + d - 1) - max(1, tl - d + 1) + 1, 0);
    return ql - 1 - nearer - ((j > tl && tl - d >= 1) ? 1 : 0);
}
// the column whose row_pref is `pref`
__device__ __forceinline__ int row_col(const int tl, const int ql, const int pref)
{
    const int r = ql - 1 - pref;
    if (tl > ql) return ql - r; // every column lies left of tl: the nearest is the last
    const int m = min(tl - 1, ql - tl); // distances 1 .. m have a column on either side of tl
    if (r <= 2 * m) return (r & 1) ? tl - ((r + 1) >> 1) : tl + (r >> 1);
    return tl - 1 > m ? tl - (r - m) : tl + (r - m); // the longer side alone
}

// what a strip is to the last row
enum : int {
    NOT_LAST = 0,
    LAST_ROW_KEYS = 1,   // the last strip: the running keys above
    LAST_ROW_STORED = 2, // the last strip of a launch with ql > ROW_KEY_MAX_QL: H[tl][j] goes to the carry row "entering strip `strips`"
};

// ---- pass 1: strip k, score only, keeping the rows and the column checkpoints
// (keyA / keyB: the last row's running keys; corner: H[tl][ql] of both halves in stored form -- the last strip only)
template <int LAST, int CODES, bool NARROW>
__device__ __forceinline__ void ck_strip(const int k, const int tl, const int ql, const int nb, const WaveMem &wm, const unsigned *qst, const unsigned *tst,
                                         const LaneConsts &c, const int gopen, const int gext, const int base, const bool indel, int &bestA,
                                         int &bestA_i, int &bestB, int &bestB_i, int &keyA, int &keyB, unsigned &corner)
{
    const int i0 = k * R;
    unsigned h[R], f[R], t[R];
#pragma unroll
    for (int r4 = 0; r4 < R / 4; ++r4) {
        const unsigned ta = tst[(size_t)(2 * ((i0 >> 2) + r4)) * 64], tb = tst[(size_t)(2 * ((i0 >> 2) + r4) + 1) * 64];
        t[4 * r4 + 0] = __builtin_amdgcn_perm(tb, ta, 0x0c040c00u) | (CODES ? CODE_SEL : 0u);
        t[4 * r4 + 1] = __builtin_amdgcn_perm(tb, ta, 0x0c050c01u) | (CODES ? CODE_SEL : 0u);
        t[4 * r4 + 2] = __builtin_amdgcn_perm(tb, ta, 0x0c060c02u) | (CODES ? CODE_SEL : 0u);
        t[4 * r4 + 3] = __builtin_amdgcn_perm(tb, ta, 0x0c070c03u) | (CODES ? CODE_SEL : 0u);
    }
    // column 0 (sw.cpp:24,38,47-49), as in sw_dp16_lane.hip
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int row = i0 + r + 1;
        const int hb = border(row, gopen, gext, indel) + row * gext + base;
        h[r] = pack2(hb, hb);
        f[r] = pk_sub(h[r], c.o_e);
    }
    const int rl = tl - 1 - i0;

    const uint2 *bp = wm.bnd + ((size_t)k * (ql + 1) + 1) * 64; // column j of the row entering this strip
    uint2 *bo = wm.bnd + ((size_t)(k + 1) * (ql + 1) + 1) * 64; // ... of the row leaving it
    uint2 *mp = wm.mid + (size_t)k * ql * 64;
    // NARROW: where the strip's groups and checkpoints go, as WAVE-UNIFORM bases (scalar registers, moved on by scalar adds) beside 32-bit
    // lane offsets -- the two record sizes of a group as two POINTERS that include the lane were four registers and spilled in the loops
    char *mg = reinterpret_cast<char *>(const_cast<uint2 *>(wm.rows)) + (size_t)8 * wm.mid_off + (size_t)k * ql * 512;
    char *cg = reinterpret_cast<char *>(const_cast<unsigned *>(wm.cku)) + (size_t)k * (nb - 1) * 16384;
    // ... and the groups of the carry rows (WaveMem: every kept row has the middle rows' format): `ig` the row entering the strip, `og`
    // the row leaving it
    const char *ig = reinterpret_cast<const char *>(wm.rows) + (size_t)k * (ql + 1) * 512;
    char *og = reinterpret_cast<char *>(const_cast<uint2 *>(wm.rows)) + (size_t)(k + 1) * (ql + 1) * 512;
    const bool tail_wide = WaveMem::tail_wide(ql); // (wave-uniform: the last group of one or two columns keeps the wide records)
    unsigned l16 = 16u * wm.lane, l8 = 8u * wm.lane;
    // (NARROW: the strip's own copies.  A wave keeps its slot, so base + lane offset of every array is invariant in the kernel's tile
    // loop: computed once in front of it, each a register pair, and with the carry rows' two more than the registers hold -- kept in
    // scratch for the kernel's whole life.  Two adds per strip instead.)
    if (NARROW) asm volatile("" : "+v"(l16), "+v"(l8));
    unsigned mh[4] = {0u, 0u, 0u, 0u}, md0 = 0u, md[2] = {0u, 0u}; // NARROW: the group's four H and its difference bytes so far
    unsigned me[2] = {0u, 0u};                                     // ... and E of its first two columns (a last group of wide records)
    unsigned ch[4] = {0u, 0u, 0u, 0u}, cd0 = 0u, cd[2] = {0u, 0u}, ce[2] = {0u, 0u}; // the same of the row that leaves the strip
    unsigned *ckp = wm.ck + (size_t)k * (nb - 1) * 64 * 64;
    unsigned hd; // H[32 k][0]
    if (NARROW) { // (column 0 of a kept row is not stored: the border's formula, as in `column 0` above)
        const int hb = border(i0, gopen, gext, indel) + i0 * gext + base;
        hd = pack2(hb, hb);
    } else {
        hd = bp[-64].x;
    }
    // column u (0 .. 3) of the group whose query dwords are qa / qb
    int j = 1;
    // (tail: a column of the last, partial group -- only there E of a kept cell may leave as a wide record's second dword)
    auto one_column = [&](const uint2 top, const unsigned qa, const unsigned qb, const int u, const bool tail = false) {
        unsigned e = top.y;
        uint2 mid;
        if (CODES)
            column<R, true, true, CODES>(h, f, t, code_table((qa >> (8 * u)) & 0xffu, c.bm, c.bx), hd, e, c, nullptr, &mid, code_table((qb >> (8 * u)) & 0xffu, c.bm, c.bx));
        else
            column<R, true, true, false>(h, f, t, __builtin_amdgcn_perm(qb, qa, 0x0c040c00u + 0x00010001u * u), hd, e, c, nullptr, &mid);
        hd = top.x;
        if (NARROW) { // (stored once per group: mid_group below)
            mh[u] = mid.x;
            if (tail && u < 2) me[u] = mid.y;
            const unsigned d = pk_sub(mid.x, mid.y);
            if (u & 1)
                md[u >> 1] = __builtin_amdgcn_perm(d, md0, 0x06040200u); // bytes {A, B} of column u - 1, {A, B} of column u
            else
                md0 = d;
        } else {
            if (!(MGL_CK_ABLATE & 4)) mp[0] = mid;
            mp += 64;
        }
        if (NARROW) { // the row that leaves the strip: once per group as well (carry_group below); the last strip's is never stored
            if (LAST == NOT_LAST) {
                ch[u] = h[R - 1];
                if (tail && u < 2) ce[u] = e;
                const unsigned d = pk_sub(h[R - 1], e);
                if (u & 1)
                    cd[u >> 1] = __builtin_amdgcn_perm(d, cd0, 0x06040200u);
                else
                    cd0 = d;
            }
        } else if (LAST == NOT_LAST) {
            bo[0] = make_uint2(h[R - 1], e);
        }
        if (LAST != NOT_LAST) { // H[tl][j]
            unsigned bot = h[R - 1];
            if (rl != R - 1) {
#pragma unroll
                for (int r = 0; r < R - 1; ++r) bot = (r == rl) ? h[r] : bot;
            }
            if (LAST == LAST_ROW_STORED) {
                bo[0] = make_uint2(bot, 0u);
            } else { // (the frame constant and pref are wave-uniform: scalar arithmetic beside the column's packed instructions)
                const int jc = j + u, lift = (ql - jc) * gext;
                const unsigned w = pk_add(bot, pack2(lift, lift)), pref = (unsigned)row_pref(tl, ql, jc);
                keyA = max(keyA, (int)((w << 16) | pref));
                keyB = max(keyB, (int)((w & 0xffff0000u) | pref));
            }
        }
        if (LAST != LAST_ROW_KEYS) bo += 64;
    };
    auto mid_group = [&](const int cols) { // NARROW: the group's `cols` columns (1 .. 4) leave in two stores
        if (cols & 1) md[cols >> 1] = __builtin_amdgcn_perm(md0, md0, 0x06040200u); // (an odd column's bytes wait in md0 for a neighbour)
        if (!(MGL_CK_ABLATE & 4)) {
            *reinterpret_cast<uint4 *>(mg + l16) = make_uint4(mh[0], mh[1], mh[2], mh[3]);
            *reinterpret_cast<uint2 *>(mg + 1024 + l8) = make_uint2(md[0], md[1]);
        }
        mg += 1536;
    };
    auto carry_group = [&](const int cols) { // ... and so does the row that leaves the strip (NARROW, LAST == NOT_LAST)
        if (cols & 1) cd[cols >> 1] = __builtin_amdgcn_perm(cd0, cd0, 0x06040200u);
        *reinterpret_cast<uint4 *>(og + l16) = make_uint4(ch[0], ch[1], ch[2], ch[3]);
        *reinterpret_cast<uint2 *>(og + 1024 + l8) = make_uint2(cd[0], cd[1]);
        og += 1536;
    };
    auto save = [&]() { // the state BEFORE column j: H[.][j-1] and the horizontal-gap values entering column j
        if (NARROW) {
#pragma unroll
            for (int x = 0; x < R / 4; ++x) *reinterpret_cast<uint4 *>(cg + x * 1024 + l16) = make_uint4(h[4 * x], h[4 * x + 1], h[4 * x + 2], h[4 * x + 3]);
#pragma unroll
            for (int x = 0; x < R / 8; ++x) {
                unsigned d[4];
#pragma unroll
                for (int y = 0; y < 4; ++y) { // rows 8 x + 2 y and the next: bytes {A, B, A, B}
                    const int r = 8 * x + 2 * y;
                    d[y] = __builtin_amdgcn_perm(pk_sub(h[r + 1], f[r + 1]), pk_sub(h[r], f[r]), 0x06040200u);
                }
                *reinterpret_cast<uint4 *>(cg + (R / 4 + x) * 1024 + l16) = make_uint4(d[0], d[1], d[2], d[3]);
            }
            cg += 16384;
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                ckp[(size_t)(2 * r) * 64] = h[r];
                ckp[(size_t)(2 * r + 1) * 64] = f[r];
            }
            ckp += 64 * 64;
        }
    };
    // The carry row and the query are read ONE GROUP OF FOUR COLUMNS AHEAD: what a group needs was requested at the top of the
    // group before it, so its latency hides behind a thousand instructions of arithmetic.  s_waitcnt vmcnt counts loads and stores in
    // one queue, in order, so a wait for those loads may leave in flight exactly the stores issued behind them -- the group's own
    // kept-row stores -- and the compiler counts them where every path into the wait has issued the same operations.  The loop's
    // header is not such a place: the prologue arrives with its loads newest in the queue, the latch with the group's stores
    // behind them, and the merged wait was vmcnt(0) -- every group drained the stores it had just issued.  So the prefetched
    // values are CONSUMED where the paths are still apart (the empty asm statements: once in front of the loop, the full wait, once
    // per strip; and at the bottom of the body, behind the stores): each wait then stands in the body with its own count, none at
    // the header, and a group's stores have until the next group's loads are consumed.  scripts/lane_ck_waits.py lists the waits
    // of a build; a count is right when the newest operation it waits for is a load (docs/history.md C.000f).
    // Reads past column ql stay inside the wave's own region (the next kept row follows; the narrow kernels' last carry row,
    // "entering strip `strips`", is allocated and never written) and are never used.
    if (NARROW) {
        // the group's H as one 16-byte vector and its difference bytes as one 8-byte vector; E of a column is H minus its zero-extended
        // byte.  (A wave with a wide tail, ql = 1, 2, 5, fetches a narrow group where its tail stands -- inside the row, not used -- and
        // its two wide records below, in front of the tail's columns: the only load of pass 1 that is waited for where it is issued,
        // once per strip of a query of at most five columns.  Fetched a group ahead they would be four more registers live through
        // every wave's loop, or a branch at every group's loads.)
        uint4 nh;
        uint2 nd;
        auto fetch = [&]() {
            nh = *reinterpret_cast<const uint4 *>(ig + l16);
            nd = *reinterpret_cast<const uint2 *>(ig + 1024 + l8);
            ig += 1536;
        };
        auto top = [&](const uint4 th, const uint2 td, const int u) {
            const unsigned hv = u == 0 ? th.x : u == 1 ? th.y : u == 2 ? th.z : th.w;
            const unsigned d = __builtin_amdgcn_perm(0u, u < 2 ? td.x : td.y, (u & 1) ? 0x0c030c02u : 0x0c010c00u); // ZERO-extended
            return make_uint2(hv, pk_sub(hv, d));
        };
        fetch();
        unsigned nqa = qst[0], nqb = qst[64];
        asm volatile("" : "+v"(nh.x), "+v"(nh.y), "+v"(nh.z), "+v"(nh.w), "+v"(nd.x), "+v"(nd.y), "+v"(nqa), "+v"(nqb)); // consumed: the prologue's wait stays in front of the loop
        for (; j + 3 <= ql; j += 4) {
            if (!(MGL_CK_ABLATE & 2) && j > 1 && ((j - 1) & (CK - 1)) == 0) save(); // (column 0 is a formula: no checkpoint)
            const uint4 th = nh;
            const uint2 td = nd;
            const unsigned qa = nqa, qb = nqb;
            qst += 128;
            fetch();
            nqa = qst[0];
            nqb = qst[64];
            one_column(top(th, td, 0), qa, qb, 0);
            one_column(top(th, td, 1), qa, qb, 1);
            one_column(top(th, td, 2), qa, qb, 2);
            one_column(top(th, td, 3), qa, qb, 3);
            mid_group(4);
            if (LAST == NOT_LAST) carry_group(4);
            asm volatile("" : "+v"(nh.x), "+v"(nh.y), "+v"(nh.z), "+v"(nh.w), "+v"(nd.x), "+v"(nd.y), "+v"(nqa), "+v"(nqb)); // consumed behind the group's stores: no wait at the header
        }
        if (j <= ql) { // the last one to three columns (j - 1 is a multiple of four here)
            if (j > 1 && ((j - 1) & (CK - 1)) == 0) save();
            const int cols = ql - j + 1;
            uint2 t0 = top(nh, nd, 0), t1 = top(nh, nd, 1);
            if (tail_wide) { // one or two columns as wide records, where the group starts (`ig` has moved past it)
                t0 = *reinterpret_cast<const uint2 *>(ig - 1536 + l8);
                t1 = *reinterpret_cast<const uint2 *>(ig - 1024 + l8);
            }
            one_column(t0, nqa, nqb, 0, true);
            if (cols >= 2) one_column(t1, nqa, nqb, 1, true);
            if (cols >= 3) one_column(top(nh, nd, 2), nqa, nqb, 2, true);
            if (!tail_wide) { // a whole group like every other; the columns past ql hold nothing anybody reads
                mid_group(cols);
                if (LAST == NOT_LAST) carry_group(cols);
            } else {
                if (!(MGL_CK_ABLATE & 4)) {
                    *reinterpret_cast<uint2 *>(mg + l8) = make_uint2(mh[0], me[0]);
                    if (cols >= 2) *reinterpret_cast<uint2 *>(mg + 512 + l8) = make_uint2(mh[1], me[1]);
                }
                if (LAST == NOT_LAST) {
                    *reinterpret_cast<uint2 *>(og + l8) = make_uint2(ch[0], ce[0]);
                    if (cols >= 2) *reinterpret_cast<uint2 *>(og + 512 + l8) = make_uint2(ch[1], ce[1]);
                }
            }
        }
    } else {
        uint2 n0 = bp[0], n1 = bp[64], n2 = bp[128], n3 = bp[192];
        unsigned nqa = qst[0], nqb = qst[64];
        asm volatile("" : "+v"(n0.x), "+v"(n0.y), "+v"(n1.x), "+v"(n1.y), "+v"(n2.x), "+v"(n2.y), "+v"(n3.x), "+v"(n3.y), "+v"(nqa), "+v"(nqb)); // consumed: the prologue's wait stays in front of the loop
        for (; j + 3 <= ql; j += 4) {
            if (!(MGL_CK_ABLATE & 2) && j > 1 && ((j - 1) & (CK - 1)) == 0) save(); // (column 0 is a formula: no checkpoint)
            const uint2 top0 = n0, top1 = n1, top2 = n2, top3 = n3;
            const unsigned qa = nqa, qb = nqb;
            qst += 128;
            bp += 256;
            n0 = bp[0];
            n1 = bp[64];
            n2 = bp[128];
            n3 = bp[192];
            nqa = qst[0];
            nqb = qst[64];
            one_column(top0, qa, qb, 0);
            one_column(top1, qa, qb, 1);
            one_column(top2, qa, qb, 2);
            one_column(top3, qa, qb, 3);
            asm volatile("" : "+v"(n0.x), "+v"(n0.y), "+v"(n1.x), "+v"(n1.y), "+v"(n2.x), "+v"(n2.y), "+v"(n3.x), "+v"(n3.y), "+v"(nqa), "+v"(nqb)); // consumed behind the group's stores: no wait at the header
        }
        if (j <= ql) { // the last one to three columns (j - 1 is a multiple of four here)
            if (j > 1 && ((j - 1) & (CK - 1)) == 0) save();
            one_column(n0, nqa, nqb, 0);
            if (j + 1 <= ql) one_column(n1, nqa, nqb, 1);
            if (j + 2 <= ql) one_column(n2, nqa, nqb, 2);
        }
    }
    if (LAST != NOT_LAST) { // H[tl][ql], where the walks of the non-softclip strategies start
        corner = h[R - 1];
        if (rl != R - 1) {
#pragma unroll
            for (int r = 0; r < R - 1; ++r) corner = (r == rl) ? h[r] : corner;
        }
    }
    // last column (sw.cpp:100-104), as in sw_dp16_lane.hip
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int row = i0 + r + 1;
        if (row <= tl) {
            const int unshift = -(row + ql) * gext - base;
            const int ca = lo16(h[r]) + unshift, cb = hi16(h[r]) + unshift;
            if (ca >= bestA) {
                bestA = ca;
                bestA_i = row;
            }
            if (cb >= bestB) {
                bestB = cb;
                bestB_i = row;
            }
        }
    }
}

// ---- pass 2: recompute the flags of block (sA, bA) for the low halves and of block (sB, bB) for the high halves; s = 16-row band
// (strip s / 2, its upper or lower half), b = block of CK columns.  needA / needB: the pair's walk waits for this block (a pair
// that does not fetches nothing; its half computes garbage nobody reads).
template <int CODES, bool NARROW>
__device__ __forceinline__ void ck_block(const int sA, const int bA, const int sB, const int bB, const bool needA, const bool needB, const BlockGeom &g,
                                         const WaveMem &wm, const LaneConsts &c, const int groups = CK / 8)
{
    unsigned h[RB], f[RB], t[RB];
#pragma unroll
    for (int r4 = 0; r4 < RB / 4; ++r4) {
        const unsigned ta = wm.tblock(sA * (RB / 4) + r4, 0), tb = wm.tblock(sB * (RB / 4) + r4, 1);
        t[4 * r4 + 0] = __builtin_amdgcn_perm(tb, ta, 0x0c040c00u) | (CODES ? CODE_SEL : 0u);
        t[4 * r4 + 1] = __builtin_amdgcn_perm(tb, ta, 0x0c050c01u) | (CODES ? CODE_SEL : 0u);
        t[4 * r4 + 2] = __builtin_amdgcn_perm(tb, ta, 0x0c060c02u) | (CODES ? CODE_SEL : 0u);
        t[4 * r4 + 3] = __builtin_amdgcn_perm(tb, ta, 0x0c070c03u) | (CODES ? CODE_SEL : 0u);
    }
    // the state entering the block's first column: the checkpoint of column CK b, or column 0 by its formula (sw.cpp:24,38,47-49)
    {
        const unsigned ia = (unsigned)((((sA >> 1) * (g.nb - 1) + max(bA - 1, 0)) * 64 + (sA & 1) * 2 * RB) * 64) + wm.lane;
        const unsigned ib = (unsigned)((((sB >> 1) * (g.nb - 1) + max(bB - 1, 0)) * 64 + (sB & 1) * 2 * RB) * 64) + wm.lane;
        // one half after the other (both at once: 64 registers of checkpoint values beside the 48 of the block's state -- spilled)
        unsigned v[2 * RB];
        // NARROW: the half's 16 rows are four uint4 of H and two of difference bytes (WaveMem) -- v[] as the wide form holds it
        auto load_narrow = [&](const int s, const int b) {
            const unsigned off = (unsigned)(((s >> 1) * (g.nb - 1) + max(b - 1, 0)) * 16384 + (s & 1) * 4096) + 16u * wm.lane;
            uint4 hv[RB / 4], dv[RB / 8];
#pragma unroll
            for (int x = 0; x < RB / 4; ++x) hv[x] = WaveMem::at32<uint4>(wm.cku, off + (unsigned)(x * 1024));
#pragma unroll
            for (int x = 0; x < RB / 8; ++x) dv[x] = WaveMem::at32<uint4>(wm.cku, off + (unsigned)(8192 - (s & 1) * 2048 + x * 1024));
#pragma unroll
            for (int x = 0; x < RB / 4; ++x) {
                v[8 * x + 0] = hv[x].x;
                v[8 * x + 2] = hv[x].y;
                v[8 * x + 4] = hv[x].z;
                v[8 * x + 6] = hv[x].w;
            }
#pragma unroll
            for (int x = 0; x < RB / 8; ++x) {
                const unsigned d[4] = {dv[x].x, dv[x].y, dv[x].z, dv[x].w};
#pragma unroll
                for (int y = 0; y < 4; ++y) { // rows 8 x + 2 y and the next; ZERO-extended bytes (a difference reaches 255)
                    const int r = 8 * x + 2 * y;
                    v[2 * r + 1] = pk_sub(v[2 * r], __builtin_amdgcn_perm(0u, d[y], 0x0c010c00u));
                    v[2 * r + 3] = pk_sub(v[2 * r + 2], __builtin_amdgcn_perm(0u, d[y], 0x0c030c02u));
                }
            }
        };
#pragma unroll
        for (int x = 0; x < 2 * RB; ++x) v[x] = 0u;
        if (needA && bA > 0) {
            if (NARROW) {
                load_narrow(sA, bA);
            } else {
#pragma unroll
                for (int x = 0; x < 2 * RB; ++x) v[x] = WaveMem::at32<unsigned>(wm.cku, 4u * (ia + (unsigned)(x * 64)));
            }
        }
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const int rowA = sA * RB + r + 1;
            const int fa_ = border(rowA, g.gopen, g.gext, g.indel) + rowA * g.gext + g.base;
            h[r] = bA > 0 ? v[2 * r] : (unsigned)fa_;
            f[r] = bA > 0 ? v[2 * r + 1] : (unsigned)(fa_ - (g.gopen - g.gext));
        }
#pragma unroll
        for (int x = 0; x < 2 * RB; ++x) v[x] = 0u;
        if (needB && bB > 0) {
            if (NARROW) {
                load_narrow(sB, bB);
            } else {
#pragma unroll
                for (int x = 0; x < 2 * RB; ++x) v[x] = WaveMem::at32<unsigned>(wm.cku, 4u * (ib + (unsigned)(x * 64)));
            }
        }
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const int rowB = sB * RB + r + 1;
            const int fb_ = border(rowB, g.gopen, g.gext, g.indel) + rowB * g.gext + g.base;
            const unsigned hb = bB > 0 ? v[2 * r] : (unsigned)fb_ << 16, gb = bB > 0 ? v[2 * r + 1] : (unsigned)(fb_ - (g.gopen - g.gext)) << 16;
            h[r] = lo_hi(h[r], hb);
            f[r] = lo_hi(f[r], gb);
        }
    }
    // the row entering the band, per column: row 16 s of the pair (WaveMem::row16; row 0 is the border row, kept like any other)
    unsigned hd;
    {
        unsigned a0 = 0u, b0 = 0u; // H[16 s][CK b]
        // (NARROW: no kept row stores column 0 -- the load is of column 1 then, some valid entry that is not used)
        if (needA) a0 = wm.row16_h<NARROW>(sA, g.ql, NARROW ? max(CK * bA, 1) : CK * bA);
        if (needB) b0 = wm.row16_h<NARROW>(sB, g.ql, NARROW ? max(CK * bB, 1) : CK * bB);
        if (NARROW || (sA & 1)) { // (the middle rows start at column 1: column 0 by its formula)
            const int row = sA * RB;
            const int v = border(row, g.gopen, g.gext, g.indel) + row * g.gext + g.base;
            a0 = bA > 0 ? a0 : (unsigned)v;
        }
        if (NARROW || (sB & 1)) {
            const int row = sB * RB;
            const int v = border(row, g.gopen, g.gext, g.indel) + row * g.gext + g.base;
            b0 = bB > 0 ? b0 : (unsigned)v << 16;
        }
        hd = lo_hi(a0, b0);
    }
    const int qmax = ((g.ql + 3) >> 2) - 1;
    if (!NARROW) {
#pragma unroll 1
        for (int gg = 0; gg < groups; ++gg) { // (groups of eight columns, up to the last one a waiting walk stands in: it only ever moves left and up)
            uint2 va[8], vb[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) va[u] = vb[u] = make_uint2(0u, 0u);
            if (needA) {
#pragma unroll
                for (int u = 0; u < 8; ++u) va[u] = wm.row16_n<NARROW>(sA, g.ql, min(CK * bA + 8 * gg + u + 1, g.ql)); // (past ql: the last column again -- flags never read)
            }
            if (needB) {
#pragma unroll
                for (int u = 0; u < 8; ++u) vb[u] = wm.row16_n<NARROW>(sB, g.ql, min(CK * bB + 8 * gg + u + 1, g.ql));
            }
            unsigned qa[2], qb[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                qa[u] = wm.qblock(min(bA * (CK / 4) + 2 * gg + u, qmax), 0);
                qb[u] = wm.qblock(min(bB * (CK / 4) + 2 * gg + u, qmax), 1);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                unsigned e = lo_hi(va[u].y, vb[u].y);
                uint4 *const out = wm.blk + (size_t)(8 * gg + u) * 64;
                if (CODES)
                    column<RB, false, false, CODES>(h, f, t, code_table((qa[u >> 2] >> (8 * (u & 3))) & 0xffu, c.bm, c.bx), hd, e, c, out, nullptr,
                                                    code_table((qb[u >> 2] >> (8 * (u & 3))) & 0xffu, c.bm, c.bx));
                else
                    column<RB, false, false, false>(h, f, t, __builtin_amdgcn_perm(qb[u >> 2], qa[u >> 2], 0x0c040c00u + 0x00010001u * (u & 3)), hd, e, c, out);
                hd = lo_hi(va[u].x, vb[u].x);
            }
        }
        return;
    }
    // NARROW
#pragma unroll 1
    for (int gg = 0; gg < groups; ++gg) {
        // the round's eight columns of the kept row: hx[u] = H of {pair A, pair B}, ex[u] = E
        unsigned hx[8], ex[8];
        unsigned qa[2], qb[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            qa[u] = wm.qblock(min(bA * (CK / 4) + 2 * gg + u, qmax), 0);
            qb[u] = wm.qblock(min(bB * (CK / 4) + 2 * gg + u, qmax), 1);
        }
        if (!WaveMem::tail_wide(g.ql)) {
            // every kept row has one format and a block's columns start a group: per pair two uint4 of H and two uint2 of difference
            // bytes, whatever the band's parity.  A group past the last repeats the last one (flags never read).
            uint4 ha[2], hb[2];
            uint2 da[2], db[2];
#pragma unroll
            for (int x = 0; x < 2; ++x) {
                ha[x] = hb[x] = make_uint4(0u, 0u, 0u, 0u);
                da[x] = db[x] = make_uint2(0u, 0u);
            }
            const int glast = (g.ql - 1) >> 2;
            // (the group's offset by a 24-BIT multiply -- a group index is below 2^14 here: as a 32-bit multiply-add the compiler took
            // v_mad_u64_u32, whose 64-bit addend was a register pair with an unused half, and where that half was the register of a
            // query dword still in flight the byte-compare form waited vmcnt(0) in front of pair B's loads: for pair A's as well)
            if (needA) {
                const unsigned row = wm.kept_row_off(sA, g.ql);
#pragma unroll
                for (int x = 0; x < 2; ++x) {
                    const unsigned grp = row + __umul24((unsigned)min(bA * (CK / 4) + 2 * gg + x, glast), 1536u);
                    ha[x] = WaveMem::at32<uint4>(wm.rows, grp + 16u * wm.lane);
                    da[x] = WaveMem::at32<uint2>(wm.rows, grp + 1024u + 8u * wm.lane);
                }
            }
            if (needB) {
                const unsigned row = wm.kept_row_off(sB, g.ql);
#pragma unroll
                for (int x = 0; x < 2; ++x) {
                    const unsigned grp = row + __umul24((unsigned)min(bB * (CK / 4) + 2 * gg + x, glast), 1536u);
                    hb[x] = WaveMem::at32<uint4>(wm.rows, grp + 16u * wm.lane);
                    db[x] = WaveMem::at32<uint2>(wm.rows, grp + 1024u + 8u * wm.lane);
                }
            }
#pragma unroll
            for (int x = 0; x < 2; ++x) {
                const unsigned a4[4] = {ha[x].x, ha[x].y, ha[x].z, ha[x].w}, b4[4] = {hb[x].x, hb[x].y, hb[x].z, hb[x].w};
                const unsigned ad[2] = {da[x].x, da[x].y}, bd[2] = {db[x].x, db[x].y};
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    hx[4 * x + u] = lo_hi(a4[u], b4[u]);
                    // pair A's byte of its own row's dword, pair B's of its own, ZERO-extended into the two halves
                    ex[4 * x + u] = pk_sub(hx[4 * x + u], __builtin_amdgcn_perm(bd[u >> 1], ad[u >> 1], (u & 1) ? 0x0c070c02u : 0x0c050c00u));
                }
            }
        } else { // a wave with a wide tail (ql = 1, 2, 5): column by column
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                uint2 va = make_uint2(0u, 0u), vb = make_uint2(0u, 0u);
                if (needA) va = wm.row16_n<true>(sA, g.ql, min(CK * bA + 8 * gg + u + 1, g.ql));
                if (needB) vb = wm.row16_n<true>(sB, g.ql, min(CK * bB + 8 * gg + u + 1, g.ql));
                hx[u] = lo_hi(va.x, vb.x);
                ex[u] = lo_hi(va.y, vb.y);
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            unsigned e = ex[u];
            uint4 *const out = wm.blk + (size_t)(8 * gg + u) * 64;
            if (CODES)
                column<RB, false, false, CODES>(h, f, t, code_table((qa[u >> 2] >> (8 * (u & 3))) & 0xffu, c.bm, c.bx), hd, e, c, out, nullptr,
                                                code_table((qb[u >> 2] >> (8 * (u & 3))) & 0xffu, c.bm, c.bx));
            else
                column<RB, false, false, false>(h, f, t, __builtin_amdgcn_perm(qb[u >> 2], qa[u >> 2], 0x0c040c00u + 0x00010001u * (u & 3)), hd, e, c, out);
            hd = hx[u];
        }
    }
}

// ---- staging.  Eight 4-base blocks of both pairs per round: all loads of a round in flight, then the stores (one block per round
// exposes a memory latency per block: a tenth of the wave's lifetime, measured).  dst: the wave's [block][A | B][lane] dwords + lane.
// ASCII sequences (sw.cpp:55 compares raw bytes).  CODES: store base codes -- a target as the code per byte, a QUERY as 8 x code, or 32
// for a byte that is not one of ACGT (sw_lane_cell.h) -- and return nonzero if a byte of the first `len` is not one of ACGT.
typedef uint32_t dwords4 __attribute__((ext_vector_type(4), aligned(4))); // four consecutive dwords at a dword-aligned address
// dwords k0 .. k0 + 3 of a sequence: one 16-byte load where all four hold bytes of it, else dword by dword, clamped (SeqWords::word)
__device__ __forceinline__ void seq_words4(const SeqWords &s, const int k0, unsigned (&w)[4])
{
    if (k0 + 3 <= s.kmax) {
        const dwords4 v = *reinterpret_cast<const dwords4 *>(s.base + k0);
        w[0] = v.x;
        w[1] = v.y;
        w[2] = v.z;
        w[3] = v.w;
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) w[u] = s.word(k0 + u);
    }
}
template <bool CODES, bool QUERY>
__device__ __forceinline__ unsigned stage_ascii(const uint8_t *seqA, const uint8_t *seqB, const int len, const int nblocks, unsigned *dst)
{
    SeqWords sa, sb;
    sa.init(seqA, len);
    sb.init(seqB, len);
    unsigned bad = 0;
    for (int cb = 0; cb < nblocks; cb += 16) { // sixteen blocks of both pairs per round: 17 dwords of each sequence, in 16-byte loads
        unsigned wa[20], wb[20];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            unsigned xa[4], xb[4];
            seq_words4(sa, cb + 4 * u, xa);
            seq_words4(sb, cb + 4 * u, xb);
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                wa[4 * u + x] = xa[x];
                wb[4 * u + x] = xb[x];
            }
        }
        wa[16] = sa.word(cb + 16);
        wb[16] = sb.word(cb + 16);
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            if (cb + u < nblocks) { // (blocks past the end of a target repeat its last dword: rows > tl, never read)
                unsigned va = __builtin_amdgcn_alignbyte(wa[u + 1], wa[u], sa.shift), vb = __builtin_amdgcn_alignbyte(wb[u + 1], wb[u], sb.shift);
                if (CODES) {
                    unsigned da, db;
                    va = ascii_codes(va, da);
                    vb = ascii_codes(vb, db);
                    if (QUERY) {
                        const unsigned na = nonzero_bytes(da), nb = nonzero_bytes(db); // 0x80 in the bytes that are no ACGT: those become 32
                        va = ((va << 3) & ~((na >> 2) - (na >> 7))) | (na >> 2);
                        vb = ((vb << 3) & ~((nb >> 2) - (nb >> 7))) | (nb >> 2);
                    } else {
                        const int nv = len - 4 * (cb + u); // bytes of this block that belong to the sequence
                        const unsigned keep = nv >= 4 ? 0xffffffffu : nv <= 0 ? 0u : (1u << (8 * nv)) - 1u;
                        bad |= (da | db) & keep;
                    }
                }
                dst[(size_t)(2 * (cb + u)) * 64] = va;
                dst[(size_t)(2 * (cb + u) + 1) * 64] = vb;
            }
        }
    }
    return bad;
}

// 2-bit packed sequences (SeqSet::packed2: base k of the array in bits 2 (k & 3) of byte k >> 2; a pair's bases start at BASE index
// `start`, any alignment): read as aligned dwords of 16 bases, clamped to the last dword that holds a base of the sequence.
struct Seq2Words {
    const uint32_t *base;
    unsigned shift; // bits
    int kmax;
    __device__ __forceinline__ void init(const uint8_t *data, int64_t start, int len)
    {
        const uintptr_t a = reinterpret_cast<uintptr_t>(data) + (uintptr_t)(start >> 2), e = reinterpret_cast<uintptr_t>(data) + (uintptr_t)((start + len - 1) >> 2);
        base = reinterpret_cast<const uint32_t *>(a & ~(uintptr_t)3);
        shift = (unsigned)(a & 3) * 8u + 2u * (unsigned)(start & 3);
        kmax = (int)(((e & ~(uintptr_t)3) - (a & ~(uintptr_t)3)) >> 2);
    }
    __device__ __forceinline__ unsigned word(int k) const { return base[k < kmax ? k : kmax]; }
};
template <bool QUERY>
__device__ __forceinline__ void stage_2bit(const uint8_t *data, const int64_t startA, const int64_t startB, const int len, const int nblocks, unsigned *dst)
{
    Seq2Words sa, sb;
    sa.init(data, startA, len);
    sb.init(data, startB, len);
    for (int cb = 0; cb < nblocks; cb += 16) { // four dwords of 16 bases = sixteen blocks of both pairs per round
        unsigned wa[5], wb[5];
#pragma unroll
        for (int u = 0; u < 5; ++u) {
            wa[u] = sa.word((cb >> 2) + u);
            wb[u] = sb.word((cb >> 2) + u);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const unsigned va = __builtin_amdgcn_alignbit(wa[u + 1], wa[u], sa.shift), vb = __builtin_amdgcn_alignbit(wb[u + 1], wb[u], sb.shift);
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                const int blk = cb + 4 * u + x;
                if (blk < nblocks) {
                    const unsigned ca = spread_2bit((va >> (8 * x)) & 0xffu), cb2 = spread_2bit((vb >> (8 * x)) & 0xffu);
                    dst[(size_t)(2 * blk) * 64] = QUERY ? ca << 3 : ca;
                    dst[(size_t)(2 * blk + 1) * 64] = QUERY ? cb2 << 3 : cb2;
                }
            }
        }
    }
}

// One TILE = 128 pairs of the launch (pairs 128 gw .. 128 gw + 127), worked on by the wave that sits in wave slot `slot` of the
// persistent grid: everything the wave keeps while it works -- WaveMem, the staged sequences -- lives in the slot's region, which
// the wave reuses tile after tile (a lane only ever reads back what it has written for the tile it is working on).
// whole lines out of LDS: `bytes` (a multiple of 4) from src (LDS, 16-byte aligned) to dst (global, 16-byte aligned)
__device__ __forceinline__ void lds_to_global(void *dst, const unsigned char *src, const int bytes, const int lane)
{
    const int whole = bytes & ~15;
    for (int k = lane * 16; k < whole; k += 1024) *reinterpret_cast<uint4 *>(static_cast<unsigned char *>(dst) + k) = *reinterpret_cast<const uint4 *>(src + k);
    for (int k = whole + lane * 4; k < bytes; k += 256) *reinterpret_cast<unsigned *>(static_cast<unsigned char *>(dst) + k) = *reinterpret_cast<const unsigned *>(src + k);
}

// VIA_LDS (= walk_in.coalesced_out, a template parameter so that every pointer the walks write through has ONE address space: with the
// choice made at run time the text went out through flat instructions, whose waits also cover the scalar loads -- pass 2 took twice as long)
// (A wave keeps its slot for all its tiles, so every address of its region is invariant in the kernel's tile loop: the compiler computes
// them once in front of it and keeps some forty of them in scratch for the kernel's whole life -- a load each where a tile needs one,
// none inside pass 1's loops.  Making slot and lane opaque per tile recomputes them instead and empties the scratch area by a third,
// but the kernel ran 2.5 ms per 10 M pairs SLOWER (65.2 against 62.6: the opaque lane number hides its range from the address
// arithmetic of every store of pass 1) -- measured, scripts/ck_regs_probe.sh, and left alone.)
template <bool VIA_LDS, bool FOLD, bool NARROW>
__device__ __forceinline__ void sw_dp16_lane_ck_tile(const DpArgs &a, const TbArgs &walk_in, const int64_t gw, const int64_t slot, const int lane, unsigned char *out_lds, const bool first)
{
    const int64_t n_ls = (a.count + 1) >> 1;
#ifdef MGL_CK_PHASES
    unsigned long long phase_t0 = __builtin_amdgcn_s_memtime();
#endif
    const int64_t ls = gw * 64 + lane;
    const bool lvalid = ls < n_ls;
    const int64_t slotA = lvalid ? 2 * ls : a.count - 1;
    const bool validB = lvalid && (2 * ls + 1 < a.count);
    const int64_t slotB = validB ? 2 * ls + 1 : slotA;

    // one geometry per launch (a.uni_tl x a.uni_ql), or -- a.grouped: a chunk sorted by geometry, whole waves of 128 pairs --
    // one per wave, read from its first pair; a.uni_tl / a.uni_ql are then the maxima that size the wave's regions
    const bool grouped = a.grouped != 0;
    const int tl = grouped ? __builtin_amdgcn_readfirstlane(a.t.length(a.first + gw * 128)) : a.uni_tl;
    const int ql = grouped ? __builtin_amdgcn_readfirstlane(a.q.length(a.first + gw * 128)) : a.uni_ql;
    const int match = a.match, gopen = a.gopen, gext = a.gext;
    const bool indel = (a.strategy & (OS_INDEL | OS_LEAD_ID)) != 0;
    const int base = dp16_base(tl, ql, match, gext);
    LaneConsts c;
    c.delta = pack2(a.mismatch - match, a.mismatch - match);
    c.one = pack2(1, 1);
    c.o_e = pack2(gopen - gext, gopen - gext);
    c.k2 = pack2(match + 2 * gext, match + 2 * gext);
    asm volatile("" : "+v"(c.delta), "+v"(c.one), "+v"(c.o_e), "+v"(c.k2));
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        c.k12[u] = 0x02020202u << (2 * u);
        c.k34[u] = 0x01010101u << (2 * u);
        asm volatile("" : "+s"(c.k12[u]), "+s"(c.k34[u]));
    }
    c.kf = pack2(a.fold_k, a.fold_k);
    c.bm = FOLD ? (unsigned)a.fold_bm : 0u;
    c.bx = FOLD ? (unsigned)a.fold_bx : 1u;
    if (FOLD) asm volatile("" : "+s"(c.kf)); // (the bytes only build the tables: left to the compiler, four registers fewer spilled)
    constexpr int CM = FOLD ? CMP_FOLD : CMP_CODES; // (waves whose targets are not all ACGT take the byte compare either way)

    const int strips = lane_strips(tl, R), nb = lane_ck_blocks(ql);
    // the wave's scratch: both queries and both targets of every lane transposed to [4-base block][A | B][lane] dwords
    unsigned *const qst = reinterpret_cast<unsigned *>(a.scratch + (size_t)slot * (size_t)lane_ck_scratch_bytes(a.uni_tl, a.uni_ql)) + lane;
    unsigned *const tst = qst + (size_t)((ql + 3) >> 2) * 128;
    WaveMem wm;
    {
        uint2 *const region = reinterpret_cast<uint2 *>(a.tb + (size_t)slot * (size_t)a.tb_stride_words);
        wm.bnd = region + lane;
        wm.mid = wm.bnd + (size_t)(strips + 1) * (ql + 1) * 64;
        wm.ck = reinterpret_cast<unsigned *>(region + ((size_t)(strips + 1) * (ql + 1) + (size_t)strips * ql) * 64) + lane;
        wm.blk = reinterpret_cast<uint4 *>(reinterpret_cast<unsigned *>(region) + ((size_t)(strips + 1) * (ql + 1) * 2 + (size_t)strips * ql * 2 + (size_t)strips * (nb - 1) * 64) * 64) + lane;
        wm.rows = region;
        wm.mid_off = (unsigned)((strips + 1) * (ql + 1) * 64);
        wm.cku = reinterpret_cast<const unsigned *>(region + ((size_t)(strips + 1) * (ql + 1) + (size_t)strips * ql) * 64);
        wm.blku = reinterpret_cast<const uint32_t *>(region) + ((size_t)(strips + 1) * (ql + 1) * 2 + (size_t)strips * ql * 2 + (size_t)strips * (nb - 1) * 64) * 64;
        wm.seq = reinterpret_cast<const unsigned *>(a.scratch + (size_t)slot * (size_t)lane_ck_scratch_bytes(a.uni_tl, a.uni_ql));
        wm.t_off = (unsigned)(((ql + 3) >> 2) * 128);
        wm.lane = (unsigned)lane;
    }
    // ---- staging: both sequences of every lane, transposed to [4-base block][A | B][lane] dwords in the wave's scratch -- as BASE
    // CODES where the wave's targets allow it (sw_lane_cell.h: 2-bit packed inputs always do; ASCII targets when every byte is one of
    // ACGT -- the queries may hold anything), else as the raw bytes.
    bool codes;
    {
        const int64_t pA = a.first + slotA, pB = a.first + slotB;
        const int qblocks = (ql + 3) >> 2, tblocks = strips * (R / 4);
        if (a.t.packed2) {
            stage_2bit<false>(a.t.data, a.t.off[pA], a.t.off[pB], tl, tblocks, tst);
            stage_2bit<true>(a.q.data, a.q.off[pA], a.q.off[pB], ql, qblocks, qst);
            codes = true;
        } else {
            const unsigned bad = stage_ascii<true, false>(a.t.data + a.t.off[pA], a.t.data + a.t.off[pB], tl, tblocks, tst);
            codes = __builtin_amdgcn_ballot_w64(bad != 0u) == 0;
            if (codes) {
                stage_ascii<true, true>(a.q.data + a.q.off[pA], a.q.data + a.q.off[pB], ql, qblocks, qst);
            } else { // a target byte outside ACGT somewhere in the wave: raw bytes for all of it
                stage_ascii<false, false>(a.t.data + a.t.off[pA], a.t.data + a.t.off[pB], tl, tblocks, tst);
                stage_ascii<false, true>(a.q.data + a.q.off[pA], a.q.data + a.q.off[pB], ql, qblocks, qst);
            }
        }
        // The borders depend on the launch's geometry and parameters alone and nothing overwrites them (the strips write columns
        // 1 .. ql of the rows they leave), so a wave of a launch with ONE geometry writes them in front of its first tile only
        // (`first`) -- once per LAUNCH: the next launch on this region may have another geometry, strategy or gap cost.  A grouped
        // launch's geometry changes from tile to tile.
        if (NARROW && (grouped || first)) {
            // row 0 (the border row, sw.cpp:14-18,31-35) in the kept rows' one format (WaveMem): H[0][j] of a group's four columns, and
            // E[1][j] = H[0][j] - o as the byte o - e of every column.  Column 0 of no kept row is stored.
            char *rg = reinterpret_cast<char *>(const_cast<uint2 *>(wm.rows));
            const int groups = (ql + 3) >> 2;
            const unsigned bytes = (unsigned)(gopen - gext) * 0x01010101u;
            for (int gi = 0; gi < groups; ++gi, rg += 1536) {
                unsigned hp[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) { // (columns past ql: the formula goes on, nobody reads them)
                    const int j = 4 * gi + 1 + u, hb0 = border(j, gopen, gext, indel) + j * gext + base;
                    hp[u] = pack2(hb0, hb0);
                }
                if (WaveMem::tail_wide(ql) && gi == groups - 1) { // a last group of one or two columns: wide records
                    *reinterpret_cast<uint2 *>(rg + 8u * (unsigned)lane) = make_uint2(hp[0], pk_sub(hp[0], c.o_e));
                    if (4 * gi + 2 <= ql) *reinterpret_cast<uint2 *>(rg + 512 + 8u * (unsigned)lane) = make_uint2(hp[1], pk_sub(hp[1], c.o_e));
                } else {
                    *reinterpret_cast<uint4 *>(rg + 16u * (unsigned)lane) = make_uint4(hp[0], hp[1], hp[2], hp[3]);
                    *reinterpret_cast<uint2 *>(rg + 1024 + 8u * (unsigned)lane) = make_uint2(bytes, bytes);
                }
            }
        }
        if (!NARROW && (grouped || first)) {
            // row 0 (the border row, sw.cpp:14-18,31-35) in stored form: H[0][j], E[1][j] = H[0][j] - o
            for (int j = 0; j <= ql; ++j) {
                const int hb0 = border(j, gopen, gext, indel) + j * gext + base;
                const unsigned hp = pack2(hb0, hb0);
                wm.bnd[(size_t)j * 64] = make_uint2(hp, pk_sub(hp, c.o_e));
            }
            // column 0 of the rows entering the other strips: H[32 k][0] (what a strip's first diagonal starts from)
            for (int k = 1; k <= strips; ++k) {
                const int hb0 = border(k * R, gopen, gext, indel) + k * R * gext + base;
                wm.bnd[(size_t)k * (ql + 1) * 64] = make_uint2(pack2(hb0, hb0), 0u);
            }
        }
    }

    CK_PHASE(0); // staging
    // ---- pass 1
    int bestA = NEG_INF, bestA_i = -1, bestB = NEG_INF, bestB_i = -1;
    int keyA = INT32_MIN, keyB = INT32_MIN; // the last row's running best (row_pref above): every column's key is >= this
    unsigned corner = 0u;                   // H[tl][ql], stored form
    // (the narrow kernels hold no stored-row strip: with the group's registers its column loop reloaded a spilled pointer in every round,
    // and launch_dp16_lane_ck sends them no query that long)
    const bool row_stored = !NARROW && ql > ROW_KEY_MAX_QL;
#define CK_STRIPS(CMP)                                                                                                                      \
    do {                                                                                                                                    \
        for (int k = 0; k < strips - 1; ++k)                                                                                                \
            ck_strip<NOT_LAST, CMP, NARROW>(k, tl, ql, nb, wm, qst, tst, c, gopen, gext, base, indel, bestA, bestA_i, bestB, bestB_i, keyA, keyB, corner); \
        if (row_stored)                                                                                                                     \
            ck_strip<LAST_ROW_STORED, CMP, NARROW>(strips - 1, tl, ql, nb, wm, qst, tst, c, gopen, gext, base, indel, bestA, bestA_i, bestB, bestB_i, keyA, keyB, corner); \
        else                                                                                                                                \
            ck_strip<LAST_ROW_KEYS, CMP, NARROW>(strips - 1, tl, ql, nb, wm, qst, tst, c, gopen, gext, base, indel, bestA, bestA_i, bestB, bestB_i, keyA, keyB, corner); \
    } while (0)
    if (codes)
        CK_STRIPS(CM);
    else
        CK_STRIPS(CMP_BYTES);
#undef CK_STRIPS

    CK_PHASE(1); // pass 1
    // ---- last row (sw.cpp:116-127): the winner of each half out of its key
    int rmA, rdA, rjA, rmB, rdB, rjB;
    const int frame = (tl + ql) * gext + base; // w - frame = the score
    const int cornerA = lo16(corner) - frame, cornerB = hi16(corner) - frame;
    if (!row_stored) {
        rjA = row_col(tl, ql, keyA & 0xffff);
        rjB = row_col(tl, ql, keyB & 0xffff);
        rmA = (keyA >> 16) - frame;
        rmB = (keyB >> 16) - frame;
        rdA = abs(tl - rjA);
        rdB = abs(tl - rjB);
    } else { // the last strip left H[tl][j] in the row "entering strip `strips`"
        rmA = rmB = NEG_INF;
        rdA = rjA = rdB = rjB = 0x7fffffff;
        const uint2 *const last = wm.bnd + (size_t)strips * (ql + 1) * 64;
        for (int j0 = 1; j0 <= ql; j0 += 8) { // eight columns' loads at once
            unsigned bots[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) bots[u] = last[(size_t)min(j0 + u, ql) * 64].x;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int j = j0 + u;
                if (j <= ql) {
                    const unsigned bot = bots[u];
                    const int unshift = -(tl + j) * gext - base;
                    const int d = abs(tl - j);
                    const int sa = lo16(bot) + unshift, sb = hi16(bot) + unshift;
                    const bool ta_ = sa > rmA || (sa == rmA && d < rdA);
                    rmA = ta_ ? sa : rmA;
                    rdA = ta_ ? d : rdA;
                    rjA = ta_ ? j : rjA;
                    const bool tb_ = sb > rmB || (sb == rmB && d < rdB);
                    rmB = tb_ ? sb : rmB;
                    rdB = tb_ ? d : rdB;
                    rjB = tb_ ? j : rjB;
                }
            }
        }
    }
    DpRecord rec[2];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int mqe = half ? bestB : bestA, mqe_t = half ? bestB_i : bestA_i;
        const int rm = half ? rmB : rmA, rd = half ? rdB : rdA, rj = half ? rjB : rjA;
        const bool row_wins = rm > mqe || (rm == mqe && rd < abs(mqe_t - ql));
        DpRecord &r = rec[half];
        r.mqe = mqe;
        r.mqe_t = mqe_t;
        r.max = row_wins ? rm : mqe;
        r.max_t = row_wins ? tl : mqe_t;
        r.max_q = row_wins ? rj : ql;
        r.seg = row_wins ? ql - rj : 0;
        r.g_tail = 0;
        r.sps = R;
        if (half ? validB : lvalid) a.rec[half ? slotB : slotA] = r;
    }

    CK_PHASE(2); // records
    // ---- pass 2
    const int64_t pA = a.first + slotA, pB = a.first + slotB;
    // where the walks write: the caller's arrays, or (walk_in.coalesced_out) this tile's 128 slots of each in LDS -- cigar [128][stride] |
    // ScoreMax [128] | offset [128] | length [128] | status [128] -- which leave as whole lines below
    constexpr bool via_lds = VIA_LDS;
    TbArgs walk = walk_in;
    unsigned char *const l_score = out_lds + 128 * LANE_CK_OUT_STRIDE_MAX, *const l_off = l_score + 128 * 24, *const l_len = l_off + 512, *const l_status = l_len + 512;
    if (via_lds) {
        walk.cigar = reinterpret_cast<char *>(out_lds);
        walk.score = walk_in.score ? reinterpret_cast<Score *>(l_score) : nullptr;
        walk.offset = reinterpret_cast<int32_t *>(l_off);
        walk.cigar_len = walk_in.cigar_len ? reinterpret_cast<int32_t *>(l_len) : nullptr;
        walk.status = walk_in.status ? reinterpret_cast<int32_t *>(l_status) : nullptr;
    }
    const int64_t oA = via_lds ? 2 * lane : walk.dest ? walk.dest[pA] : pA, oB = via_lds ? 2 * lane + 1 : walk.dest ? walk.dest[pB] : pB;
    PathWalk wa, wb;
    wa.start(walk, rec[0], oA, tl, ql, lvalid, cornerA);
    wb.start(walk, rec[1], oB, tl, ql, validB, cornerB);
    // Where the walks take the bases they compare.  ASCII input: from the caller's own arrays, in 16-byte loads (SeqBlocks) -- raw
    // bytes, which is what the reference compares, whatever form the wave staged.  2-bit input (and a.walk_staged): from the staged
    // dwords.  One value per launch, wave-uniform, fixed here in front of the loops; both forms are plain global loads.
    const bool direct = !a.t.packed2 && !a.walk_staged;
    if (direct) { // (an invalid half walks nothing: it holds the lane's pair A, or the launch's last pair)
        wa.ts.init(a.t.data + a.t.off[pA]);
        wa.qs.init(a.q.data + a.q.off[pA]);
        wb.ts.init(a.t.data + a.t.off[pB]);
        wb.qs.init(a.q.data + a.q.off[pB]);
    }
    BlockGeom geom_launch;
    BlockGeom &geom = geom_launch;
    geom.tl = tl;
    geom.ql = ql;
    geom.nb = nb;
    geom.match = match;
    geom.mismatch = a.mismatch;
    geom.gopen = gopen;
    geom.gext = gext;
    geom.base = base;
    geom.indel = indel;
    geom.codes = codes;
    geom.direct = false;
    const bool by_score = !(MGL_CK_ABLATE & 8);
    const int tblocks = strips * (R / 4), qblocks = (ql + 3) >> 2;
    // The two loops of pass 2 that read windows, once per form: in either copy the form is a constant, so it holds the loads, the
    // registers and the compare of its own form only (both forms behind a run-time branch at every load: 80 scratch accesses in the
    // verify loop).  The block's recomputation between them reads the staged codes and exists once.
    auto stretches = [&](auto direct_form) __attribute__((always_inline)) {
        BlockGeom geom = geom_launch;
        geom.direct = decltype(direct_form)::value;
        geom.codes = !decltype(direct_form)::value && codes;
        for (;;) { // every walk standing at a cell takes the diagonal stretches whose scores add up (PathWalk::verify_apply)
            unsigned ta[17], qa[17], tb[17], qb[17], ga[PathWalk::VB], gb[PathWalk::VB];
            WinShift sa = {0u, 0u}, sb = {0u, 0u};
            if (wa.can_verify()) {
                sa = wa.win64_load(wm, 0, tblocks, qblocks, geom, ta, qa);
                wa.template grid_load<NARROW>(wm, ql, ga);
            }
            if (wb.can_verify()) {
                sb = wb.win64_load(wm, 1, tblocks, qblocks, geom, tb, qb);
                wb.template grid_load<NARROW>(wm, ql, gb);
            }
            const bool ma = wa.verify_apply(ta, qa, sa, ga, 0, geom), mb = wb.verify_apply(tb, qb, sb, gb, 1, geom);
#ifdef MGL_CK_PHASES
            if (lane == 0) atomicAdd(&mgl_ck_phase_ticks[12], 1ull);
#endif
            if (!__builtin_amdgcn_ballot_w64(ma || mb)) break;
        }
        // every walk that is stuck where it stands now: the stretch to its block's left edge, where that comes before the kept
        // row (PathWalk::edge_len) -- one more dword and 16 bases of both sequences per walk, one memory latency per block round
        {
            const int ea = wa.edge_len(), eb = wb.edge_len();
            if (__builtin_amdgcn_ballot_w64((ea | eb) != 0)) {
                unsigned ta[5], qa[5], tb[5], qb[5], ha = 0u, hb = 0u;
                WinShift sa = {0u, 0u}, sb = {0u, 0u};
                if (ea) {
                    sa = wa.win_load(wm, 0, tblocks, qblocks, geom, ta, qa);
                    ha = wa.template edge_load<NARROW>(wm, nb, ea);
                }
                if (eb) {
                    sb = wb.win_load(wm, 1, tblocks, qblocks, geom, tb, qb);
                    hb = wb.template edge_load<NARROW>(wm, nb, eb);
                }
                const bool xa = wa.edge_apply(ha, ta, qa, sa, ea, 0, geom), xb = wb.edge_apply(hb, tb, qb, sb, eb, 1, geom);
#ifdef MGL_CK_PHASES
                const unsigned long long took_ = __popcll(__builtin_amdgcn_ballot_w64(xa)) + __popcll(__builtin_amdgcn_ballot_w64(xb));
                const unsigned long long tried_ = __popcll(__builtin_amdgcn_ballot_w64(ea != 0)) + __popcll(__builtin_amdgcn_ballot_w64(eb != 0));
                if (lane == 0) {
                    atomicAdd(&mgl_ck_phase_ticks[10], took_);
                    atomicAdd(&mgl_ck_phase_ticks[11], tried_ - took_);
                }
#else
                (void)xa;
                (void)xb;
#endif
            }
        }
    };
    auto block_walk = [&](auto direct_form, const int kA, const int bA, const int kB, const int bB) __attribute__((always_inline)) {
        BlockGeom geom = geom_launch;
        geom.direct = decltype(direct_form)::value;
        geom.codes = !decltype(direct_form)::value && codes;
        for (;;) {
            const bool la = wa.can_load(kA, bA), lb = wb.can_load(kB, bB);
            // (a lane with nothing to fetch still runs apply(): a run that ends at the matrix's edge needs no flags)
            unsigned fa[PathWalk::LOOK], fb[PathWalk::LOOK], ta[5], qa[5], tb[5], qb[5];
            WinShift sa = {0u, 0u}, sb = {0u, 0u};
            if (la) {
                wa.load(wm, fa);
                if (wa.mode == 0) sa = wa.win_load(wm, 0, tblocks, qblocks, geom, ta, qa);
            }
            if (lb) {
                wb.load(wm, fb);
                if (wb.mode == 0) sb = wb.win_load(wm, 1, tblocks, qblocks, geom, tb, qb);
            }
            const bool ga = wa.apply(fa, ta, qa, sa, 0, kA, bA, geom), gb = wb.apply(fb, tb, qb, sb, 1, kB, bB, geom);
            if (!__builtin_amdgcn_ballot_w64(ga || gb)) break;
        }
    };
    while (!(MGL_CK_ABLATE & 1) && __builtin_amdgcn_ballot_w64(!wa.done || !wb.done) != 0) {
        if (by_score) {
            if (direct)
                stretches(std::true_type{});
            else
                stretches(std::false_type{});
            CK_PHASE(3); // stretches that add up
            if (__builtin_amdgcn_ballot_w64(!wa.done || !wb.done) == 0) break;
        }
        // (a finished walk's half recomputes some valid block's worth of garbage: both halves run the same instructions anyway)
        const int kA = max(wa.pi - 1, 0) >> 4, bA = max(wa.pj - 1, 0) / CK, kB = max(wb.pi - 1, 0) >> 4, bB = max(wb.pj - 1, 0) / CK;
        // the columns of its block a walk can still reach end at the one it stands in: the wave recomputes up to the farthest such column
        int reach = max(!wa.done ? (max(wa.pj - 1, 0) % CK) + 1 : 0, !wb.done ? (max(wb.pj - 1, 0) % CK) + 1 : 0);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) reach = max(reach, __shfl_xor(reach, m));
        const int groups = __builtin_amdgcn_readfirstlane((reach + 7) >> 3); // (61.80 ms per 10 M pairs against 61.98 with every block in full)
        if (codes)
            ck_block<CM, NARROW>(kA, bA, kB, bB, !wa.done, !wb.done, geom, wm, c, groups);
        else
            ck_block<CMP_BYTES, NARROW>(kA, bA, kB, bB, !wa.done, !wb.done, geom, wm, c, groups);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the block's flags are in memory
        CK_PHASE(4); // a block's flags
#ifdef MGL_CK_PHASES
        if (lane == 0) atomicAdd(&mgl_ck_phase_ticks[8], 1ull);
#endif
        if (direct)
            block_walk(std::true_type{}, kA, bA, kB, bB);
        else
            block_walk(std::false_type{}, kA, bA, kB, bB);
        wa.stuck = wb.stuck = false; // either walk has moved on
        CK_PHASE(5); // the walk inside the block
    }
    CK_PHASE(6);
    if (lvalid) wa.finish(walk, a.rec + slotA, oA);
    if (validB) wb.finish(walk, a.rec + slotB, oB);
    if (via_lds) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        const int64_t p0 = a.first + gw * 128;
        const int np = (int)min((int64_t)128, a.count - gw * 128); // pairs of this tile
        lds_to_global(walk_in.cigar + (size_t)p0 * walk_in.cigar_stride, out_lds, np * walk_in.cigar_stride, lane);
        if (walk_in.score) lds_to_global(walk_in.score + p0, l_score, np * 24, lane);
        lds_to_global(walk_in.offset + p0, l_off, np * 4, lane);
        if (walk_in.cigar_len) lds_to_global(walk_in.cigar_len + p0, l_len, np * 4, lane);
        if (walk_in.status) lds_to_global(walk_in.status + p0, l_status, np * 4, lane);
        __builtin_amdgcn_wave_barrier(); // (the next tile's walks write the same LDS)
    }
    CK_PHASE(7); // overhangs, text, results
#ifdef MGL_CK_PHASES
    if (lane == 0) atomicAdd(&mgl_ck_phase_ticks[9], 1ull);
#endif
}

} // namespace

// A PERSISTENT grid: a.lane_slots waves (at most what the chip holds at two waves per SIMD -- 256 registers: no spills in pass 1's
// loops), each with one region of the workspace, each taking tile after tile: its first one by its slot number, the following ones
// off a counter in device memory (a.tile_ctr[0]; zero when the launch starts) until the tiles are gone.  The workspace a launch needs is therefore
// lane_slots regions (2 MB each at 256 x 150: 4 GB for a whole MI355X) however many pairs it holds -- round 3 gave every TILE a region
// (15 KB per pair: 208 GiB for the bench's 10 M pairs in one launch, and chunks wherever the workspace was smaller).  Every wave
// reaches the loop's exit: the counter only grows, a tile's work is bounded, nothing waits for another wave.
// ONE wave per workgroup: the waves share nothing (no LDS, no barrier), and a workgroup's registers are released only when its LAST
// wave has ended (round 3, four per workgroup: three of four SIMD slots stood empty until the slowest was through).
// A three-wave-per-SIMD build of the same code (168 registers, spills) was slower everywhere in round 3 and is gone.
// HOW THE TWO WAVES OF A SIMD SHARE IT (traced, scripts/ck_trace.py, docs/history.md C.0): the arbiter serves the OLDER wave first -- one
// wave of every SIMD runs a tile in 1.2 ms, the other, on what the first leaves free, in 2.5 (a 10 M-pair launch: 1 024 slots with 50
// tiles each, 1 024 with 25); together 1.21 tiles per ms and SIMD, one wave alone 0.95.  The counter evens that out: whoever is through
// draws the next tile.  Rules that keep the slow waves from drawing a launch's last tiles were built and measured (the end of a
// 1.25 M-pair launch moved between 8.9 and 9.6 ms either way, box by box) and are gone.
// TWO kernels, one per way the results leave (VIA_LDS: in whole lines out of LDS, TbArgs::coalesced_out; else lane by lane through the
// caller's pointers): one kernel holding both tile functions had the registers of both to colour at once (192 spilled against 66).
template <bool VIA_LDS, bool FOLD, bool NARROW>
__device__ __forceinline__ void lane_ck_grid(const DpArgs &a, const TbArgs &walk, unsigned char *out_lds)
{
    const int lane = threadIdx.x & 63;
    const int64_t tiles = (((a.count + 1) >> 1) + 63) >> 6, slots = gridDim.x, slot = blockIdx.x;
    // in-kernel clock probe (profiling level 2; off in normal runs): shader-clock ticks and 100 MHz ticks of this wave's whole life
    unsigned long long diag_t0 = 0, diag_w0 = 0;
    if (a.diag) {
        diag_t0 = __builtin_amdgcn_s_memtime();
        diag_w0 = __builtin_amdgcn_s_memrealtime();
    }
    int64_t arrived = a.gate ? 0 : INT64_MAX; // pairs of the batch known to be in device memory
    unsigned long long *const ctr = reinterpret_cast<unsigned long long *>(a.tile_ctr); // {draws, waves out}: ONE object (below)
    for (int64_t tile = slot; tile < tiles;) {
        // The host entries run ONE launch over a batch whose inputs are still crossing the link: the copy engines bring them chunk by chunk
        // and the host moves a.gate on as each chunk has landed.  A wave whose tile is not there yet looks at the word (a read over the
        // link, so only then) and sleeps in between; the copies do not depend on anything this grid does, so the wait ends -- and if the
        // word stands still for gate_timeout_ticks the wave raises gate_failed and leaves, its tiles undone (the host sees the flag).
        // (a tile's aligned loads may touch the first line of the pair behind its last one: the NEXT tile's pairs must have arrived too, so
        // that no line of an input array enters a cache before its bytes are there.  Pass 2's walks read the caller's arrays as well
        // (SeqBlocks: whole 16-byte blocks that hold at least one byte of the walk's own pair): the block of a pair's last byte may hold
        // the first bytes of the pair behind it -- for the tile's last pair that is tile t + 1, which the wave has waited for --, and
        // the block of its first byte the last bytes of the pair in front of it -- for the tile's first pair that is tile t - 1,
        // whose pairs arrived before this tile's did: the chunks land in order.)
        if (arrived < a.first + min(a.count, (tile + 2) * 128)) {
            const int64_t need = a.first + min(a.count, (tile + 2) * 128);
            // ONE wave at a time looks at the host's word (round 5).  Packed inputs arrive eight times faster than the grid consumes them:
            // a wave seldom waits.  ASCII inputs do not -- the link is the bound, every wave of the grid stands at the gate most of the
            // time -- and 2 048 waves each reading a word over the link every few microseconds put a gigabyte per second of read
            // completions on the very direction the inputs travel in.  So the word has a mirror in DEVICE memory (a.gate_dev[0]) that the
            // waiting waves watch, and whoever finds the mirror older than a microsecond (a.gate_dev[1], 100 MHz ticks; a compare-and-swap
            // picks one wave) reads the host's word and moves the mirror on.  A negative word (the host calls the grid off) goes into the
            // mirror as it is.
            int lo = 0, hi = 0, flags = 0; // lane 0 waits, everybody else waits for lane 0: {seen.lo, seen.hi, 1 = gave up}
            if (lane == 0) {
                unsigned long long since = __builtin_amdgcn_s_memrealtime();
                long long last = arrived, seen;
                for (;;) {
                    seen = (long long)__hip_atomic_load(reinterpret_cast<const unsigned long long *>(a.gate_dev), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (seen >= need || seen < 0) break;
                    const unsigned long long now = __builtin_amdgcn_s_memrealtime();
                    const unsigned long long polled = __hip_atomic_load(reinterpret_cast<const unsigned long long *>(a.gate_dev) + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (now - polled >= 100ull) {
                        unsigned long long expect = polled;
                        if (__hip_atomic_compare_exchange_strong(reinterpret_cast<unsigned long long *>(a.gate_dev) + 1, &expect, now, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                            const long long v = (long long)__hip_atomic_load(reinterpret_cast<const unsigned long long *>(a.gate), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                            if (v < 0)
                                __hip_atomic_store(reinterpret_cast<long long *>(a.gate_dev), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            else
                                __hip_atomic_fetch_max(reinterpret_cast<long long *>(a.gate_dev), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            seen = v;
                            if (seen >= need || seen < 0) break;
                        }
                    }
                    if (seen != last) {
                        last = seen;
                        since = now;
                    } else if (now - since > (unsigned long long)a.gate_timeout_ticks) {
                        flags = 1;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(32);
                }
                lo = (int)(unsigned)(unsigned long long)seen;
                hi = (int)(unsigned)((unsigned long long)seen >> 32);
            }
            lo = __builtin_amdgcn_readfirstlane(lo);
            hi = __builtin_amdgcn_readfirstlane(hi);
            flags = __builtin_amdgcn_readfirstlane(flags);
            arrived = (int64_t)((unsigned long long)(unsigned)lo | (unsigned long long)(unsigned)hi << 32);
            if (flags & 1) { // the word stood still for gate_timeout_ticks: the host sees the flag and does the call again the chunked way
                if (lane == 0) __hip_atomic_store(a.gate_failed, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                break;
            }
            if (arrived < 0) break; // the host calls the grid off (an index array failed its check, a copy failed): leave, nothing is wrong with the device
            // An acquire fence between the look that let the wave through and the loads of the pairs it announced: once per WAIT (a wave
            // waits a handful of times while the inputs cross the link, never once they are there), so it costs nothing that can be
            // measured -- and without it the order of those loads behind a relaxed load rested on a branch and on the argument that no
            // cache holds a line of pairs that have just arrived (the margin above; the grid starts with empty caches).  That argument
            // still holds; the fence is what makes the order the language's, not the hardware's.  (-DMGL_CK_NO_GATE_FENCE: round 4's form.)
#ifndef MGL_CK_NO_GATE_FENCE
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#endif
        }
#ifdef MGL_CK_TRACE
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
#endif
        sw_dp16_lane_ck_tile<VIA_LDS, FOLD, NARROW>(a, walk, tile, slot, lane, out_lds, tile == slot); // (later tiles: slots + a draw)
#ifdef MGL_CK_TRACE
        if (lane == 0 && tile < (1 << 17)) {
            unsigned hw;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
            unsigned xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            mgl_ck_trace[4 * tile + 0] = (unsigned long long)slot;
            mgl_ck_trace[4 * tile + 1] = (unsigned long long)hw | (unsigned long long)(xcc & 15u) << 32;
            mgl_ck_trace[4 * tile + 2] = t0;
            mgl_ck_trace[4 * tile + 3] = __builtin_amdgcn_s_memrealtime();
        }
#endif
        if (tiles <= slots) break; // (every tile has its wave: the counter is not even touched)
        unsigned next = 0;
        if (lane == 0) {
            next = (unsigned)__hip_atomic_fetch_add(ctr, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // The waves of one launch draw `tiles` times at most (tiles - slots draws that find a tile, one per wave that does not), so a
            // larger number means the word did not stand at zero when the launch started: somebody else's launch is on it, or memory is
            // not what it was.  The host finds the flag at its next look (mgl_sw_ctx_check, every later call): MGL_SW_ERR_DEVICE, never
            // a silent tile left undone.
            if (next >= (unsigned)tiles && a.grid_fault) __hip_atomic_store(a.grid_fault, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        tile = slots + (int64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)next);
    }
    // THE LAST WAVE OUT ZEROES THE COUNTER (round 5).  Every wave of the grid comes through here -- after its last draw, or from the gate
    // when the host has called the launch off or the gate stood still -- and counts itself out in the word's HIGH half; the one that
    // finds slots - 1 there knows that nobody will draw again and puts the word back to zero.  So a launch finds its counter at zero
    // however the launch before it on that word ended.  (Round 4 never reset the word and kept a host-side copy of where it stood, "moved
    // on by exactly `tiles` per launch" -- which a launch called off at its gate did not do: the copy and the word parted, and 64 launches
    // later the grid that came round to that word left its tiles undone with status 0.)
    // Draws (low half) and waves out (high half) are ONE 64-bit atomic object on purpose: a wave's draws come before its count-out in
    // that object's modification order (same thread, same object), the last count-out reads the value every other count-out has left,
    // and the store of zero follows it -- all with RELAXED operations.  As two words the same chain needed an acquire-release on every
    // wave's way out, which on this chip is a write-back and an invalidate of the XCD's L2 (buffer_wbl2 / buffer_inv, 2 048 of them
    // while the last tiles are still writing their rows): against round 4's library on one box, launches of 2 M pairs were
    // 1.3-1.6 % behind it in that form and are 0.7 % behind it in this one (profiles/r05_ab_r04_vs_head.txt; 10 M pairs: level).
    if (tiles > slots && lane == 0) {
        const unsigned out = (unsigned)(__hip_atomic_fetch_add(ctr, 1ull << 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 32);
        if (out == (unsigned)slots - 1u) {
            __hip_atomic_store(ctr, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else if (out >= (unsigned)slots && a.grid_fault) {
            __hip_atomic_store(a.grid_fault, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    if (a.diag && lane == 0) {
        a.diag[2 * slot] = __builtin_amdgcn_s_memtime() - diag_t0;
        a.diag[2 * slot + 1] = __builtin_amdgcn_s_memrealtime() - diag_w0;
    }
}

__global__ __launch_bounds__(64, 2) void sw_dp16_lane_ck_kernel(const DpArgs a, const TbArgs walk)
{
    __shared__ __attribute__((aligned(16))) unsigned char out_lds[LANE_CK_OUT_LDS_BYTES]; // a tile's results on their way out
    lane_ck_grid<true, false, false>(a, walk, out_lds);
}

// results lane by lane through the caller's pointers (scattered destinations, strides the LDS form does not take); no LDS
__global__ __launch_bounds__(64, 2) void sw_dp16_lane_ck_scatter_kernel(const DpArgs a, const TbArgs walk) { lane_ck_grid<false, false, false>(a, walk, nullptr); }

// ... the twins for parameters with a folded diagonal (a.fold_k != 0, sw_device.h: diag_fold): the base-code waves form the diagonal
// in one v_pk_mad_u16 (sw_lane_cell.h, CMP_FOLD) -- and keep pass 1's kept rows (carry and middle rows alike) and checkpoints as the
// NARROW records (WaveMem; launch_dp16_lane_ck sends them only launches whose o - e is a byte)
__global__ __launch_bounds__(64, 2) void sw_dp16_lane_ck_kernel_fold(const DpArgs a, const TbArgs walk)
{
    __shared__ __attribute__((aligned(16))) unsigned char out_lds[LANE_CK_OUT_LDS_BYTES];
    lane_ck_grid<true, true, true>(a, walk, out_lds);
}
__global__ __launch_bounds__(64, 2) void sw_dp16_lane_ck_scatter_kernel_fold(const DpArgs a, const TbArgs walk) { lane_ck_grid<false, true, true>(a, walk, nullptr); }
// ... and the folded diagonal with the WIDE records, for the folding parameter sets the narrow ones do not take
__global__ __launch_bounds__(64, 2) void sw_dp16_lane_ck_kernel_fold_wide(const DpArgs a, const TbArgs walk)
{
    __shared__ __attribute__((aligned(16))) unsigned char out_lds[LANE_CK_OUT_LDS_BYTES];
    lane_ck_grid<true, true, false>(a, walk, out_lds);
}
__global__ __launch_bounds__(64, 2) void sw_dp16_lane_ck_scatter_kernel_fold_wide(const DpArgs a, const TbArgs walk) { lane_ck_grid<false, true, false>(a, walk, nullptr); }

// either wire format, the same for both sequence sets (the kernel stages base codes, sw_lane_cell.h)
bool lane16_ck_supported(const SeqSet &t, const SeqSet &q) { return (t.packed2 != 0) == (q.packed2 != 0); }

// a.lane_slots regions at a.tb / a.scratch; wherever the launch holds more tiles than slots: a.tile_ctr, one 64-bit word {draws, waves out}
// that stands at zero when the kernel starts and that no other launch in flight uses.  The grid's last wave out puts them back to zero
// (above), so no launch needs a reset in front of it -- a memset in front of every launch is a KERNEL of its own, and behind a grid that
// holds every wave slot of the chip it waited for that grid's end (traced in round 4: the two streams of the host entries stopped
// overlapping).
hipError_t launch_dp16_lane_ck(const DpArgs &a, const TbArgs &walk, hipStream_t stream)
{
    const int64_t tiles = ((a.count + 1) / 2 + 63) / 64;
    if (a.lane_slots < 1 || (tiles > a.lane_slots && !a.tile_ctr)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(tiles < a.lane_slots ? tiles : a.lane_slots)), block(64);
    // The narrow records (WaveMem) are a form of the *_fold twins: one form per kernel, chosen here, so that no store of pass 1 stands
    // behind a run-time branch and no kernel holds the registers of both forms.  They need 0 <= o - e <= 255 and a last row that is
    // not stored (a.uni_ql bounds the query of every wave of a grouped launch); a folding parameter set outside that, and
    // MGL_SW_DEBUG_CK_WIDE=1, take the *_fold_wide kernels: the same arithmetic, the wide records.  Parameters without a folded
    // diagonal keep the wide records (the narrow form of the unfolded kernels would be four kernels more for the slower half of the sets).
    const int o_e = a.gopen - a.gext;
    const bool narrow = !a.ck_wide && o_e >= 0 && o_e <= 255 && a.uni_ql <= ROW_KEY_MAX_QL;
    if (walk.coalesced_out)
        hipLaunchKernelGGL(!a.fold_k ? sw_dp16_lane_ck_kernel : narrow ? sw_dp16_lane_ck_kernel_fold : sw_dp16_lane_ck_kernel_fold_wide, grid, block, 0, stream, a, walk);
    else
        hipLaunchKernelGGL(!a.fold_k ? sw_dp16_lane_ck_scatter_kernel : narrow ? sw_dp16_lane_ck_scatter_kernel_fold : sw_dp16_lane_ck_scatter_kernel_fold_wide, grid, block, 0,
                           stream, a, walk);
    return hipGetLastError();
}

} // namespace mgl_sw_dev

#ifdef MGL_CK_TRACE
extern "C" int mgl_ck_trace_dump(const char *path)
{
    static unsigned long long h[4 << 17];
    hipDeviceSynchronize();
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(mgl_ck_trace), sizeof h) != hipSuccess) return 1;
    FILE *f = fopen(path, "wb");
    if (!f) return 2;
    fwrite(h, 1, sizeof h, f);
    fclose(f);
    memset(h, 0, sizeof h);
    hipMemcpyToSymbol(HIP_SYMBOL(mgl_ck_trace), h, sizeof h);
    return 0;
}
#endif

#ifdef MGL_CK_PHASES
extern "C" void mgl_ck_phases_dump()
{
    unsigned long long h[16] = {0};
    hipDeviceSynchronize();
    hipMemcpyFromSymbol(h, HIP_SYMBOL(mgl_ck_phase_ticks), sizeof h);
    static const char *names[8] = {"staging", "pass 1", "records", "stretches", "block flags", "walk in block", "(loop exit)", "finish"};
    unsigned long long tot = 0;
    for (int k = 0; k < 8; ++k) tot += h[k];
    for (int k = 0; k < 8; ++k) fprintf(stderr, "phase %-20s %6.2f %%  %10.1f ticks per wave\n", names[k], 100.0 * h[k] / (double)tot, (double)h[k] / (double)h[9]);
    fprintf(stderr, "waves %llu, block rounds per wave %.2f\n", h[9], (double)h[8] / (double)h[9]);
    fprintf(stderr, "edge stretches per wave: taken %.3f, tried and not adding up %.3f; verify iterations per wave %.2f\n", (double)h[10] / (double)h[9],
            (double)h[11] / (double)h[9], (double)h[12] / (double)h[9]);
    memset(h, 0, sizeof h);
    hipMemcpyToSymbol(HIP_SYMBOL(mgl_ck_phase_ticks), h, sizeof h);
}
#endif
