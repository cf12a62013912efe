// sw_extend.h -- mgl_sw_extend_batch_device: anchored extension with Z-drop over a band centred on the main diagonal (DESIGN.md
// section 9c; the definition is tests/extend_textbook.py's).  The output record and the workspace formulas, shared by the kernel
// (sw_extend.hip) and the host side (sw_extend.cpp); minus infinity, the range guard and the carry / element parts of a slot are the
// banded entry's (sw_banded.h).  tests/extend_textbook.py mirrors the slot formulas, tests/test_extend_textbook.py pins them.
#ifndef MGL_SW_EXTEND_H
#define MGL_SW_EXTEND_H

#include "sw_banded.h"

namespace mgl_sw_dev {

struct Extension { // == mgl_sw_extension
    int32_t score, t_end, q_end, score_qend, t_end_qend, rows_done, dropped, cigar_from;
};
static_assert(sizeof(Extension) == 32, "mgl_sw_extension is eight int32");

constexpr int EXTEND_NO_QEND = -0x40000000; // score_qend where no row of the extension reaches column ql in the band

// ---- one pair's workspace slot: the carry row | the CIGAR elements of the walk | the decisions, as in sw_banded.h.  The band is
// -band <= j - i <= band whatever the lengths are, so strip k sweeps the columns max(1, 64k + 1 - band) .. min(ql, 64k + 64 + band) --
// at most min(ql, 2 band + 64) of them -- in that many steps plus 63 of skew, rounded up to whole dwords.  Monotone in tl and in ql:
// the host sizes every slot at (max_tl, max_ql)
__host__ __device__ inline int extend_strip_steps(int ql, int band)
{
    const int64_t w = 2 * (int64_t)band + 64;
    return (int)((((int64_t)ql < w ? (int64_t)ql : w) + 63 + 7) & ~(int64_t)7);
}
__host__ __device__ inline int64_t extend_pair_bytes(int tl, int ql, int band, bool score_only)
{
    return banded_carry_bytes(ql) + (score_only ? 0 : banded_elem_bytes(tl, ql) + (int64_t)((tl + 63) / 64) * extend_strip_steps(ql, band) * 32);
}

// ---- MGL_SW_FLAG_EXTEND_ADAPTIVE_BAND (the definition is tests/extend_adaptive_textbook.py's, which mirrors the
// formula): the band is re-centred every EXTEND_RECENTRE_ROWS rows, a strip's sweep is as wide as before, and behind the decisions the
// slot keeps one int32 per strip, the strip's centre d_k, which the walk reads back.  Still monotone in tl and in ql
constexpr int EXTEND_RECENTRE_ROWS = 64; // == MGL_SW_EXTEND_RECENTRE_ROWS: the kernel's strip, and part of the function's definition
__host__ __device__ inline int64_t extend_centre_bytes(int tl) { return ((int64_t)((tl + 63) / 64) * 4 + 255) / 256 * 256; }
__host__ __device__ inline int64_t extend_adaptive_pair_bytes(int tl, int ql, int band, bool score_only)
{
    return extend_pair_bytes(tl, ql, band, score_only) + (score_only ? 0 : extend_centre_bytes(tl));
}

struct ExtendArgs {
    SeqSet t, q;              // ASCII, per-pair start + length (len arrays set)
    int64_t n;                // pairs 0 .. n - 1: wave w takes pairs w, w + slots, w + 2 slots, ...
    int match, mismatch, gopen, gext; // normalised
    int band;                 // at most max(max_tl, max_ql); launch_extend_adaptive: at most 2 BANDED_MAX_LEN
    int zdrop;                // < 0: off
    int max_tl, max_ql;       // the caller's bounds (a pair beyond them: MGL_SW_ERR_BAD_ARG)
    Extension *ext;
    char *cigar;              // not score_only
    int cigar_stride;
    int32_t *cigar_len;
    int32_t *status;          // optional
    int binary_cigar;
    int score_only;
    int to_query_end;         // MGL_SW_FLAG_EXTEND_TO_QUERY_END
    unsigned char *ws;        // `slots` slots of slot_bytes
    int64_t slot_bytes;
    int slots;                // = waves of the launch
};

hipError_t launch_extend(const ExtendArgs &a, hipStream_t stream);
hipError_t launch_extend_adaptive(const ExtendArgs &a, hipStream_t stream); // sw_extend_adaptive.hip

} // namespace mgl_sw_dev

#endif
