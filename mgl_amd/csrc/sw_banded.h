// sw_banded.h -- mgl_sw_align_batch_device_banded: the GATK function restricted to a diagonal band (the
// definition is tests/banded_textbook.py's).  The band's geometry, the range guard and the workspace formulas, shared by the kernel
// (sw_banded.hip) and the host side (sw_banded.cpp).  tests/banded_textbook.py mirrors banded_range_ok() and the slot formulas,
// tests/test_banded_textbook.py pins them at their edges.
#ifndef MGL_SW_BANDED_H
#define MGL_SW_BANDED_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sw_device.h"

namespace mgl_sw_dev {

// Minus infinity of the banded kernel: what a read from an out-of-band cell gives.  The range guard keeps every finite H, E, F within
// +-2^29 and gext within 2^24, so the sentinel loses every comparison strictly, `sentinel - gext` neither wraps nor reaches a finite
// value, and the open (a finite H - gopen) replaces it at the first in-band cell.
constexpr int BANDED_NEG = -(1 << 30);
constexpr int BANDED_MAX_LEN = 1 << 28;     // lengths beyond this are outside the guard (int32 geometry)
constexpr int64_t BANDED_MAX_SCORE = 1 << 29;

// cell (i, j), border included, is in the band iff lo <= j - i <= hi.  `band` is at most BANDED_MAX_LEN here (the host clamps it: a
// band of max(tl, ql) covers a pair's matrix, a wider one just the same)
__host__ __device__ inline int banded_lo(int tl, int ql, int band) { return (ql < tl ? ql - tl : 0) - band; }
__host__ __device__ inline int banded_hi(int tl, int ql, int band) { return (ql > tl ? ql - tl : 0) + band; }

// The range guard, per pair, on the normalised parameters.  Every finite value of the recurrence lies in
// [-(|mismatch| min(tl, ql) + 2 gopen + gext max(tl, ql)), match min(tl, ql)]: a border is at least -(gopen + gext (max - 1)), a
// diagonal step adds at least mismatch and at most match, an E or F is at least the H it opened from minus gopen.
__host__ __device__ inline bool banded_range_ok(int tl, int ql, int match, int mismatch, int gopen, int gext)
{
    if (tl < 1 || ql < 1 || tl > BANDED_MAX_LEN || ql > BANDED_MAX_LEN) return false;
    if (match < 0 || mismatch > 0 || gopen < 0 || gext < 0 || gopen > (1 << 24) || gext > (1 << 24)) return false;
    const int64_t lo = tl < ql ? tl : ql, hi = tl < ql ? ql : tl;
    const int64_t s = (int64_t)match > -(int64_t)mismatch ? (int64_t)match : -(int64_t)mismatch;
    return s * lo + 2 * (int64_t)gopen + (int64_t)gext * hi <= BANDED_MAX_SCORE;
}

// ---- one pair's workspace slot: the carry row | the CIGAR elements of the walk | the decisions.
// The carry row: {H, E} of the row above the strip per column 0 .. ql.  The walk's elements: one dword each, at most tl + ql + 4.
// The decisions: four bits per cell, eight steps of a lane in a dword, [strip of 64 rows][step / 8][lane]; strip k sweeps the columns
// max(1, 64k + 1 + lo) .. min(ql, 64k + 64 + hi) -- at most min(ql, hi - lo + 64) of them -- in that many steps plus 63 of skew,
// rounded up to whole dwords
__host__ __device__ inline int64_t banded_carry_bytes(int ql) { return ((int64_t)(ql + 1) * 8 + 255) / 256 * 256; }
__host__ __device__ inline int64_t banded_elem_bytes(int tl, int ql) { return ((int64_t)(tl + ql + 4) * 4 + 255) / 256 * 256; }
__host__ __device__ inline int banded_strip_steps(int tl, int ql, int band)
{
    const int64_t w = (int64_t)banded_hi(tl, ql, band) - banded_lo(tl, ql, band) + 64;
    return (int)((((int64_t)ql < w ? (int64_t)ql : w) + 63 + 7) & ~(int64_t)7);
}
__host__ __device__ inline int64_t banded_dir_bytes(int tl, int ql, int band) { return (int64_t)((tl + 63) / 64) * banded_strip_steps(tl, ql, band) * 32; }
__host__ __device__ inline int64_t banded_pair_bytes(int tl, int ql, int band, bool score_only)
{
    return banded_carry_bytes(ql) + (score_only ? 0 : banded_elem_bytes(tl, ql) + banded_dir_bytes(tl, ql, band));
}
// What the host sizes every slot with (it cannot see the lengths): the largest banded_pair_bytes of any pair within (max_tl, max_ql) --
// 27 MiB for 10 000 x 10 000 at band 512, where the square pair itself needs 5.7 MiB; tests/banded_textbook.py mirrors it and
// tests/test_banded_textbook.py checks the mirror by brute force.  The largest of any pair: for a given number of strips the steps grow with ql above tl
// (take max_ql and the fewest rows) and, below tl, peak where ql meets tl - ql + 2 band + 64 (take the most rows)
__host__ inline int64_t banded_slot_bound(int max_tl, int max_ql, int band, bool score_only)
{
    const int64_t fixed = banded_carry_bytes(max_ql) + (score_only ? 0 : banded_elem_bytes(max_tl, max_ql));
    if (score_only) return fixed;
    const int strips = (max_tl + 63) / 64;
    if (strips > (1 << 16)) return fixed + (int64_t)strips * (((int64_t)max_ql + 63 + 7) & ~(int64_t)7) * 32; // (no pair needs more)
    int64_t best = 0;
    for (int k = 1; k <= strips; ++k) {
        const int t_min = 64 * (k - 1) + 1, t_max = 64 * k < max_tl ? 64 * k : max_tl;
        const int64_t peak = ((int64_t)t_max + 2 * (int64_t)band + 64 + 1) / 2;
        const int qs[4] = {max_ql, (int)(peak < max_ql ? peak : max_ql), (int)(peak + 1 < max_ql ? peak + 1 : max_ql), t_max < max_ql ? t_max : max_ql};
        for (int x = 0; x < 4; ++x) {
            const int q = qs[x] < 1 ? 1 : qs[x];
            const int64_t s1 = banded_strip_steps(t_min, q, band), s2 = banded_strip_steps(t_max, q, band);
            const int64_t s = s1 > s2 ? s1 : s2;
            if ((int64_t)k * s > best) best = (int64_t)k * s;
        }
    }
    return fixed + best * 32;
}

constexpr int BANDED_WAVES_PER_CU = 8; // the grid: at most this many resident waves per CU, one workspace slot each

struct BandedArgs {
    SeqSet t, q;              // ASCII, per-pair start + length (len arrays set)
    int64_t n;                // pairs 0 .. n - 1: wave w takes pairs w, w + slots, w + 2 slots, ...
    int match, mismatch, gopen, gext, strategy; // normalised
    int band;                 // at most max(max_tl, max_ql)
    int max_tl, max_ql;       // the caller's bounds (a pair beyond them: MGL_SW_ERR_BAD_ARG)
    int32_t *offset;
    Score *score;
    char *cigar;              // not score_only
    int cigar_stride;
    int32_t *cigar_len;
    int32_t *status;          // optional
    int binary_cigar;
    int score_only;
    unsigned char *ws;        // `slots` slots of slot_bytes
    int64_t slot_bytes;
    int slots;                // = waves of the launch
};

hipError_t launch_banded(const BandedArgs &a, hipStream_t stream);

} // namespace mgl_sw_dev

#endif
