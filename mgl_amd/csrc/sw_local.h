// sw_local.h -- local (zero-floor) Smith-Waterman, mgl_sw_local_batch_device_matrix: the arguments of its two kernels (sw_local.hip)
// and kernel A's range guard, shared by the kernels and the host side (sw_local.cpp).  tests/local_textbook.py mirrors
// local_lane_ok() and tests/test_local_textbook.py pins it at its edges.
#ifndef MGL_SW_LOCAL_H
#define MGL_SW_LOCAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sw_device.h"

namespace mgl_sw_dev {

// mgl_sw_local_hit
struct LocalHit {
    int32_t score, t_begin, t_end, q_begin, q_end;
};

constexpr int LOCAL_LANE_R = 32;               // kernel A: target rows per strip (registers)
constexpr int LOCAL_LANE_LDS_LIMIT = 64 * 1024; // kernel A: the LDS carve of one wave
constexpr int LOCAL_GHOST_CODE = MATRIX_DIM;   // kernel A: the code of a column beyond a query's end (a profile row of zero bytes)

// kernel A's byte bias: a profile entry is S + K, K = max(0, -min(matrix))
__host__ __device__ inline int local_lane_bias(int smin) { return smin < 0 ? -smin : 0; }
// code table, matrix, the strip profile (MATRIX_DIM + 1 codes x R rows: the ghost code's row is zero), the tile's target as codes
__host__ __device__ inline int local_lane_lds_bytes(int max_tl)
{
    return 256 + MATRIX_DIM * MATRIX_DIM + (MATRIX_DIM + 1) * LOCAL_LANE_R + (lane_strips(max_tl, LOCAL_LANE_R) * LOCAL_LANE_R + 15) / 16 * 16;
}
// Kernel A's range guard.  Kernel A keeps H, E, F as packed UNSIGNED 16-bit values floored at zero (v_pk_sub_u16 with clamp); the
// diagonal is H + (S + K) before the clamp takes K off again.  So: every S + K a byte, the largest H (max(S) per aligned pair, at most
// min(tl, ql) of them) plus a profile byte within 16 bits, the gap constants within 16 bits, the target's codes in the LDS carve.
// gopen / gext are the normalised (non-negative) penalties.
__host__ __device__ inline bool local_lane_ok(int smin, int smax, int gopen, int gext, int max_tl, int max_ql)
{
    if (max_tl < 1 || max_ql < 1 || gext < 0 || gopen < 0) return false;
    const int k = local_lane_bias(smin);
    if (smax + k > 255) return false;
    const int64_t lo = max_tl < max_ql ? max_tl : max_ql;
    if ((int64_t)(smax > 0 ? smax : 0) * lo + 255 > 65535) return false;
    if (gopen > 65535 || gext > 65535) return false;
    return local_lane_lds_bytes(max_tl) <= LOCAL_LANE_LDS_LIMIT;
}
// kernel A, one wave slot: the carry row (H, E of a strip's last row per column, 64 lanes; columns 0 .. max_ql and the three a group of
// four columns reads past the last) and the two queries as codes
__host__ __device__ inline int64_t local_lane_bnd_bytes(int max_ql) { return (int64_t)(max_ql + 4) * 64 * 8; }
__host__ __device__ inline int64_t local_lane_region_bytes(int max_ql)
{
    return (local_lane_bnd_bytes(max_ql) + (int64_t)((max_ql + 3) / 4) * 2 * 64 * 4 + 255) / 256 * 256;
}

// kernel B, one pair: the carry row (H, E per column) and, without score_only, one decision byte per cell laid out by anti-diagonal
// step ([strip of 64 rows][step][lane], ql + 63 steps a strip)
__host__ __device__ inline int64_t local_pair_dir_bytes(int tl, int ql) { return (int64_t)((tl + 63) / 64) * (ql + 63) * 64; }
__host__ __device__ inline int64_t local_pair_bytes(int tl, int ql, bool score_only)
{
    return ((int64_t)(ql + 1) * 8 + (score_only ? 0 : local_pair_dir_bytes(tl, ql)) + 255) / 256 * 256;
}

struct LocalArgs {
    SeqSet t, q;              // ASCII, per-pair start + length (len arrays set)
    int64_t first, count;     // pairs [first, first + count)
    int gopen, gext;          // normalised
    int smin, smax;           // of the matrix
    int max_tl, max_ql;       // the caller's bounds (a pair beyond them: MGL_SW_ERR_BAD_ARG)
    const int8_t *matrix;     // MATRIX_DIM x MATRIX_DIM, row = target code
    const uint8_t *code;      // 256 bytes -> 0 .. MATRIX_DIM-1
    LocalHit *hit;            // per pair
    int32_t *status;          // optional
    char *cigar;              // kernel B, not score_only
    int cigar_stride;
    int32_t *cigar_len;
    int binary_cigar;
    int score_only;
    // kernel B: workspace of `slots` pairs, slot_bytes each (pair first + k uses slot k)
    unsigned char *ws;
    int64_t slot_bytes;
    // kernel A: persistent grid over tiles of 128 pairs
    const int32_t *tile_order; // tiles largest first
    int lane_slots;            // wave slots = regions of local_lane_region_bytes(max_ql) at ws
    unsigned *tile_ctr;        // {draws, waves out}, zero at launch (needed when tiles > lane_slots); the last wave out zeroes it
    int32_t *grid_fault;       // optional: a wave drew a number no launch of its size can draw
};

hipError_t launch_local_lane(const LocalArgs &a, hipStream_t stream);
hipError_t launch_local_pairs(const LocalArgs &a, hipStream_t stream);

} // namespace mgl_sw_dev

#endif
