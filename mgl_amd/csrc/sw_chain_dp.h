// sw_chain_dp.h -- mgl_sw_chain_anchors_batch_device: the chain stage of seed - chain - extend.  A colinear chaining DP over a read's
// candidate anchors, the best chain traced back, and the chains of the batch written as the CSR arrays that
// mgl_sw_align_chain_batch_device reads (the definition is tests/chain_dp_textbook.py's).  The arguments of the
// three kernels and the layout of the workspace, shared by sw_chain_dp.hip and the host side (sw_chain_dp.cpp).
//
// The workspace, every part on a multiple of 256:
//   per read        `count`, K_p: the length of the read's chain (0 for a refused read)
//   per candidate   `stage`: the chain of read p, LAST anchor first, as indices from the read's first candidate, at
//                   stage[d_cand_start[p] ..].  The ranges of two reads that pass the range check cannot overlap unless a range
//                   between them descends; then they race for their common entries, and the compaction reads no candidate outside
//                   [0, total_cand) and writes no chain entry at or beyond total_cand
//   per wave        a slot of `slot_bytes` for pred, one byte per candidate (i - pred(i), 0 for -1) -- only where max_cand is above
//                   CHAIN_DP_LDS_PRED and the bytes do not fit the wave's LDS
#ifndef MGL_SW_CHAIN_DP_H
#define MGL_SW_CHAIN_DP_H

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mgl_sw_dev {

constexpr int64_t CHAIN_DP_MAX_CHUNK = (int64_t)1 << 30; // reads and candidates of one call
constexpr int CHAIN_DP_MAX_PRED = 64;                    // the ring: one wave
constexpr int CHAIN_DP_LDS_PRED = 32768;                 // candidates whose pred bytes a wave keeps in LDS
constexpr int CHAIN_DP_WAVES_PER_CU = 16;                // the DP grid: at most this many waves per CU

__host__ __device__ inline int64_t chain_dp_round(int64_t bytes, int64_t to) { return (bytes + to - 1) / to * to; }

// the int32 guard of pen: the largest value the sum in front of the shift can take
__host__ __device__ inline bool chain_dp_pen_ok(int max_dist_t, int max_dist_q, int bw, int pen_gap, int pen_skip)
{
    return (int64_t)pen_gap * bw + (int64_t)pen_skip * (max_dist_t < max_dist_q ? max_dist_t : max_dist_q) < ((int64_t)1 << 31);
}

struct ChainDpStaging {
    int64_t count, stage; // int32 per read, int32 per candidate
    int64_t bytes;        // the slots begin here
    int64_t slot_bytes;   // 0: pred lives in LDS
    int lds_bytes;        // the DP kernel's dynamic LDS
};
__host__ inline ChainDpStaging chain_dp_staging(int64_t n, int64_t total_cand, int max_cand)
{
    ChainDpStaging s{};
    s.count = 0;
    s.stage = chain_dp_round(n * 4, 256);
    s.bytes = s.stage + chain_dp_round(total_cand * 4, 256);
    const bool lds = max_cand <= CHAIN_DP_LDS_PRED;
    s.slot_bytes = lds ? 0 : chain_dp_round(max_cand, 256);
    s.lds_bytes = lds ? (int)chain_dp_round(max_cand > 64 ? max_cand : 64, 256) : 0;
    return s;
}

struct ChainDpArgs {
    const int32_t *t_len, *q_len;                // the caller's, per read
    const int64_t *cand_start;                   // n + 1
    const int32_t *cand_t, *cand_q, *cand_len;
    int64_t n, total_cand;
    int max_cand, max_pred, max_dist_t, max_dist_q, bw, pen_gap, pen_skip;
    // ---- workspace
    int32_t *count, *stage;
    unsigned char *ws;                           // the pred slots, or null
    int64_t slot_bytes;
    int waves, lds_bytes;
    // ---- the caller's outputs
    int64_t *chain_start;                        // n + 1
    int32_t *chain_t, *chain_q, *chain_len;      // total_cand each
    int32_t *chain_score;                        // n
    int32_t *f_out, *pred_out;                   // optional, per candidate
    int32_t *status;                             // optional, per read
    const int32_t *cand_group;                   // per candidate; null: sw_chain_dp_kernel<false>, every candidate in one group
};

hipError_t launch_chain_dp(const ChainDpArgs &a, hipStream_t stream);      // sw_chain_dp_kernel<cand_group != null>: count, stage, score, f, pred, status
hipError_t launch_chain_dp_scan(const ChainDpArgs &a, hipStream_t stream); // chain_start = the prefix sum of count
hipError_t launch_chain_dp_pack(const ChainDpArgs &a, hipStream_t stream); // the chains into their CSR place

} // namespace mgl_sw_dev

#endif
