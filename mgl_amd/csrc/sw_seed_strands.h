// sw_seed_strands.h -- mgl_sw_seed_strands_batch_device and mgl_sw_select_strand_batch_device: the seed stage over both orientations of
// a read and the choice between them behind the chain stage (the definition is tests/strand_textbook.py's).  The
// arguments of the kernels and the layout of the workspace, shared by sw_seed_strands.hip and the host side (sw_seed_strands.cpp).
//
// Pair p is two ROWS: row 2p is (T_p, Q_p), row 2p + 1 is (T_p, rc(Q_p)).  The seed stage's workspace is seed_workspace(2n, max_cand) of
// sw_seed.h -- a count and a staging per ROW, so that sw_seed_scan_kernel and sw_seed_pack_kernel serve the 2n rows as they are -- and
// behind it one slot per workgroup of TWICE seed_workspace's slot_bytes: the first half is the forward row's (the layout sw_seed.h
// describes), the second the reverse row's.  The choice's workspace is one int32 per pair: K_p, or -1 for a refused pair.
#ifndef MGL_SW_SEED_STRANDS_H
#define MGL_SW_SEED_STRANDS_H

#include "sw_seed.h"

namespace mgl_sw_dev {

constexpr int64_t STRAND_MAX_PAIRS = (int64_t)1 << 29; // pairs of one call: 2^30 rows
constexpr int STRAND_LDS_TAB = 2048;                   // entries of ONE orientation's table kept in LDS
constexpr int STRAND_LDS_HITS = SEED_LDS_HITS;         // raw hits of ONE row kept in LDS

struct SeedStrandsArgs {
    SeedStageArgs s;                       // n = the ROWS (2 pairs'), the outputs over the rows; ws laid out as above
    int32_t *row_t_len, *row_q_len;        // optional, per row
};

struct SelectStrandArgs {
    const uint8_t *queries;                // the caller's
    const int64_t *q_start;
    const int32_t *q_len;
    const int64_t *chain_start;            // 2n + 1
    const int32_t *chain_t, *chain_q, *chain_len; // total_chain each
    const int32_t *chain_score;            // 2n
    int64_t n, total_chain, query_bytes;
    int32_t *count;                        // the workspace: n
    // ---- the caller's outputs
    int32_t *strand;                       // n
    uint8_t *queries_out;                  // query_bytes
    int64_t *anchor_start;                 // n + 1
    int32_t *anchor_t, *anchor_q, *anchor_len; // total_chain each
    int32_t *score, *status;               // optional, per pair
};

hipError_t launch_seed_strands(const SeedStrandsArgs &a, hipStream_t stream);       // sw_seed_strands_kernel: per row count, staging, status
hipError_t launch_select_strand(const SelectStrandArgs &a, hipStream_t stream);      // the choice, K_p, strand, score, status
hipError_t launch_select_strand_scan(const SelectStrandArgs &a, hipStream_t stream); // anchor_start = the prefix sum of K_p
hipError_t launch_select_strand_pack(const SelectStrandArgs &a, hipStream_t stream); // the anchors and the oriented reads

} // namespace mgl_sw_dev

#endif
