// sw_rank.h -- mgl_sw_rank_chains_batch_device: the stage behind the chain DP.  The best max_chains chains of every read backtracked
// from the chain stage's f and pred over the read's rows, ranked, marked primary or secondary and given a mapping quality (DESIGN.md
// section 9k; the definition is tests/rank_textbook.py's).  The arguments of the two kernels and the layout of the workspace, shared by
// sw_rank.hip and the host side (sw_rank.cpp).
//
// The workspace, both parts on a multiple of 256:
//   per read        `count`: the anchors of the read's kept chains together (0 for a refused read)
//   per candidate   `stage` (only where the anchor outputs are wanted): the kept chains of read p one after the other in rank order,
//                   each ascending, as indices into the candidate arrays, at stage[d_cand_start[strands * p] ..].  The chains of a
//                   read are disjoint, so they fit the read's own range.  The ranges of two reads that pass the range check cannot
//                   overlap unless a range between them descends; then they race for their common entries, and the pack kernel reads
//                   no candidate outside [0, total_cand) and writes no entry at or beyond total_cand
// There are no slots: a row's working set lives in LDS at every supported size (sw_rank.hip).
#ifndef MGL_SW_RANK_H
#define MGL_SW_RANK_H

#include "../../include/mgl_sw.h"

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mgl_sw_dev {

constexpr int64_t RANK_MAX_CHUNK = (int64_t)1 << 30; // rows and candidates of one call
constexpr int RANK_THREADS = 256;                    // a workgroup per read
constexpr int RANK_MAX_CHAINS = 16;                  // the list the lanes hold
constexpr int RANK_MAX_PRED = 64;                    // i - pred(i) is kept as a byte
constexpr int RANK_CAP_SMALL = 4096;                 // rows up to here: two workgroups per CU
constexpr int RANK_MAX_CAND = 8192;                  // the seed stages' ceiling: one workgroup per CU

__host__ __device__ inline int64_t rank_round(int64_t bytes, int64_t to) { return (bytes + to - 1) / to * to; }

struct RankWorkspace {
    int64_t count, stage; // int32 per read, int32 per candidate (anchors wanted)
    int64_t bytes;
};
__host__ inline RankWorkspace rank_workspace(int64_t n, int64_t total_cand, bool anchors)
{
    RankWorkspace w{};
    w.count = 0;
    w.stage = rank_round(n * 4, 256);
    w.bytes = w.stage + (anchors ? rank_round(total_cand * 4, 256) : 0);
    return w;
}

struct RankArgs {
    const int32_t *row_q_len;                   // rows
    const int64_t *cand_start;                  // rows + 1
    const int32_t *cand_t, *cand_q, *cand_len;  // total_cand
    const int32_t *f, *pred;                    // total_cand: the chain stage's
    const int32_t *row_status;                  // optional, rows
    int64_t n, total_cand;                      // n: the reads
    int strands, max_cand, max_chains, min_score, min_cnt, mask_level;
    int groups;                                 // the grid of sw_rank_chains_kernel
    // ---- workspace
    int32_t *count, *stage;                     // stage: null where no anchors are wanted
    // ---- the caller's outputs
    int32_t *n_chains;                          // n
    mgl_sw_ranked_chain *records;               // n * max_chains
    int64_t *ranked_start;                      // optional, n + 1, with the three below
    int32_t *ranked_t, *ranked_q, *ranked_len;  // total_cand each
    int32_t *status;                            // optional, n
};

hipError_t launch_rank_chains(const RankArgs &a, hipStream_t stream); // sw_rank_chains_kernel: n_chains, records, status, count, stage
hipError_t launch_rank_pack(const RankArgs &a, hipStream_t stream);   // sw_rank_pack_kernel: the staged candidates into their CSR place

} // namespace mgl_sw_dev

#endif
