// sw_lines.h -- mgl_sw_expand_chains_batch_device and mgl_sw_classify_alignments_batch_device: the two stages that let the read mapper
// align every ranked chain (the definition is tests/lines_textbook.py's).  The first turns "read with up to 16
// ranked chains" into "one alignment job per chain", the second turns the jobs' alignments back into the lines of a read.  The arguments
// of the kernels and the layout of the one workspace, shared by sw_lines.hip and the host side (sw_lines.cpp).
//
// The workspace of the expand stage, every part on a multiple of 256:
//   per read   `jobs` (int32): the read's jobs, 0 for a refused or cut read
//   per read   `anchors` (int32): the anchors of those jobs together
//   per read   `strands` (int32): bit 0 -- a job on strand 0, bit 1 -- a job on strand 1
//   per read   `anchor_at` (int64): where the first job's anchors go in the jobs' anchor arrays
// The classify stage has no workspace.
#ifndef MGL_SW_LINES_H
#define MGL_SW_LINES_H

#include "../../include/mgl_sw.h"

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mgl_sw_dev {

constexpr int64_t LINES_MAX_READS = (int64_t)1 << 29; // reads of one call
constexpr int64_t LINES_MAX_JOBS = (int64_t)1 << 30;  // jobs of one call
constexpr int64_t LINES_MAX_BYTES = (int64_t)1 << 40; // query_bytes
constexpr int LINES_MAX_CHAINS = 16;                  // the rank stage's list: a quarter wave holds a read's jobs
constexpr int LINES_ORIENT_THREADS = 256;             // a workgroup per (read, strand)

__host__ __device__ inline int64_t lines_round(int64_t bytes, int64_t to) { return (bytes + to - 1) / to * to; }

struct ExpandWorkspace {
    int64_t jobs, anchors, strands, anchor_at;
    int64_t bytes;
};
__host__ inline ExpandWorkspace expand_workspace(int64_t n)
{
    ExpandWorkspace w{};
    const int64_t per = lines_round(n * 4, 256);
    w.jobs = 0;
    w.anchors = per;
    w.strands = 2 * per;
    w.anchor_at = 3 * per;
    w.bytes = 3 * per + lines_round(n * 8, 256);
    return w;
}

struct ExpandArgs {
    const uint8_t *queries;                     // query_bytes
    const int64_t *q_start;                     // n
    const int32_t *q_len;                       // n
    const int32_t *rank_status;                 // optional, n
    const int32_t *n_chains;                    // n
    const mgl_sw_ranked_chain *records;         // n * max_chains
    const int64_t *ranked_start;                // n + 1
    const int32_t *ranked_t, *ranked_q, *ranked_len; // total_anchors
    int64_t n, query_bytes, total_anchors, job_capacity;
    int max_chains, keep_secondary;
    int groups;                                 // the grid of the orientation copy
    // ---- workspace
    int32_t *ws_jobs, *ws_anchors, *ws_strands;
    int64_t *ws_anchor_at;
    // ---- the caller's outputs
    int64_t *n_jobs;                            // 1
    int64_t *job_start;                         // n + 1
    mgl_sw_job *jobs;                           // job_capacity
    int64_t *job_q_start;                       // job_capacity
    int32_t *job_q_len;                         // job_capacity
    int64_t *job_anchor_start;                  // job_capacity + 1
    int32_t *job_anchor_t, *job_anchor_q, *job_anchor_len; // total_anchors
    uint8_t *oriented;                          // 2 * query_bytes
    int32_t *status;                            // optional, n
};

struct ClassifyArgs {
    const int64_t *job_start;                   // n + 1
    const mgl_sw_job *jobs;                     // job_capacity
    const mgl_sw_chain_alignment *aln;          // job_capacity
    const int32_t *aln_status;                  // job_capacity
    int64_t n, job_capacity;
    int match, min_score, mask_level;
    mgl_sw_line *lines;                         // job_capacity
    int32_t *n_lines, *primary_job;             // n
    int32_t *status;                            // optional, n
};

hipError_t launch_expand_count(const ExpandArgs &a, hipStream_t stream);  // sw_expand_count_kernel: the checks, the workspace's counts
hipError_t launch_expand_scan(const ExpandArgs &a, hipStream_t stream);   // sw_expand_scan_kernel: the capacity rule, job_start, anchor_at, n_jobs
hipError_t launch_expand_pack(const ExpandArgs &a, hipStream_t stream);   // sw_expand_pack_kernel: the jobs, their arrays and anchors, the empty tail
hipError_t launch_expand_orient(const ExpandArgs &a, hipStream_t stream); // sw_expand_orient_kernel: the oriented buffer
hipError_t launch_classify(const ClassifyArgs &a, hipStream_t stream);    // sw_classify_kernel: a quarter wave per read

} // namespace mgl_sw_dev

#endif
