// sw_describe.h -- mgl_sw_describe_alignments_batch_device: the stage behind an alignment.  What the alignment's CIGAR says about its
// two spans: matches, mismatches, inserted and deleted bases and runs, the MD text and the extended (= / X) CIGAR (DESIGN.md section
// 9l; the definition is tests/describe_textbook.py's).  The arguments of the kernel, shared by sw_describe.hip and the host side
// (sw_describe.cpp).  No workspace: everything the kernel keeps lives in registers and in the wave's own part of LDS.
#ifndef MGL_SW_DESCRIBE_H
#define MGL_SW_DESCRIBE_H

#include "../../include/mgl_sw.h"

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mgl_sw_dev {

constexpr int64_t DESCRIBE_MAX_CHUNK = (int64_t)1 << 30; // alignments of one call
constexpr int DESCRIBE_WAVES = 4;                        // waves of a workgroup, each on alignments of its own
constexpr int DESCRIBE_CHUNK = 512;                      // CIGAR elements a wave keeps in LDS at a time
constexpr int DESCRIBE_GROUPS_PER_CU = 4;                // 16 waves a CU: 4 a SIMD

struct DescribeArgs {
    const uint8_t *targets, *queries;
    const int64_t *t_start, *q_start;
    const int32_t *t_len, *q_len;
    const mgl_sw_chain_alignment *aln; // t_beg, t_end, q_beg, q_end alone are read
    const char *cigar;
    const int32_t *cigar_len;
    const int32_t *status_in;          // optional
    int64_t n;
    int cigar_stride, md_stride, xcigar_stride, binary;
    int groups;                        // the grid
    mgl_sw_alignment_stats *stats;
    char *md, *xcigar;                 // optional
    int32_t *status;                   // optional
};

hipError_t launch_describe(const DescribeArgs &a, hipStream_t stream); // sw_describe_kernel

} // namespace mgl_sw_dev

#endif
