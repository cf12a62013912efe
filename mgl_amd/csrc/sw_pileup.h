// sw_pileup.h -- mgl_sw_pileup_alignments_batch_device and mgl_sw_pileup_sites_device: the stage behind describe and classify.  What
// a batch of alignments adds up to per position of the reference -- eight planes of counts: the query's base over every M column, the
// deleted columns, the insertions behind a position and their bases -- and what those counts say per position: depth, the call, the
// best other base and the candidate sites (the definition is tests/pileup_textbook.py's).  The arguments of the
// kernels, shared by sw_pileup.hip and the host side (sw_pileup.cpp).  The first entry has no workspace; the second borrows one: a
// count and an offset per block of positions and the scan's storage.
#ifndef MGL_SW_PILEUP_H
#define MGL_SW_PILEUP_H

#include "../../include/mgl_sw.h"

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace mgl_sw_dev {

constexpr int PILEUP_PLANES = 8;                          // A C G T other | deleted | insertions, inserted bases
constexpr int64_t PILEUP_MAX_REGION = 0x7fffffff;         // positions of one table
constexpr int64_t PILEUP_MAX_SITES = (int64_t)1 << 30;    // site_capacity
constexpr int PILEUP_SITE_BLOCK = 256;                    // positions (and threads) of a block of the sites kernels

struct PileupArgs {
    const uint8_t *queries;
    const int64_t *t_start, *q_start;
    const int32_t *t_len, *q_len;
    const mgl_sw_chain_alignment *aln; // t_beg, t_end, q_beg, q_end alone are read
    const char *cigar;
    const int32_t *cigar_len;
    const int32_t *status_in, *select; // optional
    int64_t n;
    int cigar_stride, binary;
    int groups;                        // the grid
    int64_t region_beg, region_len;
    uint32_t *counts;                  // [8 * region_len], channel-major; added into
    int32_t *status;                   // optional
};

struct PileupSitesArgs {
    const uint32_t *counts;
    const uint8_t *ref;                // d_targets + region_beg
    int64_t region_len, blocks;        // blocks = ceil(region_len / PILEUP_SITE_BLOCK)
    int min_depth, min_alt, min_frac;
    int64_t *block_count, *block_start; // the workspace: [blocks + 1] each; block_start is the exclusive scan of block_count
    void *scan_tmp;
    size_t scan_bytes;
    uint8_t *call, *flags;             // optional
    mgl_sw_site *sites;                // optional where site_capacity is 0
    int64_t site_capacity;
    int64_t *n_sites;
};

hipError_t launch_pileup(const PileupArgs &a, hipStream_t stream);                  // sw_pileup_kernel
hipError_t pileup_scan_bytes(int64_t entries, size_t *bytes);                       // the scan's storage; no device work
hipError_t launch_pileup_flag(const PileupSitesArgs &a, hipStream_t stream);       // sw_pileup_flag_kernel: call, flags, sites per block
hipError_t launch_pileup_scan(const PileupSitesArgs &a, hipStream_t stream);       // rocPRIM's device scan over the blocks' counts
hipError_t launch_pileup_write(const PileupSitesArgs &a, hipStream_t stream);      // sw_pileup_write_kernel: the records, in position order

} // namespace mgl_sw_dev

#endif
