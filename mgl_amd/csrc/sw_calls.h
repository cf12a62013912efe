// sw_calls.h -- mgl_sw_pileup_insertions_batch_device and mgl_sw_genotype_sites_device: the stage behind the pileup and its sites.
// What the insertions behind the candidate sites ARE -- per site a row of counts: how many insertions of which length, and which base
// stands in which of their columns -- and what the planes and those rows say per site: the events (a substitution, a deletion run, an
// insertion), their genotype, its likelihoods and its quality, in integers (the definition is
// tests/calls_textbook.py's).  The arguments of the kernels, shared by sw_calls.hip and the host side (sw_calls.cpp).  The first entry
// has no workspace; the second borrows one: a count and an offset per block of site slots and the scan's storage.
#ifndef MGL_SW_CALLS_H
#define MGL_SW_CALLS_H

#include "../../include/mgl_sw.h"

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace mgl_sw_dev {

constexpr int CALLS_MAX_INS = 64;                         // max_ins: the inserted columns a row keeps (a lane each)
constexpr int CALLS_MAX_DEL = 4096;                       // max_del: the sites one deletion call runs over
constexpr int CALLS_MAX_COST = 1 << 20;                   // a cost, in 1/256 phred per read
constexpr int64_t CALLS_MAX_CALLS = (int64_t)1 << 30;     // call_capacity
constexpr int CALLS_SITE_BLOCK = 256;                     // site slots (and threads) of a block of the genotype kernels

struct InsertionsArgs {
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
    int64_t region_beg;
    const mgl_sw_site *sites;          // pos and nothing else is read, of the first min(max(n_sites[0], 0), site_capacity) records
    const int64_t *n_sites;
    int64_t site_capacity;
    int max_ins;
    uint32_t *ins;                     // [site_capacity * (6 * max_ins + 1)]; added into
    int32_t *status;                   // optional
};

struct GenotypeArgs {
    const uint32_t *counts;            // the pileup's planes
    const uint8_t *ref;                // d_targets + region_beg
    int64_t region_len;
    const mgl_sw_site *sites;
    const int64_t *n_sites;
    int64_t site_capacity, blocks;     // blocks = ceil(site_capacity / CALLS_SITE_BLOCK)
    const uint32_t *ins;               // optional: without it no insertion is called
    int max_ins, max_del;
    int cost_match, cost_het, cost_error;
    int64_t *block_count, *block_start; // the workspace: [blocks + 1] each; block_start is the exclusive scan of block_count
    void *scan_tmp;
    size_t scan_bytes;
    mgl_sw_call *calls;                // optional where call_capacity is 0
    int64_t call_capacity;
    int64_t *n_calls;
    uint8_t *ins_seq;                  // [call_capacity * max_ins]; optional without ins
};

hipError_t launch_insertions(const InsertionsArgs &a, hipStream_t stream);        // sw_insertions_kernel
hipError_t genotype_scan_bytes(int64_t entries, size_t *bytes);                   // the scan's storage; no device work
hipError_t launch_genotype_count(const GenotypeArgs &a, hipStream_t stream);      // sw_genotype_count_kernel: events per block
hipError_t launch_genotype_scan(const GenotypeArgs &a, hipStream_t stream);       // rocPRIM's device scan over the blocks' counts
hipError_t launch_genotype_write(const GenotypeArgs &a, hipStream_t stream);      // sw_genotype_write_kernel: the records, in site order

} // namespace mgl_sw_dev

#endif
