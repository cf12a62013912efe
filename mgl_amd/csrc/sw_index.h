// sw_index.h -- the minimizer index of one reference and the two stages around it: mgl_sw_index_build_device,
// mgl_sw_seed_index_batch_device and mgl_sw_locate_window_batch_device (the definition is
// tests/index_textbook.py's).  The arguments of the kernels, shared by sw_index.hip and the host side (sw_index.cpp).
//
// The index: the reference's sketch (sw_seed.h: the (w, k) minimizers) as M entries ascending by (key, position), keys and positions
// apart, and a bucket table over the top `bucket_bits` = min(2k, INDEX_MAX_BUCKET_BITS, max(INDEX_MIN_BUCKET_BITS, ceil(log2 M)))
// bits of a key: bucket[b] is the first entry whose key's top bits are not below b, bucket[2^bucket_bits] = M.  A lookup reads one
// pair of bucket bounds and searches between them -- about one entry per bucket while M is below 2^INDEX_MAX_BUCKET_BITS.
//
// The seed stage's workspace is seed_workspace(rows, max_cand) of sw_seed.h -- a count and a staging per ROW (rows = strands * n), so
// that sw_seed_scan_kernel and sw_seed_pack_kernel serve the rows as they are -- and behind it ONE slot of seed_workspace's slot_bytes
// per workgroup: a read's rows are worked off one after the other.  Locate has no workspace.
#ifndef MGL_SW_INDEX_H
#define MGL_SW_INDEX_H

#include "sw_seed.h"

namespace mgl_sw_dev {

constexpr int INDEX_MIN_BUCKET_BITS = 10, INDEX_MAX_BUCKET_BITS = 24;
constexpr int INDEX_MAX_OCC_REF = 8192;
constexpr int INDEX_SCAN_THREADS = 256; // block counts the build's scan sums in one step
constexpr int64_t INDEX_MAX_REF = ((int64_t)1 << 31) - 1;

struct IndexView {
    const uint32_t *keys;   // M, ascending
    const int32_t *pos;     // M, ascending within a key
    const uint32_t *bucket; // 2^bucket_bits + 1
    int64_t ref_len, entries;
    int k, w, bucket_bits;
};

struct IndexBuildArgs {
    const uint8_t *ref;
    int64_t ref_len, blocks; // blocks of SEED_BLOCK k-mer positions
    int k, w;
    uint32_t *block_count;   // blocks: a block's selected positions
    uint32_t *block_start;   // blocks + 1: their exclusive prefix sum, M at the end
    uint64_t *entries;       // M: key << 32 | position (the second pass)
};

struct SeedIndexArgs {
    IndexView ix;
    SeedStageArgs s;                // n = the ROWS; targets, t_start, t_len unused; k, w the index's; ws laid out as above
    int strands, max_occ_ref;
    int32_t *row_t_len, *row_q_len; // optional, per row
};

struct LocateArgs {
    const int32_t *q_len;
    const int64_t *anchor_start;                       // n + 1
    const int32_t *anchor_t, *anchor_q, *anchor_len;   // total_anchors each
    int64_t n, ref_len, total_anchors;
    int slack, max_tl;
    // ---- the caller's outputs
    int64_t *t_start; // n
    int32_t *t_len;   // n
    int32_t *anchor_t_out; // total_anchors; may be anchor_t
    int32_t *status;  // optional
};

// The contigs of a reference (mgl_sw_index_build_contigs_device; tests/contig_textbook.py): contig c is
// [start[c], end[c]) of the buffer, ascending, with at least one byte that is no base between two of them.  n = 0: no table, ONE contig
// [0, ref_len) -- what an index of mgl_sw_index_build_device is to the stages below.
constexpr int64_t CONTIG_MAX = (int64_t)1 << 20;
constexpr int CONTIG_LDS_MAX = 4096; // contigs whose start and end sw_contig_of_kernel searches in LDS (32 KiB)
struct ContigView {
    const int32_t *start, *end; // n each, device memory
    int32_t n, ref_len;
};

struct ContigOfArgs {
    ContigView cv;
    int64_t total;
    const int32_t *t, *len; // total each
    int32_t *group;         // total
};

struct LocateContigsArgs {
    LocateArgs l;     // ref_len unused: cv has it
    ContigView cv;
    int32_t *rid;     // n
};

hipError_t launch_contig_gaps(const uint8_t *ref, const ContigView &cv, int32_t *flag, hipStream_t stream); // sw_contig_gap_kernel: *flag = 1 for a base in a gap
hipError_t launch_contig_of(const ContigOfArgs &a, hipStream_t stream);                    // sw_contig_of_kernel
hipError_t launch_locate_window_contigs(const LocateContigsArgs &a, hipStream_t stream);   // sw_locate_window_contigs_kernel
hipError_t launch_index_count(const IndexBuildArgs &a, hipStream_t stream);  // sw_index_sketch_kernel, pass 1: block_count
hipError_t launch_index_scan(const IndexBuildArgs &a, hipStream_t stream);   // block_start
hipError_t launch_index_write(const IndexBuildArgs &a, hipStream_t stream);  // sw_index_sketch_kernel, pass 2: entries
hipError_t index_sort_entries(uint64_t *entries, uint64_t *sorted, int64_t m, int k, hipStream_t stream); // by bits [0, 32 + 2k); frees its storage
hipError_t launch_index_split(const uint64_t *sorted, int64_t m, uint32_t *keys, int32_t *pos, hipStream_t stream);
hipError_t launch_index_buckets(const uint32_t *keys, int64_t m, int k, int bucket_bits, uint32_t *bucket, hipStream_t stream);
hipError_t launch_seed_index(const SeedIndexArgs &a, hipStream_t stream);    // sw_seed_index_kernel: per row count, staging, status
hipError_t launch_locate_window(const LocateArgs &a, hipStream_t stream);    // sw_locate_window_kernel

} // namespace mgl_sw_dev

#endif
