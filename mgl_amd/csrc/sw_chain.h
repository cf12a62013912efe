// sw_chain.h -- mgl_sw_align_chain_batch_device: a chain of colinear anchors aligned end to end -- the left side of the first anchor and
// the right side of the last one extended as mgl_sw_extend_seed_batch_device extends a seed's, every gap between two consecutive anchors
// filled globally over a diagonal band, all of it joined into one alignment (the definition is
// tests/chain_textbook.py's).  The output record, the staging of a batch and the three kernels around the extension kernels, shared by
// sw_chain.hip and the host side (sw_chain.cpp).
//
// The whole batch is staged in the context's workspace, in front of the slots (the anchor counts are device data: the host cannot cut
// the batch into chunks of known size):
//   per pair      what sw_seed_extend.h stages per pair -- the reversed left flanks, the four flank descriptors, `flank`, the two sides'
//                 outputs -- and `pstat`, the status the split gave the pair (0, MGL_SW_ERR_BAD_ARG or MGL_SW_ERR_UNSUPPORTED)
//   per anchor    the gap descriptor `owner`, and the gap's outputs: its score H(gt, gq), a status, a CIGAR length and a BINARY CIGAR
//                 row of gstride bytes (no rows when score-only).  Anchor a's gap is the one behind it
//
// The gap descriptor is the pair the anchor belongs to, or CHAIN_NO_OWNER.  The fill takes the gap's offsets into the caller's arrays
// from there: the owner's starts and anchors a and a + 1, which the split has checked.  One word, so that a d_anchor_start whose ranges
// overlap cannot leave a descriptor that is half one pair's and half another's: the split claims every anchor of a well-formed range
// [start[p], start[p + 1]) inside [0, total_anchors) with an atomic minimum, the lowest pair wins, and the join refuses a pair that does
// not own its whole range.  An anchor nobody claimed, a pair's last anchor and the anchors of a pair the split refused are no gap.
//
// gstride: seed_side_cigar_stride() at the gap bounds.  The argument of sw_seed_extend.h holds for a gap: of its n elements only the
// first and the last can merge into an anchor, each into another one (or, n = 1, both anchors and the gap into one), so the joined
// CIGAR has at least n elements, and a gap that overflows its row has more than the caller's row could hold joined.
#ifndef MGL_SW_CHAIN_H
#define MGL_SW_CHAIN_H

#include "sw_seed_extend.h"

namespace mgl_sw_dev {

struct ChainAlignment { // == mgl_sw_chain_alignment
    int32_t score, t_beg, t_end, q_beg, q_end, anchor_score, dropped, cigar_from;
};
static_assert(sizeof(ChainAlignment) == 32, "mgl_sw_chain_alignment is eight int32");

constexpr int CHAIN_NO_OWNER = 0x7f7f7f7f;           // above every pair index (SEED_MAX_CHUNK); what a memset of 0x7f leaves
constexpr int64_t CHAIN_MAX_SUM = (int64_t)1 << 30;  // the sum guard's bound

// The sum guard, per pair, on the normalised parameters.  A pair is K anchors, K - 1 gaps and two sides whose lengths add up to
// (tl, ql).  banded_range_ok() bounds a filled segment -- a gap or a side, K + 1 of them -- by s min + 2 gopen + gext max, an anchor is
// within s sl, and min(a) + min(b) <= min(a + b): the bounds add up to at most the left-hand side here, so every partial sum of
// segment scores lies within +-2^30 and the record's score is an int32
__host__ __device__ inline bool chain_sum_ok(int tl, int ql, int64_t k, int match, int mismatch, int gopen, int gext)
{
    const int64_t lo = tl < ql ? tl : ql;
    const int64_t s = (int64_t)match > -(int64_t)mismatch ? (int64_t)match : -(int64_t)mismatch;
    return s * lo + 2 * (int64_t)gopen * (k + 1) + (int64_t)gext * ((int64_t)tl + ql) <= CHAIN_MAX_SUM;
}

// where the parts of a batch of n pairs and `anchors` anchors stand, from the workspace's start; every part begins on a multiple of 256
struct ChainStaging {
    SeedStaging pair;                            // the per-pair parts, as sw_seed_extend.h lays them out, at offset 0
    int64_t pstat;                               // int32 per pair
    int64_t owner, gscore, gstatus, gclen, grow; // per anchor: int32 each, and rows of gstride bytes
    int64_t gstride;
    int64_t bytes;
};
__host__ inline ChainStaging chain_staging(int64_t n, int64_t anchors, int max_tl, int max_ql, int max_gap_tl, int max_gap_ql, int cigar_stride, bool binary,
                                           bool score_only)
{
    ChainStaging s{};
    s.pair = seed_staging(n, max_tl, max_ql, cigar_stride, binary, score_only);
    s.gstride = seed_side_cigar_stride(max_gap_tl, max_gap_ql, cigar_stride, binary, score_only);
    int64_t at = s.pair.bytes;
    auto part = [&](int64_t bytes) {
        const int64_t here = at;
        at += seed_round(bytes, 256);
        return here;
    };
    s.pstat = part(n * 4);
    s.owner = part(anchors * 4);
    s.gscore = part(anchors * 4);
    s.gstatus = part(anchors * 4);
    s.gclen = part(anchors * 4);
    s.grow = part(anchors * s.gstride);
    s.bytes = at;
    return s;
}

struct ChainArgs {
    const uint8_t *targets, *queries;              // the caller's
    const int64_t *t_start, *q_start;
    const int32_t *t_len, *q_len;
    const int64_t *anchor_start;                   // n + 1
    const int32_t *anchor_t, *anchor_q, *anchor_len;
    int64_t n, total_anchors;
    int max_tl, max_ql, max_gap_tl, max_gap_ql;
    int match, mismatch, gopen, gext;              // normalised
    int band;                                      // the fill's: at most max(max_gap_tl, max_gap_ql)
    // ---- staging per pair (sw_seed_extend.h)
    uint8_t *rev_t, *rev_q;
    int64_t tstride, qstride;
    int64_t *off[4];
    int32_t *len[4];
    int4 *flank;
    int32_t *pstat;
    const Extension *side_ext[2];
    const int32_t *side_status[2], *side_clen[2];
    const uint32_t *side_cigar[2];                 // binary rows of istride bytes; null when score_only
    int64_t istride;
    // ---- staging per anchor
    int32_t *owner, *gscore, *gstatus, *gclen;
    uint32_t *grow;                                // binary rows of gstride bytes; null when score_only
    int64_t gstride;
    // ---- the fill's slots
    unsigned char *ws;
    int64_t slot_bytes;
    int slots;
    // ---- the caller's outputs
    ChainAlignment *aln;
    Extension *left_out, *right_out;               // optional
    int32_t *gap_score_out;                        // optional; zeroed by the host before the join
    char *cigar;                                   // not score_only
    int cigar_stride;
    int32_t *cigar_len;                            // optional when score_only
    int32_t *status;                               // optional
    int binary_cigar, score_only;
};

hipError_t launch_chain_split(const ChainArgs &a, hipStream_t stream);
hipError_t launch_gap_fill(const ChainArgs &a, hipStream_t stream);
hipError_t launch_chain_join(const ChainArgs &a, hipStream_t stream);

} // namespace mgl_sw_dev

#endif
