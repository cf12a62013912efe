// sw_seed_extend.h -- mgl_sw_extend_seed_batch_device: a seed in the middle of a read extended both ways and joined into one alignment
// (the definition is tests/seed_extend_textbook.py's).  The output record, the staging of a chunk of pairs and the
// two kernels around the extension kernels, shared by sw_seed_extend.hip and the host side (sw_seed_extend.cpp).
//
// A chunk of m pairs is staged in the context's workspace, in front of the extension kernels' slots:
//   the reversed left flanks    m rows of tstride bytes (target) and m of qstride (query), the flank at the row's start
//   the descriptors             per side and sequence an int64 start and an int32 length, laid out as the arrays a SeqSet points to: the
//                               left starts are offsets into the reversed copies, the right starts offsets into the caller's arrays (the
//                               right flanks are not copied).  A side with an empty flank, and both sides of an invalid pair, get
//                               length 0 twice: the extension kernel answers that with a zero record and touches nothing else.
//                               `flank` keeps what the lengths really are, {left t, left q, right t, right q}, or -1 four times for an
//                               invalid pair: the join knows an empty or invalid side from there, not from the extension's status
//   the sides' outputs          per side an Extension, a status, a CIGAR length and a BINARY CIGAR row of istride bytes (no rows when
//                               score-only)
//
// istride: a side must not overflow its internal row when the joined CIGAR would have fit the caller's.  The join merges at most the
// seed into a side's nearest element, so the joined CIGAR has at least as many elements as either side.  A joined text of
// cigar_stride bytes holds at most cigar_stride / 2 elements (a digit and a letter each), a binary one cigar_stride / 4; and a side of a
// pair within (max_tl, max_ql) has at most max_tl + max_ql elements, each spending a base.  The smaller of the two counts, times four
// bytes, is the row: a side that overflows it has more elements than the caller's row could hold joined.
#ifndef MGL_SW_SEED_EXTEND_H
#define MGL_SW_SEED_EXTEND_H

#include "sw_extend.h"

namespace mgl_sw_dev {

// the most pairs in a chunk: the split and the join run one workgroup of one wave per pair, and a grid has fewer than 2^31 of them
constexpr int64_t SEED_MAX_CHUNK = 1 << 30;

struct SeedAlignment { // == mgl_sw_seed_alignment
    int32_t score, t_beg, t_end, q_beg, q_end, seed_score, dropped, cigar_from;
};
static_assert(sizeof(SeedAlignment) == 32, "mgl_sw_seed_alignment is eight int32");

__host__ __device__ inline int64_t seed_round(int64_t bytes, int64_t to) { return (bytes + to - 1) / to * to; }
// (the lengths are capped at BANDED_MAX_LEN: no pair beyond passes a side's range guard)
__host__ __device__ inline int64_t seed_flank_stride(int max_len) { return seed_round(max_len < BANDED_MAX_LEN ? max_len : BANDED_MAX_LEN, 64); }
__host__ __device__ inline int64_t seed_side_cigar_stride(int max_tl, int max_ql, int cigar_stride, bool binary, bool score_only)
{
    if (score_only) return 0;
    const int64_t geom = (int64_t)(max_tl < BANDED_MAX_LEN ? max_tl : BANDED_MAX_LEN) + (max_ql < BANDED_MAX_LEN ? max_ql : BANDED_MAX_LEN);
    const int64_t out = binary ? cigar_stride / 4 : cigar_stride / 2;
    const int64_t el = out < geom ? out : geom;
    return 4 * (el < 1 ? 1 : el < (1 << 29) ? el : (1 << 29) - 1); // (an int, as every cigar_stride: 2^29 elements need both bounds at 2^28)
}

// where the parts of a chunk of m pairs stand, from the workspace's start; every part begins on a multiple of 256
struct SeedStaging {
    int64_t tstride, qstride, istride;
    int64_t rev_t, rev_q;                  // reversed left flanks
    int64_t off[4], len[4], flank;         // descriptors: {left t, left q, right t, right q}; flank: int4 per pair
    int64_t ext[2], status[2], clen[2], cigar[2]; // the sides' outputs: {left, right}
    int64_t bytes;
};
__host__ inline SeedStaging seed_staging(int64_t m, int max_tl, int max_ql, int cigar_stride, bool binary, bool score_only)
{
    SeedStaging s{};
    s.tstride = seed_flank_stride(max_tl);
    s.qstride = seed_flank_stride(max_ql);
    s.istride = seed_side_cigar_stride(max_tl, max_ql, cigar_stride, binary, score_only);
    int64_t at = 0;
    auto part = [&](int64_t bytes) {
        const int64_t here = at;
        at += seed_round(bytes, 256);
        return here;
    };
    s.rev_t = part(m * s.tstride);
    s.rev_q = part(m * s.qstride);
    for (int x = 0; x < 4; ++x) s.off[x] = part(m * 8);
    for (int x = 0; x < 4; ++x) s.len[x] = part(m * 4);
    s.flank = part(m * 16);
    for (int x = 0; x < 2; ++x) {
        s.ext[x] = part(m * (int64_t)sizeof(Extension));
        s.status[x] = part(m * 4);
        s.clen[x] = part(m * 4);
        s.cigar[x] = part(m * s.istride);
    }
    s.bytes = at;
    return s;
}
// what one more pair adds to every part, and the number of parts: seed_staging(m).bytes is at least m times the first and less than
// that plus 256 bytes of rounding per part
constexpr int SEED_STAGING_PARTS = 2 + 4 + 4 + 1 + 2 * 4;
__host__ inline int64_t seed_staging_pair_bytes(const SeedStaging &s) { return s.tstride + s.qstride + 4 * 8 + 4 * 4 + 16 + 2 * ((int64_t)sizeof(Extension) + 4 + 4 + s.istride); }

struct SeedArgs {
    const uint8_t *targets, *queries;              // the caller's, with the chunk's start, length and seed arrays
    const int64_t *t_start, *q_start;
    const int32_t *t_len, *q_len, *seed_t, *seed_q, *seed_len;
    int64_t n;                                     // the chunk's pairs
    int max_tl, max_ql;
    int match, mismatch;                           // normalised
    // ---- staging (see above)
    uint8_t *rev_t, *rev_q;
    int64_t tstride, qstride;
    int64_t *off[4];
    int32_t *len[4];
    int4 *flank;
    const Extension *side_ext[2];
    const int32_t *side_status[2], *side_clen[2];
    const uint32_t *side_cigar[2];                 // binary rows of istride bytes; null when score_only
    int64_t istride;
    // ---- the caller's outputs, at the chunk's start
    SeedAlignment *aln;
    Extension *left_out, *right_out;               // optional
    char *cigar;                                   // not score_only
    int cigar_stride;
    int32_t *cigar_len;                            // optional when score_only
    int32_t *status;                               // optional
    int binary_cigar, score_only;
};

hipError_t launch_seed_split(const SeedArgs &a, hipStream_t stream);
hipError_t launch_seed_join(const SeedArgs &a, hipStream_t stream);

} // namespace mgl_sw_dev

#endif
