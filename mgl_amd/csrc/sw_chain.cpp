// sw_chain.cpp -- mgl_sw_align_chain_batch_device (include/mgl_sw.h): a chain of anchors, its two sides extended, its gaps filled and all
// of it joined into one alignment.  Host side only: argument checks, one workspace for the staging of the whole
// batch and the slots, and five launches on the caller's stream -- sw_chain_split_kernel, the extension kernel over the left flanks and
// over the right ones (sw_extend.hip or sw_extend_adaptive.hip, as they are), sw_gap_fill_kernel, sw_chain_join_kernel -- behind two
// memsets (the gap descriptors, d_gap_score_out).  No synchronisation.  The entry's frame is sw_stage_host.h's, the two sides'
// extension sw_band_host.h's.
#include "../../include/mgl_sw.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "sw_band_host.h"
#include "sw_chain.h"

using namespace mgl_sw_dev;

static_assert(sizeof(mgl_sw_chain_alignment) == sizeof(ChainAlignment), "mgl_sw_chain_alignment and the kernel's record are one layout");

using namespace mgl_sw_host;

extern "C" {

int mgl_sw_align_chain_batch_device(mgl_sw_ctx *ctx, void *stream, int64_t n, const uint8_t *d_targets, const int64_t *d_t_start,
                                    const int32_t *d_t_len, const uint8_t *d_queries, const int64_t *d_q_start, const int32_t *d_q_len,
                                    const int64_t *d_anchor_start, const int32_t *d_anchor_t, const int32_t *d_anchor_q, const int32_t *d_anchor_len,
                                    int64_t total_anchors, int max_tl, int max_ql, int max_gap_tl, int max_gap_ql, int match, int mismatch, int gopen,
                                    int gext, int band, int zdrop, mgl_sw_chain_alignment *d_aln_out, mgl_sw_extension *d_left_out,
                                    mgl_sw_extension *d_right_out, int32_t *d_gap_score_out, char *d_cigar_out, int cigar_stride,
                                    int32_t *d_cigar_len_out, int32_t *d_status_out, int flags)
{
    const bool score_only = (flags & MGL_SW_FLAG_SCORE_ONLY) != 0, binary = (flags & MGL_SW_FLAG_BINARY_CIGAR) != 0;
    // ---- arguments first: nothing below touches a device before they are known good
    const char *bad = nullptr;
    if (n < 0) bad = "n < 0";
    else if (!d_targets || !d_t_start || !d_t_len || !d_queries || !d_q_start || !d_q_len) bad = "null sequence, start or length array";
    else if (!d_anchor_start || !d_anchor_t || !d_anchor_q || !d_anchor_len) bad = "null anchor array";
    else if (total_anchors < 0) bad = "total_anchors < 0";
    else if (n > SEED_MAX_CHUNK || total_anchors > SEED_MAX_CHUNK) bad = "more than 2^30 pairs or anchors";
    else if (!d_aln_out) bad = "null alignment array";
    else if (band < 0) bad = "band < 0";
    else if (max_tl < 1 || max_ql < 1) bad = "max_tl / max_ql < 1";
    else if (max_gap_tl < 0 || max_gap_ql < 0) bad = "max_gap_tl / max_gap_ql < 0";
    else if (!score_only && (!d_cigar_out || !d_cigar_len_out || cigar_stride < (binary ? 4 : 2))) bad = "CIGAR array missing or cigar_stride too small";
    if (bad) return refuse(ctx, "mgl_sw_align_chain_batch_device", bad);
    if (!ctx) return no_context();
    Stage stage(ctx, stream);
    if (n == 0) return MGL_SW_OK;
    mgl_sw_normalize_params(&match, &mismatch, &gopen, &gext);
    hipStream_t st = stage.st;
    // a gap bound of 0: no gap with bases on both sides is admitted, and a slot for a 1 x 1 gap is what stands there
    const int gap_tl = std::min(std::max(max_gap_tl, 1), BANDED_MAX_LEN), gap_ql = std::min(std::max(max_gap_ql, 1), BANDED_MAX_LEN);

    // ---- the extension of one side (sw_band_host.h)
    ExtendArgs e{};
    const int64_t ext_bound = extend_sides_setup(stage, e, match, mismatch, gopen, gext, flags, band, zdrop, max_tl, max_ql);
    // ---- the fill of a gap: the banded entry's band clamp and slot bound (sw_banded.cpp), at the gap bounds
    const int fill_band = clamp_band(band, gap_tl, gap_ql);
    const int64_t fill_bound = banded_slot_bound(gap_tl, gap_ql, fill_band, score_only);

    // ---- one workspace: the staging of the whole batch, then the slots.  The extension launches and the fill follow one another on
    // the stream, so their slots share one region: each kind is cut from it at its own size, and a kind whose bound the region does
    // not hold gets one slot of all there is (a segment that does not fit its slot: MGL_SW_ERR_UNSUPPORTED)
    const int64_t limit = stage.limit();
    const ChainStaging sg = chain_staging(n, total_anchors, max_tl, max_ql, gap_tl, gap_ql, cigar_stride, binary, score_only);
    const int64_t room = limit - sg.bytes;
    if (room < 256)
        return ctx_fail(ctx, MGL_SW_ERR_NOMEM, "mgl_sw_align_chain_batch_device: the workspace limit does not hold the batch's staging beside a slot: split the batch");
    const int64_t ext_slot = std::min(ext_bound, room), fill_slot = std::min(fill_bound, room);
    const int64_t most = (int64_t)ctx_cus(ctx) * BANDED_WAVES_PER_CU;
    const int64_t ext_waves = std::max<int64_t>(1, std::min<int64_t>({n, most, room / ext_slot}));
    const int64_t fill_waves = std::max<int64_t>(1, std::min<int64_t>({std::max<int64_t>(total_anchors, 1), most, room / fill_slot}));
    unsigned char *ws = nullptr;
    const int rc = stage.borrow((size_t)(sg.bytes + std::max(ext_waves * ext_slot, fill_waves * fill_slot)), &ws);
    if (rc != MGL_SW_OK) return rc;
    e.ws = ws + sg.bytes;
    e.slot_bytes = ext_slot;
    e.slots = (int)ext_waves;
    e.cigar_stride = (int)sg.pair.istride;
    e.n = n;

    ChainArgs s{};
    s.targets = d_targets;
    s.queries = d_queries;
    s.t_start = d_t_start;
    s.q_start = d_q_start;
    s.t_len = d_t_len;
    s.q_len = d_q_len;
    s.anchor_start = d_anchor_start;
    s.anchor_t = d_anchor_t;
    s.anchor_q = d_anchor_q;
    s.anchor_len = d_anchor_len;
    s.n = n;
    s.total_anchors = total_anchors;
    s.max_tl = max_tl;
    s.max_ql = max_ql;
    s.max_gap_tl = max_gap_tl;
    s.max_gap_ql = max_gap_ql;
    s.match = match;
    s.mismatch = mismatch;
    s.gopen = gopen;
    s.gext = gext;
    s.band = fill_band;
    bind_seed_staging(s, ws, sg.pair, score_only);
    s.pstat = reinterpret_cast<int32_t *>(ws + sg.pstat);
    s.owner = reinterpret_cast<int32_t *>(ws + sg.owner);
    s.gscore = reinterpret_cast<int32_t *>(ws + sg.gscore);
    s.gstatus = reinterpret_cast<int32_t *>(ws + sg.gstatus);
    s.gclen = reinterpret_cast<int32_t *>(ws + sg.gclen);
    s.grow = score_only ? nullptr : reinterpret_cast<uint32_t *>(ws + sg.grow);
    s.gstride = sg.gstride;
    s.ws = ws + sg.bytes;
    s.slot_bytes = fill_slot;
    s.slots = (int)fill_waves;
    s.aln = reinterpret_cast<ChainAlignment *>(d_aln_out);
    s.left_out = reinterpret_cast<Extension *>(d_left_out);
    s.right_out = reinterpret_cast<Extension *>(d_right_out);
    s.gap_score_out = d_gap_score_out;
    s.cigar = d_cigar_out;
    s.cigar_stride = cigar_stride;
    s.cigar_len = d_cigar_len_out;
    s.status = d_status_out;
    s.binary_cigar = binary ? 1 : 0;
    s.score_only = score_only ? 1 : 0;

    hipError_t he = hipSuccess;
    if (total_anchors > 0) he = hipMemsetAsync(s.owner, CHAIN_NO_OWNER & 0xff, (size_t)total_anchors * 4, st); // every anchor unclaimed
    if (he != hipSuccess) return stage.fail(he, "hipMemsetAsync(gap descriptors)");
    if (d_gap_score_out && total_anchors > 0) he = hipMemsetAsync(d_gap_score_out, 0, (size_t)total_anchors * 4, st);
    if (he != hipSuccess) return stage.fail(he, "hipMemsetAsync(d_gap_score_out)");
    he = launch_chain_split(s, st);
    if (he != hipSuccess) return stage.fail(he, "launch_chain_split");
    const int src = launch_extend_sides(stage, e, s, ws, sg.pair);
    if (src != MGL_SW_OK) return src;
    he = launch_gap_fill(s, st);
    if (he != hipSuccess) return stage.fail(he, "launch_gap_fill");
    ++stage.launches;
    he = launch_chain_join(s, st);
    if (he != hipSuccess) return stage.fail(he, "launch_chain_join");
    return stage.done();
}

} // extern "C"
