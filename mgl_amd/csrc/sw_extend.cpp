// sw_extend.cpp -- mgl_sw_extend_batch_device (include/mgl_sw.h): anchored extension with Z-drop over a band centred on the main
// diagonal, or -- MGL_SW_FLAG_EXTEND_ADAPTIVE_BAND -- re-centred every 64 rows.  Host side only: argument checks, the workspace slots and
// the launch of sw_extend_kernel (sw_extend.hip) or sw_extend_adaptive_kernel (sw_extend_adaptive.hip), as sw_band_host.h has them.
// The entry's frame is sw_stage_host.h's.
#include "../../include/mgl_sw.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "sw_band_host.h"
#include "sw_extend.h"

using namespace mgl_sw_dev;

static_assert(sizeof(mgl_sw_extension) == sizeof(Extension), "mgl_sw_extension and the kernel's record are one layout");
static_assert(MGL_SW_EXTEND_RECENTRE_ROWS == EXTEND_RECENTRE_ROWS, "the band is re-centred once per strip of the kernel");

using namespace mgl_sw_host;

extern "C" {

int mgl_sw_extend_batch_device(mgl_sw_ctx *ctx, void *stream, int64_t n, const uint8_t *d_targets, const int64_t *d_t_start,
                               const int32_t *d_t_len, const uint8_t *d_queries, const int64_t *d_q_start, const int32_t *d_q_len, int max_tl,
                               int max_ql, int match, int mismatch, int gopen, int gext, int band, int zdrop, mgl_sw_extension *d_ext_out,
                               char *d_cigar_out, int cigar_stride, int32_t *d_cigar_len_out, int32_t *d_status_out, int flags)
{
    const bool score_only = (flags & MGL_SW_FLAG_SCORE_ONLY) != 0, binary = (flags & MGL_SW_FLAG_BINARY_CIGAR) != 0;
    const bool adaptive = (flags & MGL_SW_FLAG_EXTEND_ADAPTIVE_BAND) != 0;
    // ---- arguments first: nothing below touches a device before they are known good
    const char *bad = nullptr;
    if (n < 0) bad = "n < 0";
    else if (!d_targets || !d_t_start || !d_t_len || !d_queries || !d_q_start || !d_q_len) bad = "null sequence, start or length array";
    else if (!d_ext_out) bad = "null extension array";
    else if (band < 0) bad = "band < 0";
    else if (max_tl < 1 || max_ql < 1) bad = "max_tl / max_ql < 1";
    else if (!score_only && (!d_cigar_out || !d_cigar_len_out || cigar_stride < (binary ? 4 : 2))) bad = "CIGAR array missing or cigar_stride too small";
    if (bad) return refuse(ctx, "mgl_sw_extend_batch_device", bad);
    if (!ctx) return no_context();
    Stage stage(ctx, stream);
    if (n == 0) return MGL_SW_OK;
    mgl_sw_normalize_params(&match, &mismatch, &gopen, &gext);

    ExtendArgs a{};
    a.t = SeqSet{d_targets, d_t_start, d_t_len, max_tl, 0};
    a.q = SeqSet{d_queries, d_q_start, d_q_len, max_ql, 0};
    a.n = n;
    a.match = match;
    a.mismatch = mismatch;
    a.gopen = gopen;
    a.gext = gext;
    a.band = clamp_extend_band(adaptive, band, max_tl, max_ql);
    a.zdrop = zdrop;
    a.max_tl = max_tl;
    a.max_ql = max_ql;
    a.ext = reinterpret_cast<Extension *>(d_ext_out);
    a.status = d_status_out;
    a.cigar = d_cigar_out;
    a.cigar_stride = cigar_stride;
    a.cigar_len = d_cigar_len_out;
    a.binary_cigar = binary ? 1 : 0;
    a.score_only = score_only ? 1 : 0;
    a.to_query_end = (flags & MGL_SW_FLAG_EXTEND_TO_QUERY_END) ? 1 : 0;
    // ---- the slots are sized for the largest pair the bounds admit
    const int64_t slot_bound = extend_slot_bound(adaptive, max_tl, max_ql, a.band, score_only);
    if (adaptive) return launch_on_slots(stage, a, slot_bound, launch_extend_adaptive, "launch_extend_adaptive", MGL_SW_KERNEL_EXTEND_ADAPTIVE);
    return launch_on_slots(stage, a, slot_bound, launch_extend, "launch_extend", MGL_SW_KERNEL_EXTEND);
}

} // extern "C"
