// sw_banded.cpp -- mgl_sw_align_batch_device_banded (include/mgl_sw.h): the GATK function over a diagonal band.  Host side only: argument
// checks and the launch of sw_banded_kernel (sw_banded.hip) on workspace slots (sw_band_host.h).  The entry's frame is sw_stage_host.h's.
#include "../../include/mgl_sw.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "sw_band_host.h"

using namespace mgl_sw_dev;

using namespace mgl_sw_host;

extern "C" {

int mgl_sw_align_batch_device_banded(mgl_sw_ctx *ctx, void *stream, int64_t n, const uint8_t *d_targets, const int64_t *d_t_start,
                                     const int32_t *d_t_len, const uint8_t *d_queries, const int64_t *d_q_start, const int32_t *d_q_len,
                                     int max_tl, int max_ql, int match, int mismatch, int gopen, int gext, int strategy, int band,
                                     int32_t *d_offset_out, mgl_sw_score *d_score_out, char *d_cigar_out, int cigar_stride,
                                     int32_t *d_cigar_len_out, int32_t *d_status_out, int flags)
{
    const bool score_only = (flags & MGL_SW_FLAG_SCORE_ONLY) != 0, binary = (flags & MGL_SW_FLAG_BINARY_CIGAR) != 0;
    // ---- arguments first: nothing below touches a device before they are known good
    const char *bad = nullptr;
    if (n < 0) bad = "n < 0";
    else if (!d_targets || !d_t_start || !d_t_len || !d_queries || !d_q_start || !d_q_len) bad = "null sequence, start or length array";
    else if (!d_offset_out) bad = "null offset array";
    else if (band < 0) bad = "band < 0";
    else if (strategy != MGL_SW_OS_SOFTCLIP && strategy != MGL_SW_OS_INDEL && strategy != MGL_SW_OS_LEAD_ID && strategy != MGL_SW_OS_IGNORE) bad = "unknown overhang strategy";
    else if (max_tl < 1 || max_ql < 1) bad = "max_tl / max_ql < 1";
    else if (score_only && !d_score_out) bad = "MGL_SW_FLAG_SCORE_ONLY without a score array";
    else if (!score_only && (!d_cigar_out || !d_cigar_len_out || cigar_stride < (binary ? 4 : 2))) bad = "CIGAR array missing or cigar_stride too small";
    if (bad) return refuse(ctx, "mgl_sw_align_batch_device_banded", bad);
    if (!ctx) return no_context();
    Stage stage(ctx, stream);
    if (n == 0) return MGL_SW_OK;
    mgl_sw_normalize_params(&match, &mismatch, &gopen, &gext);

    BandedArgs a{};
    a.t = SeqSet{d_targets, d_t_start, d_t_len, max_tl, 0};
    a.q = SeqSet{d_queries, d_q_start, d_q_len, max_ql, 0};
    a.n = n;
    a.match = match;
    a.mismatch = mismatch;
    a.gopen = gopen;
    a.gext = gext;
    a.strategy = strategy;
    a.band = clamp_band(band, max_tl, max_ql);
    a.max_tl = max_tl;
    a.max_ql = max_ql;
    a.offset = d_offset_out;
    a.score = reinterpret_cast<Score *>(d_score_out);
    a.status = d_status_out;
    a.cigar = d_cigar_out;
    a.cigar_stride = cigar_stride;
    a.cigar_len = d_cigar_len_out;
    a.binary_cigar = binary ? 1 : 0;
    a.score_only = score_only ? 1 : 0;
    // ---- the slots are sized for the largest pair the bounds admit
    return launch_on_slots(stage, a, banded_slot_bound(std::min(max_tl, BANDED_MAX_LEN), std::min(max_ql, BANDED_MAX_LEN), a.band, score_only), launch_banded,
                           "launch_banded", MGL_SW_KERNEL_BANDED);
}

} // extern "C"
