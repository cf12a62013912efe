// sw_chain_dp.cpp -- mgl_sw_chain_anchors_batch_device and mgl_sw_chain_anchors_grouped_batch_device (include/mgl_sw.h): candidate anchors in, the best colinear chain of every read
// out, in the CSR layout mgl_sw_align_chain_batch_device reads.  Host side only: argument checks, one workspace
// (the counts, the staging of the chains, and pred slots where max_cand is above what a wave keeps in LDS) and three launches on the
// caller's stream -- sw_chain_dp_kernel, sw_chain_dp_scan_kernel, sw_chain_dp_pack_kernel.  No synchronisation.  The entry's frame is
// sw_stage_host.h's.
#include "../../include/mgl_sw.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "sw_chain_dp.h"
#include "sw_stage_host.h"

using namespace mgl_sw_dev;
using namespace mgl_sw_host;

namespace {

// both entries: `grouped` says whether d_cand_group is required (and then sw_chain_dp_kernel<true> runs)
int chain_anchors(const char *entry, const bool grouped, mgl_sw_ctx *ctx, void *stream, int64_t n, const int32_t *d_t_len, const int32_t *d_q_len,
                  const int64_t *d_cand_start, const int32_t *d_cand_t, const int32_t *d_cand_q, const int32_t *d_cand_len, const int32_t *d_cand_group,
                  int64_t total_cand, int max_cand, int max_pred, int max_dist_t, int max_dist_q, int bw, int pen_gap, int pen_skip,
                  int64_t *d_chain_start_out, int32_t *d_chain_t_out, int32_t *d_chain_q_out, int32_t *d_chain_len_out, int32_t *d_chain_score_out,
                  int32_t *d_f_out, int32_t *d_pred_out, int32_t *d_status_out)
{
    // ---- arguments first: nothing below touches a device before they are known good
    const char *bad = nullptr;
    if (n < 0 || total_cand < 0) bad = "n < 0 or total_cand < 0";
    else if (n > CHAIN_DP_MAX_CHUNK || total_cand > CHAIN_DP_MAX_CHUNK) bad = "more than 2^30 reads or candidates";
    else if (!d_t_len || !d_q_len) bad = "null length array";
    else if (!d_cand_start || !d_cand_t || !d_cand_q || !d_cand_len) bad = "null candidate array";
    else if (grouped && !d_cand_group) bad = "null group array";
    else if (!d_chain_start_out || !d_chain_t_out || !d_chain_q_out || !d_chain_len_out || !d_chain_score_out) bad = "null chain array";
    else if (max_cand < 0) bad = "max_cand < 0";
    else if (max_pred < 1 || max_pred > CHAIN_DP_MAX_PRED) bad = "max_pred outside 1 .. 64";
    else if (max_dist_t < 0 || max_dist_q < 0 || bw < 0) bad = "max_dist_t, max_dist_q or bw < 0";
    else if (pen_gap < 0 || pen_skip < 0) bad = "pen_gap or pen_skip < 0";
    else if (!chain_dp_pen_ok(max_dist_t, max_dist_q, bw, pen_gap, pen_skip)) bad = "pen_gap * bw + pen_skip * min(max_dist_t, max_dist_q) >= 2^31";
    if (bad) return refuse(ctx, entry, bad);
    if (!ctx) return no_context();
    // there is no kernel id for this stage: the timing record keeps the fill_kernel it has (Stage's default)
    Stage stage(ctx, stream);
    hipStream_t st = stage.st;
    max_cand = (int)std::min<int64_t>(max_cand, total_cand); // (no read that passes the range check has more)

    // ---- one workspace: the counts and the staging of the whole batch, then one pred slot per wave where LDS does not hold pred
    const int64_t limit = stage.limit();
    const ChainDpStaging sg = chain_dp_staging(n, total_cand, max_cand);
    const int64_t room = limit - sg.bytes;
    if (room < std::max<int64_t>(sg.slot_bytes, 0) || room < 0)
        return ctx_fail(ctx, MGL_SW_ERR_NOMEM,
                        (std::string(entry) + ": the workspace limit does not hold the batch's staging beside a pred slot: split the batch").c_str());
    int64_t waves = std::min<int64_t>(std::max<int64_t>(n, 1), (int64_t)ctx_cus(ctx) * CHAIN_DP_WAVES_PER_CU);
    if (sg.slot_bytes > 0) waves = std::min(waves, room / sg.slot_bytes);
    unsigned char *ws = nullptr;
    const int rc = stage.borrow((size_t)(sg.bytes + waves * sg.slot_bytes), &ws);
    if (rc != MGL_SW_OK) return rc;

    ChainDpArgs a{};
    a.t_len = d_t_len;
    a.q_len = d_q_len;
    a.cand_start = d_cand_start;
    a.cand_t = d_cand_t;
    a.cand_q = d_cand_q;
    a.cand_len = d_cand_len;
    a.n = n;
    a.total_cand = total_cand;
    a.max_cand = max_cand;
    a.max_pred = max_pred;
    a.max_dist_t = max_dist_t;
    a.max_dist_q = max_dist_q;
    a.bw = bw;
    a.pen_gap = pen_gap;
    a.pen_skip = pen_skip;
    a.count = reinterpret_cast<int32_t *>(ws + sg.count);
    a.stage = reinterpret_cast<int32_t *>(ws + sg.stage);
    a.ws = sg.slot_bytes > 0 ? ws + sg.bytes : nullptr;
    a.slot_bytes = sg.slot_bytes;
    a.waves = (int)waves;
    a.lds_bytes = sg.lds_bytes;
    a.chain_start = d_chain_start_out;
    a.chain_t = d_chain_t_out;
    a.chain_q = d_chain_q_out;
    a.chain_len = d_chain_len_out;
    a.chain_score = d_chain_score_out;
    a.f_out = d_f_out;
    a.pred_out = d_pred_out;
    a.status = d_status_out;
    a.cand_group = grouped ? d_cand_group : nullptr;

    hipError_t he = launch_chain_dp(a, st);
    if (he != hipSuccess) return stage.fail(he, "launch_chain_dp");
    he = launch_chain_dp_scan(a, st);
    if (he != hipSuccess) return stage.fail(he, "launch_chain_dp_scan");
    he = launch_chain_dp_pack(a, st);
    if (he != hipSuccess) return stage.fail(he, "launch_chain_dp_pack");
    return stage.done();
}

} // namespace

extern "C" {

int mgl_sw_chain_anchors_batch_device(mgl_sw_ctx *ctx, void *stream, int64_t n, const int32_t *d_t_len, const int32_t *d_q_len,
                                      const int64_t *d_cand_start, const int32_t *d_cand_t, const int32_t *d_cand_q, const int32_t *d_cand_len,
                                      int64_t total_cand, int max_cand, int max_pred, int max_dist_t, int max_dist_q, int bw, int pen_gap, int pen_skip,
                                      int64_t *d_chain_start_out, int32_t *d_chain_t_out, int32_t *d_chain_q_out, int32_t *d_chain_len_out,
                                      int32_t *d_chain_score_out, int32_t *d_f_out, int32_t *d_pred_out, int32_t *d_status_out)
{
    return chain_anchors("mgl_sw_chain_anchors_batch_device", false, ctx, stream, n, d_t_len, d_q_len, d_cand_start, d_cand_t, d_cand_q, d_cand_len, nullptr,
                         total_cand, max_cand, max_pred, max_dist_t, max_dist_q, bw, pen_gap, pen_skip, d_chain_start_out, d_chain_t_out, d_chain_q_out,
                         d_chain_len_out, d_chain_score_out, d_f_out, d_pred_out, d_status_out);
}

int mgl_sw_chain_anchors_grouped_batch_device(mgl_sw_ctx *ctx, void *stream, int64_t n, const int32_t *d_t_len, const int32_t *d_q_len,
                                              const int64_t *d_cand_start, const int32_t *d_cand_t, const int32_t *d_cand_q, const int32_t *d_cand_len,
                                              const int32_t *d_cand_group, int64_t total_cand, int max_cand, int max_pred, int max_dist_t, int max_dist_q,
                                              int bw, int pen_gap, int pen_skip, int64_t *d_chain_start_out, int32_t *d_chain_t_out, int32_t *d_chain_q_out,
                                              int32_t *d_chain_len_out, int32_t *d_chain_score_out, int32_t *d_f_out, int32_t *d_pred_out,
                                              int32_t *d_status_out)
{
    return chain_anchors("mgl_sw_chain_anchors_grouped_batch_device", true, ctx, stream, n, d_t_len, d_q_len, d_cand_start, d_cand_t, d_cand_q, d_cand_len,
                         d_cand_group, total_cand, max_cand, max_pred, max_dist_t, max_dist_q, bw, pen_gap, pen_skip, d_chain_start_out, d_chain_t_out,
                         d_chain_q_out, d_chain_len_out, d_chain_score_out, d_f_out, d_pred_out, d_status_out);
}

} // extern "C"
