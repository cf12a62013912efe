// sw_rank.cpp -- mgl_sw_rank_chains_batch_device (include/mgl_sw.h): the chain stage's f and pred in, the best max_chains chains of
// every read out, ranked, with parents and mapping qualities.  Host side only: argument checks, one workspace
// (the reads' anchor counts and, where the anchor outputs are wanted, the staging of the chains) and one launch on the caller's
// stream -- sw_rank_chains_kernel -- or three: the chain stage's own prefix sum (launch_chain_dp_scan, as it is) and
// sw_rank_pack_kernel behind it.  No synchronisation.  The entry's frame is sw_stage_host.h's.
#include "../../include/mgl_sw.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "sw_chain_dp.h"
#include "sw_rank.h"
#include "sw_stage_host.h"

using namespace mgl_sw_dev;
using namespace mgl_sw_host;

static_assert(sizeof(mgl_sw_ranked_chain) == 48, "twelve int32");

extern "C" {

int mgl_sw_rank_chains_batch_device(mgl_sw_ctx *ctx, void *stream, int64_t n, int strands, const int32_t *d_row_q_len, const int64_t *d_cand_start,
                                    const int32_t *d_cand_t, const int32_t *d_cand_q, const int32_t *d_cand_len, int64_t total_cand, const int32_t *d_f,
                                    const int32_t *d_pred, const int32_t *d_row_status, int max_cand, int max_chains, int min_score, int min_cnt,
                                    int mask_level, int32_t *d_n_chains_out, mgl_sw_ranked_chain *d_records_out, int64_t *d_ranked_start_out,
                                    int32_t *d_ranked_t_out, int32_t *d_ranked_q_out, int32_t *d_ranked_len_out, int32_t *d_status_out)
{
    // ---- arguments first: nothing below touches a device before they are known good
    const int wanted = (d_ranked_start_out != nullptr) + (d_ranked_t_out != nullptr) + (d_ranked_q_out != nullptr) + (d_ranked_len_out != nullptr);
    const char *bad = nullptr;
    if (n < 0 || total_cand < 0) bad = "n < 0 or total_cand < 0";
    else if (strands != 1 && strands != 2) bad = "strands outside 1, 2";
    else if (n > RANK_MAX_CHUNK / strands || total_cand > RANK_MAX_CHUNK) bad = "more than 2^30 rows or candidates";
    else if (!d_row_q_len || !d_cand_start || !d_cand_t || !d_cand_q || !d_cand_len) bad = "null row or candidate array";
    else if (!d_f || !d_pred) bad = "null f or pred";
    else if (!d_n_chains_out || !d_records_out) bad = "null d_n_chains_out or d_records_out";
    else if (wanted != 0 && wanted != 4) bad = "the four anchor outputs go together: all or none";
    else if (max_cand < 0 || max_cand > RANK_MAX_CAND) bad = "max_cand outside 0 .. 8192";
    else if (max_chains < 1 || max_chains > RANK_MAX_CHAINS) bad = "max_chains outside 1 .. 16";
    else if (min_score < 1 || min_cnt < 1) bad = "min_score or min_cnt < 1";
    else if (mask_level < 1 || mask_level > 256) bad = "mask_level outside 1 .. 256";
    if (bad) return refuse(ctx, "mgl_sw_rank_chains_batch_device", bad);
    if (!ctx) return no_context();
    // there is no kernel id for this stage: the timing record keeps the fill_kernel it has (Stage's default)
    Stage stage(ctx, stream);
    hipStream_t st = stage.st;
    const bool anchors = wanted == 4;

    // ---- one workspace: the counts and, for the anchor outputs, the staging of the whole batch
    const int64_t limit = stage.limit();
    const RankWorkspace wk = rank_workspace(n, total_cand, anchors);
    if (wk.bytes > limit)
        return ctx_fail(ctx, MGL_SW_ERR_NOMEM, "mgl_sw_rank_chains_batch_device: the workspace limit does not hold the batch's counts and staging: split the batch");
    unsigned char *ws = nullptr;
    const int rc = stage.borrow((size_t)std::max<int64_t>(wk.bytes, 256), &ws);
    if (rc != MGL_SW_OK) return rc;

    RankArgs a{};
    a.row_q_len = d_row_q_len;
    a.cand_start = d_cand_start;
    a.cand_t = d_cand_t;
    a.cand_q = d_cand_q;
    a.cand_len = d_cand_len;
    a.f = d_f;
    a.pred = d_pred;
    a.row_status = d_row_status;
    a.n = n;
    a.total_cand = total_cand;
    a.strands = strands;
    a.max_cand = max_cand;
    a.max_chains = max_chains;
    a.min_score = min_score;
    a.min_cnt = min_cnt;
    a.mask_level = mask_level;
    // the LDS of the small form leaves room for two workgroups on a CU, that of the large form for one (sw_rank.hip)
    a.groups = (int)std::min<int64_t>(std::max<int64_t>(n, 1), (int64_t)ctx_cus(ctx) * (max_cand <= RANK_CAP_SMALL ? 2 : 1));
    a.count = reinterpret_cast<int32_t *>(ws + wk.count);
    a.stage = anchors ? reinterpret_cast<int32_t *>(ws + wk.stage) : nullptr;
    a.n_chains = d_n_chains_out;
    a.records = d_records_out;
    a.ranked_start = d_ranked_start_out;
    a.ranked_t = d_ranked_t_out;
    a.ranked_q = d_ranked_q_out;
    a.ranked_len = d_ranked_len_out;
    a.status = d_status_out;

    hipError_t he = launch_rank_chains(a, st);
    if (he != hipSuccess) return stage.fail(he, "launch_rank_chains");
    if (anchors) {
        ChainDpArgs scan{}; // the chain stage's prefix sum reads count and n and writes chain_start, nothing else
        scan.n = n;
        scan.count = a.count;
        scan.chain_start = d_ranked_start_out;
        he = launch_chain_dp_scan(scan, st);
        if (he != hipSuccess) return stage.fail(he, "launch_chain_dp_scan");
        he = launch_rank_pack(a, st);
        if (he != hipSuccess) return stage.fail(he, "launch_rank_pack");
    }
    return stage.done();
}

} // extern "C"
