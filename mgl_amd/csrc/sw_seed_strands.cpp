// sw_seed_strands.cpp -- mgl_sw_seed_strands_batch_device and mgl_sw_select_strand_batch_device (include/mgl_sw.h): the seed stage over
// both orientations of every read, as 2n rows for mgl_sw_chain_anchors_batch_device, and the choice of a read's strand behind that
// stage, as arguments for mgl_sw_align_chain_batch_device.  Host side only: argument checks, one workspace and
// three launches on the caller's stream each.  No synchronisation.  The entries' frame is sw_stage_host.h's.
#include "../../include/mgl_sw.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "sw_seed_strands.h"
#include "sw_stage_host.h"

using namespace mgl_sw_dev;
using namespace mgl_sw_host;

extern "C" {

int mgl_sw_seed_strands_batch_device(mgl_sw_ctx *ctx, void *stream, int64_t n, const uint8_t *d_targets, const int64_t *d_t_start,
                                     const int32_t *d_t_len, const uint8_t *d_queries, const int64_t *d_q_start, const int32_t *d_q_len, int k, int w,
                                     int max_occ, int merge, int max_cand, int64_t cand_capacity, int64_t *d_cand_start_out, int32_t *d_cand_t_out,
                                     int32_t *d_cand_q_out, int32_t *d_cand_len_out, int32_t *d_row_t_len_out, int32_t *d_row_q_len_out,
                                     int32_t *d_status_out)
{
    // ---- arguments first: nothing below touches a device before they are known good
    const char *bad = nullptr;
    if (n < 0 || n > STRAND_MAX_PAIRS) bad = "n outside 0 .. 2^29";
    else if (!d_targets || !d_t_start || !d_t_len) bad = "null target array";
    else if (!d_queries || !d_q_start || !d_q_len) bad = "null query array";
    else if (!d_cand_start_out || !d_cand_t_out || !d_cand_q_out || !d_cand_len_out) bad = "null candidate array";
    else if (k < SEED_MIN_K || k > SEED_MAX_K) bad = "k outside 4 .. 16";
    else if (w < 1 || w > SEED_MAX_W) bad = "w outside 1 .. 32";
    else if (max_occ < 1 || max_occ > SEED_MAX_OCC) bad = "max_occ outside 1 .. 64";
    else if (merge != 0 && merge != 1) bad = "merge is neither 0 nor 1";
    else if (max_cand < 1 || max_cand > SEED_MAX_CAND) bad = "max_cand outside 1 .. 8192";
    else if (cand_capacity < 0 || cand_capacity > SEED_MAX_PAIRS) bad = "cand_capacity outside 0 .. 2^30";
    if (bad) return refuse(ctx, "mgl_sw_seed_strands_batch_device", bad);
    if (!ctx) return no_context();
    // there is no kernel id for this stage: the timing record keeps the fill_kernel it has (Stage's default)
    Stage stage(ctx, stream);
    hipStream_t st = stage.st;

    // ---- one workspace: the counts and the staging of the 2n rows, then one slot of two halves per workgroup
    const int64_t rows = 2 * n;
    const int64_t limit = stage.limit();
    const SeedWorkspace sg = seed_workspace(rows, max_cand);
    const int64_t slot_bytes = 2 * (int64_t)sg.slot_bytes, room = limit - sg.bytes;
    if (room < slot_bytes)
        return ctx_fail(ctx, MGL_SW_ERR_NOMEM,
                        "mgl_sw_seed_strands_batch_device: the workspace limit does not hold the staging of the batch's 2n rows beside a slot: split the batch");
    const int64_t groups = std::min(std::min<int64_t>(std::max<int64_t>(n, 1), (int64_t)ctx_cus(ctx) * SEED_GROUPS_PER_CU), room / slot_bytes);
    unsigned char *ws = nullptr;
    const int rc = stage.borrow((size_t)(sg.bytes + groups * slot_bytes), &ws);
    if (rc != MGL_SW_OK) return rc;

    SeedStrandsArgs aa{};
    SeedStageArgs &a = aa.s;
    a.targets = d_targets;
    a.queries = d_queries;
    a.t_start = d_t_start;
    a.q_start = d_q_start;
    a.t_len = d_t_len;
    a.q_len = d_q_len;
    a.n = rows;
    a.cand_capacity = cand_capacity;
    a.k = k;
    a.w = w;
    a.max_occ = max_occ;
    a.merge = merge;
    a.max_cand = max_cand;
    a.ws = ws;
    a.groups = (int)groups;
    a.cand_start = d_cand_start_out;
    a.cand_t = d_cand_t_out;
    a.cand_q = d_cand_q_out;
    a.cand_len = d_cand_len_out;
    a.status = d_status_out;
    aa.row_t_len = d_row_t_len_out;
    aa.row_q_len = d_row_q_len_out;

    hipError_t he = launch_seed_strands(aa, st);
    if (he != hipSuccess) return stage.fail(he, "launch_seed_strands");
    // the scan and the pack of the seed stage read nothing but the rows' counts and staging: they serve the 2n rows as they are
    he = launch_seed_scan(a, st);
    if (he != hipSuccess) return stage.fail(he, "launch_seed_scan");
    he = launch_seed_pack(a, st);
    if (he != hipSuccess) return stage.fail(he, "launch_seed_pack");
    return stage.done();
}

int mgl_sw_select_strand_batch_device(mgl_sw_ctx *ctx, void *stream, int64_t n, const uint8_t *d_queries, const int64_t *d_q_start,
                                      const int32_t *d_q_len, const int64_t *d_chain_start, const int32_t *d_chain_t, const int32_t *d_chain_q,
                                      const int32_t *d_chain_len, const int32_t *d_chain_score, int64_t total_chain, int64_t query_bytes,
                                      int32_t *d_strand_out, uint8_t *d_queries_out, int64_t *d_anchor_start_out, int32_t *d_anchor_t_out,
                                      int32_t *d_anchor_q_out, int32_t *d_anchor_len_out, int32_t *d_score_out, int32_t *d_status_out)
{
    const char *bad = nullptr;
    if (n < 0 || n > STRAND_MAX_PAIRS) bad = "n outside 0 .. 2^29";
    else if (!d_queries || !d_q_start || !d_q_len) bad = "null query array";
    else if (!d_chain_start || !d_chain_t || !d_chain_q || !d_chain_len || !d_chain_score) bad = "null chain array";
    else if (total_chain < 0 || total_chain > SEED_MAX_PAIRS) bad = "total_chain outside 0 .. 2^30";
    else if (query_bytes < 0) bad = "query_bytes below 0";
    else if (!d_strand_out || !d_queries_out) bad = "null strand or query output";
    else if (!d_anchor_start_out || !d_anchor_t_out || !d_anchor_q_out || !d_anchor_len_out) bad = "null anchor array";
    if (bad) return refuse(ctx, "mgl_sw_select_strand_batch_device", bad);
    if (!ctx) return no_context();
    Stage stage(ctx, stream);
    hipStream_t st = stage.st;

    // ---- the workspace: K_p per pair
    const int64_t limit = stage.limit();
    const int64_t bytes = seed_ws_round(std::max<int64_t>(n, 1) * 4, 256);
    if (bytes > limit) return ctx_fail(ctx, MGL_SW_ERR_NOMEM, "mgl_sw_select_strand_batch_device: the workspace limit does not hold 4 bytes per pair");
    unsigned char *ws = nullptr;
    const int rc = stage.borrow((size_t)bytes, &ws);
    if (rc != MGL_SW_OK) return rc;

    SelectStrandArgs a{};
    a.queries = d_queries;
    a.q_start = d_q_start;
    a.q_len = d_q_len;
    a.chain_start = d_chain_start;
    a.chain_t = d_chain_t;
    a.chain_q = d_chain_q;
    a.chain_len = d_chain_len;
    a.chain_score = d_chain_score;
    a.n = n;
    a.total_chain = total_chain;
    a.query_bytes = query_bytes;
    a.count = reinterpret_cast<int32_t *>(ws);
    a.strand = d_strand_out;
    a.queries_out = d_queries_out;
    a.anchor_start = d_anchor_start_out;
    a.anchor_t = d_anchor_t_out;
    a.anchor_q = d_anchor_q_out;
    a.anchor_len = d_anchor_len_out;
    a.score = d_score_out;
    a.status = d_status_out;

    hipError_t he = launch_select_strand(a, st);
    if (he != hipSuccess) return stage.fail(he, "launch_select_strand");
    he = launch_select_strand_scan(a, st);
    if (he != hipSuccess) return stage.fail(he, "launch_select_strand_scan");
    he = launch_select_strand_pack(a, st);
    if (he != hipSuccess) return stage.fail(he, "launch_select_strand_pack");
    return stage.done();
}

} // extern "C"
