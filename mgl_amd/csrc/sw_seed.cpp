// sw_seed.cpp -- mgl_sw_seed_batch_device (include/mgl_sw.h): reads and their windows in, candidate anchors out, in the CSR layout
// mgl_sw_chain_anchors_batch_device reads.  Host side only: argument checks, one workspace (the counts, the staging
// of the candidates, and one slot per workgroup for what outgrows its LDS) and three launches on the caller's stream -- sw_seed_kernel,
// sw_seed_scan_kernel, sw_seed_pack_kernel.  No synchronisation.  The entry's frame is sw_stage_host.h's.
#include "../../include/mgl_sw.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "sw_seed.h"
#include "sw_stage_host.h"

using namespace mgl_sw_dev;
using namespace mgl_sw_host;

extern "C" {

int mgl_sw_seed_batch_device(mgl_sw_ctx *ctx, void *stream, int64_t n, const uint8_t *d_targets, const int64_t *d_t_start, const int32_t *d_t_len,
                             const uint8_t *d_queries, const int64_t *d_q_start, const int32_t *d_q_len, int k, int w, int max_occ, int merge,
                             int max_cand, int64_t cand_capacity, int64_t *d_cand_start_out, int32_t *d_cand_t_out, int32_t *d_cand_q_out,
                             int32_t *d_cand_len_out, int32_t *d_status_out)
{
    // ---- arguments first: nothing below touches a device before they are known good
    const char *bad = nullptr;
    if (n < 0 || n > SEED_MAX_PAIRS) bad = "n outside 0 .. 2^30";
    else if (!d_targets || !d_t_start || !d_t_len) bad = "null target array";
    else if (!d_queries || !d_q_start || !d_q_len) bad = "null query array";
    else if (!d_cand_start_out || !d_cand_t_out || !d_cand_q_out || !d_cand_len_out) bad = "null candidate array";
    else if (k < SEED_MIN_K || k > SEED_MAX_K) bad = "k outside 4 .. 16";
    else if (w < 1 || w > SEED_MAX_W) bad = "w outside 1 .. 32";
    else if (max_occ < 1 || max_occ > SEED_MAX_OCC) bad = "max_occ outside 1 .. 64";
    else if (merge != 0 && merge != 1) bad = "merge is neither 0 nor 1";
    else if (max_cand < 1 || max_cand > SEED_MAX_CAND) bad = "max_cand outside 1 .. 8192";
    else if (cand_capacity < 0 || cand_capacity > SEED_MAX_PAIRS) bad = "cand_capacity outside 0 .. 2^30";
    if (bad) return refuse(ctx, "mgl_sw_seed_batch_device", bad);
    if (!ctx) return no_context();
    // there is no kernel id for this stage: the timing record keeps the fill_kernel it has (Stage's default)
    Stage stage(ctx, stream);
    hipStream_t st = stage.st;

    // ---- one workspace: the counts and the staging of the whole batch, then one slot per workgroup
    const int64_t limit = stage.limit();
    const SeedWorkspace sg = seed_workspace(n, max_cand);
    const int64_t room = limit - sg.bytes;
    if (room < sg.slot_bytes)
        return ctx_fail(ctx, MGL_SW_ERR_NOMEM, "mgl_sw_seed_batch_device: the workspace limit does not hold the batch's staging beside a slot: split the batch");
    const int64_t groups = std::min(std::min<int64_t>(std::max<int64_t>(n, 1), (int64_t)ctx_cus(ctx) * SEED_GROUPS_PER_CU), room / sg.slot_bytes);
    unsigned char *ws = nullptr;
    const int rc = stage.borrow((size_t)(sg.bytes + groups * sg.slot_bytes), &ws);
    if (rc != MGL_SW_OK) return rc;

    SeedStageArgs a{};
    a.targets = d_targets;
    a.queries = d_queries;
    a.t_start = d_t_start;
    a.q_start = d_q_start;
    a.t_len = d_t_len;
    a.q_len = d_q_len;
    a.n = n;
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

    hipError_t he = launch_seed(a, st);
    if (he != hipSuccess) return stage.fail(he, "launch_seed");
    he = launch_seed_scan(a, st);
    if (he != hipSuccess) return stage.fail(he, "launch_seed_scan");
    he = launch_seed_pack(a, st);
    if (he != hipSuccess) return stage.fail(he, "launch_seed_pack");
    return stage.done();
}

} // extern "C"
