// sw_lines.cpp -- mgl_sw_expand_chains_batch_device and mgl_sw_classify_alignments_batch_device (include/mgl_sw.h): the rank stage's
// chains in, one alignment job per chain out; and the jobs' alignments in, the lines of every read out.  Host
// side only: argument checks, for the first entry one workspace (three counts and one offset per read) and four launches on the
// caller's stream -- count, scan, pack, orient --, for the second one launch and no workspace.  No synchronisation.  The entries'
// frame is sw_stage_host.h's.
#include "../../include/mgl_sw.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "sw_lines.h"
#include "sw_stage_host.h"

using namespace mgl_sw_dev;
using namespace mgl_sw_host;

static_assert(sizeof(mgl_sw_job) == 32, "eight int32");
static_assert(sizeof(mgl_sw_line) == 32, "eight int32");

extern "C" {

int mgl_sw_expand_chains_batch_device(mgl_sw_ctx *ctx, void *stream, int64_t n, const uint8_t *d_queries, const int64_t *d_q_start, const int32_t *d_q_len,
                                      int64_t query_bytes, const int32_t *d_rank_status, const int32_t *d_n_chains, const mgl_sw_ranked_chain *d_records,
                                      int max_chains, const int64_t *d_ranked_start, const int32_t *d_ranked_t, const int32_t *d_ranked_q,
                                      const int32_t *d_ranked_len, int64_t total_anchors, int keep_secondary, int64_t job_capacity, int64_t *d_n_jobs_out,
                                      int64_t *d_job_start_out, mgl_sw_job *d_jobs_out, int64_t *d_job_q_start_out, int32_t *d_job_q_len_out,
                                      int64_t *d_job_anchor_start_out, int32_t *d_job_anchor_t_out, int32_t *d_job_anchor_q_out,
                                      int32_t *d_job_anchor_len_out, uint8_t *d_oriented_out, int32_t *d_status_out)
{
    // ---- arguments first: nothing below touches a device before they are known good
    const char *bad = nullptr;
    if (n < 0 || n > LINES_MAX_READS) bad = "n outside 0 .. 2^29";
    else if (max_chains < 1 || max_chains > LINES_MAX_CHAINS) bad = "max_chains outside 1 .. 16";
    else if (job_capacity < 0 || job_capacity > LINES_MAX_JOBS) bad = "job_capacity outside 0 .. 2^30";
    else if (total_anchors < 0 || total_anchors > LINES_MAX_JOBS) bad = "total_anchors outside 0 .. 2^30";
    else if (query_bytes < 0 || query_bytes > LINES_MAX_BYTES) bad = "query_bytes outside 0 .. 2^40";
    else if (keep_secondary != 0 && keep_secondary != 1) bad = "keep_secondary outside 0, 1";
    else if (!d_queries || !d_q_start || !d_q_len) bad = "null read array";
    else if (!d_n_chains || !d_records || !d_ranked_start || !d_ranked_t || !d_ranked_q || !d_ranked_len) bad = "null chain count, records or ranked anchor array";
    else if (!d_n_jobs_out || !d_job_start_out || !d_jobs_out || !d_job_q_start_out || !d_job_q_len_out) bad = "null job output";
    else if (!d_job_anchor_start_out || !d_job_anchor_t_out || !d_job_anchor_q_out || !d_job_anchor_len_out) bad = "null job anchor output";
    else if (!d_oriented_out) bad = "null d_oriented_out";
    else if (d_oriented_out < d_queries + query_bytes && d_queries < d_oriented_out + 2 * query_bytes) bad = "d_oriented_out overlaps d_queries";
    if (bad) return refuse(ctx, "mgl_sw_expand_chains_batch_device", bad);
    if (!ctx) return no_context();
    // there is no kernel id for this stage: the timing record keeps the fill_kernel it has (Stage's default)
    Stage stage(ctx, stream);
    hipStream_t st = stage.st;

    const ExpandWorkspace wk = expand_workspace(n);
    if (wk.bytes > stage.limit())
        return ctx_fail(ctx, MGL_SW_ERR_NOMEM, "mgl_sw_expand_chains_batch_device: the workspace limit does not hold 20 bytes per read: split the batch");
    unsigned char *ws = nullptr;
    const int rc = stage.borrow((size_t)std::max<int64_t>(wk.bytes, 256), &ws);
    if (rc != MGL_SW_OK) return rc;

    ExpandArgs a{};
    a.queries = d_queries;
    a.q_start = d_q_start;
    a.q_len = d_q_len;
    a.rank_status = d_rank_status;
    a.n_chains = d_n_chains;
    a.records = d_records;
    a.ranked_start = d_ranked_start;
    a.ranked_t = d_ranked_t;
    a.ranked_q = d_ranked_q;
    a.ranked_len = d_ranked_len;
    a.n = n;
    a.query_bytes = query_bytes;
    a.total_anchors = total_anchors;
    a.job_capacity = job_capacity;
    a.max_chains = max_chains;
    a.keep_secondary = keep_secondary;
    // a workgroup per (read, strand); as many as keep the device busy, and they go round beyond that
    a.groups = (int)std::min<int64_t>(std::max<int64_t>(2 * n, 1), (int64_t)ctx_cus(ctx) * 8);
    a.ws_jobs = reinterpret_cast<int32_t *>(ws + wk.jobs);
    a.ws_anchors = reinterpret_cast<int32_t *>(ws + wk.anchors);
    a.ws_strands = reinterpret_cast<int32_t *>(ws + wk.strands);
    a.ws_anchor_at = reinterpret_cast<int64_t *>(ws + wk.anchor_at);
    a.n_jobs = d_n_jobs_out;
    a.job_start = d_job_start_out;
    a.jobs = d_jobs_out;
    a.job_q_start = d_job_q_start_out;
    a.job_q_len = d_job_q_len_out;
    a.job_anchor_start = d_job_anchor_start_out;
    a.job_anchor_t = d_job_anchor_t_out;
    a.job_anchor_q = d_job_anchor_q_out;
    a.job_anchor_len = d_job_anchor_len_out;
    a.oriented = d_oriented_out;
    a.status = d_status_out;

    hipError_t he = launch_expand_count(a, st);
    if (he != hipSuccess) return stage.fail(he, "launch_expand_count");
    he = launch_expand_scan(a, st); // (n = 0 too: n_jobs = 0)
    if (he != hipSuccess) return stage.fail(he, "launch_expand_scan");
    he = launch_expand_pack(a, st); // (n = 0 too: the empty tail)
    if (he != hipSuccess) return stage.fail(he, "launch_expand_pack");
    he = launch_expand_orient(a, st);
    if (he != hipSuccess) return stage.fail(he, "launch_expand_orient");
    return stage.done();
}

int mgl_sw_classify_alignments_batch_device(mgl_sw_ctx *ctx, void *stream, int64_t n, const int64_t *d_job_start, const mgl_sw_job *d_jobs,
                                            int64_t job_capacity, const mgl_sw_chain_alignment *d_aln, const int32_t *d_aln_status, int match,
                                            int min_score, int mask_level, mgl_sw_line *d_lines_out, int32_t *d_n_lines_out,
                                            int32_t *d_primary_job_out, int32_t *d_status_out)
{
    const char *bad = nullptr;
    if (n < 0 || n > LINES_MAX_READS) bad = "n outside 0 .. 2^29";
    else if (job_capacity < 0 || job_capacity > LINES_MAX_JOBS) bad = "job_capacity outside 0 .. 2^30";
    else if (!d_job_start || !d_jobs || !d_aln || !d_aln_status) bad = "null job start, job, alignment or alignment status array";
    else if (!d_lines_out || !d_n_lines_out || !d_primary_job_out) bad = "null d_lines_out, d_n_lines_out or d_primary_job_out";
    else if (match < 1 || min_score < 1) bad = "match or min_score < 1";
    else if (mask_level < 1 || mask_level > 256) bad = "mask_level outside 1 .. 256";
    if (bad) return refuse(ctx, "mgl_sw_classify_alignments_batch_device", bad);
    if (!ctx) return no_context();
    if (n == 0) return MGL_SW_OK;
    Stage stage(ctx, stream);

    ClassifyArgs a{};
    a.job_start = d_job_start;
    a.jobs = d_jobs;
    a.aln = d_aln;
    a.aln_status = d_aln_status;
    a.n = n;
    a.job_capacity = job_capacity;
    a.match = match;
    a.min_score = min_score;
    a.mask_level = mask_level;
    a.lines = d_lines_out;
    a.n_lines = d_n_lines_out;
    a.primary_job = d_primary_job_out;
    a.status = d_status_out;
    const hipError_t he = launch_classify(a, stage.st);
    if (he != hipSuccess) return stage.fail(he, "launch_classify");
    return stage.done(); // (no workspace: the timing record is not touched)
}

} // extern "C"
