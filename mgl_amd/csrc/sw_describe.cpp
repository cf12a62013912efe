// sw_describe.cpp -- mgl_sw_describe_alignments_batch_device (include/mgl_sw.h): an alignment entry's records and CIGAR slots in, the
// counts, the MD text and the extended CIGAR of every alignment out.  Host side only: argument checks and one
// launch on the caller's stream, sw_describe_kernel.  No workspace and no synchronisation; the timing record is not touched, so it
// keeps the fill_kernel it has.  The entry's frame is sw_stage_host.h's.
#include "../../include/mgl_sw.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "sw_describe.h"
#include "sw_stage_host.h"

using namespace mgl_sw_dev;
using namespace mgl_sw_host;

static_assert(sizeof(mgl_sw_alignment_stats) == 32, "eight int32");
// the entry reads the records of either alignment entry: one layout
static_assert(sizeof(mgl_sw_seed_alignment) == sizeof(mgl_sw_chain_alignment), "one layout");
static_assert(offsetof(mgl_sw_seed_alignment, t_beg) == offsetof(mgl_sw_chain_alignment, t_beg) &&
                  offsetof(mgl_sw_seed_alignment, t_end) == offsetof(mgl_sw_chain_alignment, t_end) &&
                  offsetof(mgl_sw_seed_alignment, q_beg) == offsetof(mgl_sw_chain_alignment, q_beg) &&
                  offsetof(mgl_sw_seed_alignment, q_end) == offsetof(mgl_sw_chain_alignment, q_end),
              "one layout");

extern "C" {

int mgl_sw_describe_alignments_batch_device(mgl_sw_ctx *ctx, void *stream, int64_t n, const uint8_t *d_targets, const int64_t *d_t_start,
                                            const int32_t *d_t_len, const uint8_t *d_queries, const int64_t *d_q_start, const int32_t *d_q_len,
                                            const mgl_sw_chain_alignment *d_aln, const char *d_cigar, int cigar_stride, const int32_t *d_cigar_len,
                                            const int32_t *d_status_in, mgl_sw_alignment_stats *d_stats_out, char *d_md_out, int md_stride,
                                            char *d_xcigar_out, int xcigar_stride, int32_t *d_status_out, int flags)
{
    // ---- arguments first: nothing below touches a device before they are known good
    const bool binary = (flags & MGL_SW_FLAG_BINARY_CIGAR) != 0;
    const char *bad = nullptr;
    if (n < 0) bad = "n < 0";
    else if (n > DESCRIBE_MAX_CHUNK) bad = "more than 2^30 alignments";
    else if (!d_targets || !d_t_start || !d_t_len || !d_queries || !d_q_start || !d_q_len) bad = "null sequence, start or length array";
    else if (!d_aln || !d_cigar || !d_cigar_len) bad = "null alignment records, CIGAR array or CIGAR lengths";
    else if (!d_stats_out) bad = "null d_stats_out";
    else if (cigar_stride < 1 || (binary && cigar_stride % 4 != 0)) bad = "cigar_stride below 1, or no multiple of 4 for binary CIGARs";
    else if (d_md_out && md_stride < 1) bad = "md_stride below 1";
    else if (d_xcigar_out && (xcigar_stride < 1 || (binary && xcigar_stride % 4 != 0))) bad = "xcigar_stride below 1, or no multiple of 4 for binary CIGARs";
    if (bad) return refuse(ctx, "mgl_sw_describe_alignments_batch_device", bad);
    if (!ctx) return no_context();
    if (n == 0) return MGL_SW_OK;
    Stage stage(ctx, stream);

    DescribeArgs a{};
    a.targets = d_targets;
    a.queries = d_queries;
    a.t_start = d_t_start;
    a.q_start = d_q_start;
    a.t_len = d_t_len;
    a.q_len = d_q_len;
    a.aln = d_aln;
    a.cigar = d_cigar;
    a.cigar_len = d_cigar_len;
    a.status_in = d_status_in;
    a.n = n;
    a.cigar_stride = cigar_stride;
    a.md_stride = d_md_out ? md_stride : 0;
    a.xcigar_stride = d_xcigar_out ? xcigar_stride : 0;
    a.binary = binary ? 1 : 0;
    // a wave per alignment, DESCRIBE_WAVES a workgroup; as many workgroups as stay resident, and the waves go round beyond that
    a.groups = (int)std::min<int64_t>((n + DESCRIBE_WAVES - 1) / DESCRIBE_WAVES, (int64_t)ctx_cus(ctx) * DESCRIBE_GROUPS_PER_CU);
    a.stats = d_stats_out;
    a.md = d_md_out;
    a.xcigar = d_xcigar_out;
    a.status = d_status_out;
    const hipError_t he = launch_describe(a, stage.st);
    if (he != hipSuccess) return stage.fail(he, "launch_describe");
    return stage.done(); // (no workspace: the timing record is not touched)
}

} // extern "C"
