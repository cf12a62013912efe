// sw_pileup.cpp -- mgl_sw_pileup_alignments_batch_device and mgl_sw_pileup_sites_device (include/mgl_sw.h): an alignment entry's
// records and CIGAR slots in, eight planes of counts per position of a region added to; and those planes in, the call, the flags and
// the candidate sites of every position out.  Host side only: argument checks, for the first entry one launch
// on the caller's stream and no workspace, for the second one workspace (a count and a first place per block of positions and the
// scan's storage) and three steps -- flag, scan, write.  No synchronisation.  The entries' frame is sw_stage_host.h's.
#include "../../include/mgl_sw.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "sw_describe.h"
#include "sw_pileup.h"
#include "sw_stage_host.h"

using namespace mgl_sw_dev;
using namespace mgl_sw_host;

static_assert(sizeof(mgl_sw_site) == 32, "eight int32");

extern "C" {

int mgl_sw_pileup_alignments_batch_device(mgl_sw_ctx *ctx, void *stream, int64_t n, const uint8_t *d_targets, const int64_t *d_t_start,
                                          const int32_t *d_t_len, const uint8_t *d_queries, const int64_t *d_q_start, const int32_t *d_q_len,
                                          const mgl_sw_chain_alignment *d_aln, const char *d_cigar, int cigar_stride, const int32_t *d_cigar_len,
                                          const int32_t *d_status_in, const int32_t *d_select, int64_t region_beg, int64_t region_len,
                                          uint32_t *d_counts, int32_t *d_status_out, int flags)
{
    // ---- arguments first: nothing below touches a device before they are known good
    const bool binary = (flags & MGL_SW_FLAG_BINARY_CIGAR) != 0;
    const char *bad = nullptr;
    if (n < 0) bad = "n < 0";
    else if (n > DESCRIBE_MAX_CHUNK) bad = "more than 2^30 alignments";
    else if (!d_targets || !d_t_start || !d_t_len || !d_queries || !d_q_start || !d_q_len) bad = "null sequence, start or length array";
    else if (!d_aln || !d_cigar || !d_cigar_len) bad = "null alignment records, CIGAR array or CIGAR lengths";
    else if (cigar_stride < 1 || (binary && cigar_stride % 4 != 0)) bad = "cigar_stride below 1, or no multiple of 4 for binary CIGARs";
    else if (region_beg < 0) bad = "region_beg < 0";
    else if (region_len < 1 || region_len > PILEUP_MAX_REGION) bad = "region_len outside 1 .. 2^31 - 1";
    else if (!d_counts) bad = "null d_counts";
    if (bad) return refuse(ctx, "mgl_sw_pileup_alignments_batch_device", bad);
    if (!ctx) return no_context();
    if (n == 0) return MGL_SW_OK;
    Stage stage(ctx, stream);

    PileupArgs a{};
    a.queries = d_queries; // (the target's bytes are not read: the planes take the QUERY's base, and a position is an offset)
    a.t_start = d_t_start;
    a.q_start = d_q_start;
    a.t_len = d_t_len;
    a.q_len = d_q_len;
    a.aln = d_aln;
    a.cigar = d_cigar;
    a.cigar_len = d_cigar_len;
    a.status_in = d_status_in;
    a.select = d_select;
    a.n = n;
    a.cigar_stride = cigar_stride;
    a.binary = binary ? 1 : 0;
    // a wave per alignment, DESCRIBE_WAVES a workgroup; as many workgroups as stay resident, and the waves go round beyond that
    a.groups = (int)std::min<int64_t>((n + DESCRIBE_WAVES - 1) / DESCRIBE_WAVES, (int64_t)ctx_cus(ctx) * DESCRIBE_GROUPS_PER_CU);
    a.region_beg = region_beg;
    a.region_len = region_len;
    a.counts = d_counts;
    a.status = d_status_out;
    const hipError_t he = launch_pileup(a, stage.st);
    if (he != hipSuccess) return stage.fail(he, "launch_pileup");
    return stage.done(); // (no workspace: the timing record is not touched)
}

int mgl_sw_pileup_sites_device(mgl_sw_ctx *ctx, void *stream, const uint32_t *d_counts, int64_t region_len, const uint8_t *d_targets,
                               int64_t region_beg, int min_depth, int min_alt, int min_frac, uint8_t *d_call_out, uint8_t *d_flags_out,
                               mgl_sw_site *d_sites_out, int64_t site_capacity, int64_t *d_n_sites_out)
{
    const char *bad = nullptr;
    if (!d_counts || !d_targets || !d_n_sites_out) bad = "null d_counts, d_targets or d_n_sites_out";
    else if (region_len < 1 || region_len > PILEUP_MAX_REGION) bad = "region_len outside 1 .. 2^31 - 1";
    else if (region_beg < 0) bad = "region_beg < 0";
    else if (min_depth < 1 || min_alt < 1) bad = "min_depth or min_alt < 1";
    else if (min_frac < 1 || min_frac > 256) bad = "min_frac outside 1 .. 256";
    else if (site_capacity < 0 || site_capacity > PILEUP_MAX_SITES) bad = "site_capacity outside 0 .. 2^30";
    else if (!d_sites_out && site_capacity > 0) bad = "null d_sites_out with a site_capacity above 0";
    if (bad) return refuse(ctx, "mgl_sw_pileup_sites_device", bad);
    if (!ctx) return no_context();
    Stage stage(ctx, stream);

    PileupSitesArgs a{};
    a.counts = d_counts;
    a.ref = d_targets + region_beg;
    a.region_len = region_len;
    a.blocks = (region_len + PILEUP_SITE_BLOCK - 1) / PILEUP_SITE_BLOCK;
    a.min_depth = min_depth;
    a.min_alt = min_alt;
    a.min_frac = min_frac;
    a.call = d_call_out;
    a.flags = d_flags_out;
    a.sites = d_sites_out;
    a.site_capacity = site_capacity;
    a.n_sites = d_n_sites_out;
    // the workspace: the blocks' counts, their first places (one more of each: the total), the scan's storage
    hipError_t he = pileup_scan_bytes(a.blocks + 1, &a.scan_bytes);
    if (he != hipSuccess) return ctx_hip_fail(ctx, he, "pileup_scan_bytes");
    a.scan_bytes = std::max<size_t>(a.scan_bytes, 256);
    const int64_t part = ((a.blocks + 1) * (int64_t)sizeof(int64_t) + 255) / 256 * 256;
    const int64_t bytes = 2 * part + (int64_t)((a.scan_bytes + 255) / 256 * 256);
    if (bytes > stage.limit())
        return ctx_fail(ctx, MGL_SW_ERR_NOMEM, "mgl_sw_pileup_sites_device: the workspace limit does not hold 16 bytes per 256 positions: split the region");
    unsigned char *ws = nullptr;
    const int rc = stage.borrow((size_t)bytes, &ws);
    if (rc != MGL_SW_OK) return rc;
    a.block_count = reinterpret_cast<int64_t *>(ws);
    a.block_start = reinterpret_cast<int64_t *>(ws + part);
    a.scan_tmp = ws + 2 * part;

    he = launch_pileup_flag(a, stage.st);
    if (he != hipSuccess) return stage.fail(he, "launch_pileup_flag");
    he = launch_pileup_scan(a, stage.st);
    if (he != hipSuccess) return stage.fail(he, "launch_pileup_scan");
    he = launch_pileup_write(a, stage.st);
    if (he != hipSuccess) return stage.fail(he, "launch_pileup_write");
    return stage.done();
}

} // extern "C"
