// sw_calls.cpp -- mgl_sw_pileup_insertions_batch_device and mgl_sw_genotype_sites_device (include/mgl_sw.h): the pileup's alignments
// and the candidate sites in, a row of insertion lengths and inserted bases per site added to; and the planes, the sites and those
// rows in, the events of every site with genotype, likelihoods and quality out.  Host side only: argument
// checks, for the first entry one launch on the caller's stream and no workspace, for the second one workspace (a count and a first
// place per block of site slots and the scan's storage) and three steps -- count, scan, write.  No synchronisation.  The entries'
// frame is sw_stage_host.h's.
#include "../../include/mgl_sw.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "sw_calls.h"
#include "sw_describe.h"
#include "sw_pileup.h"
#include "sw_stage_host.h"

using namespace mgl_sw_dev;
using namespace mgl_sw_host;

static_assert(sizeof(mgl_sw_call) == 64, "sixteen int32");

extern "C" {

int mgl_sw_pileup_insertions_batch_device(mgl_sw_ctx *ctx, void *stream, int64_t n, const uint8_t *d_targets, const int64_t *d_t_start,
                                          const int32_t *d_t_len, const uint8_t *d_queries, const int64_t *d_q_start, const int32_t *d_q_len,
                                          const mgl_sw_chain_alignment *d_aln, const char *d_cigar, int cigar_stride, const int32_t *d_cigar_len,
                                          const int32_t *d_status_in, const int32_t *d_select, int64_t region_beg, const mgl_sw_site *d_sites,
                                          const int64_t *d_n_sites, int64_t site_capacity, int max_ins, uint32_t *d_ins, int32_t *d_status_out,
                                          int flags)
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
    else if (!d_sites || !d_n_sites || !d_ins) bad = "null d_sites, d_n_sites or d_ins";
    else if (site_capacity < 1 || site_capacity > PILEUP_MAX_SITES) bad = "site_capacity outside 1 .. 2^30";
    else if (max_ins < 1 || max_ins > CALLS_MAX_INS) bad = "max_ins outside 1 .. 64";
    if (bad) return refuse(ctx, "mgl_sw_pileup_insertions_batch_device", bad);
    if (!ctx) return no_context();
    if (n == 0) return MGL_SW_OK;
    Stage stage(ctx, stream);

    InsertionsArgs a{};
    a.queries = d_queries; // (the target's bytes are not read: a position is an offset, and the inserted bases are the QUERY's)
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
    // the pileup's grid: a wave per alignment, DESCRIBE_WAVES a workgroup; as many workgroups as stay resident
    a.groups = (int)std::min<int64_t>((n + DESCRIBE_WAVES - 1) / DESCRIBE_WAVES, (int64_t)ctx_cus(ctx) * DESCRIBE_GROUPS_PER_CU);
    a.region_beg = region_beg;
    a.sites = d_sites;
    a.n_sites = d_n_sites;
    a.site_capacity = site_capacity;
    a.max_ins = max_ins;
    a.ins = d_ins;
    a.status = d_status_out;
    const hipError_t he = launch_insertions(a, stage.st);
    if (he != hipSuccess) return stage.fail(he, "launch_insertions");
    return stage.done(); // (no workspace: the timing record is not touched)
}

int mgl_sw_genotype_sites_device(mgl_sw_ctx *ctx, void *stream, const uint32_t *d_counts, int64_t region_len, const uint8_t *d_targets,
                                 int64_t region_beg, const mgl_sw_site *d_sites, const int64_t *d_n_sites, int64_t site_capacity,
                                 const uint32_t *d_ins, int max_ins, int max_del, int cost_match, int cost_het, int cost_error,
                                 mgl_sw_call *d_calls_out, int64_t call_capacity, int64_t *d_n_calls_out, uint8_t *d_ins_seq_out)
{
    auto cost_ok = [](const int c) { return c >= 1 && c <= CALLS_MAX_COST; };
    const char *bad = nullptr;
    if (!d_counts || !d_targets || !d_n_calls_out) bad = "null d_counts, d_targets or d_n_calls_out";
    else if (!d_sites || !d_n_sites) bad = "null d_sites or d_n_sites";
    else if (region_len < 1 || region_len > PILEUP_MAX_REGION) bad = "region_len outside 1 .. 2^31 - 1";
    else if (region_beg < 0) bad = "region_beg < 0";
    else if (site_capacity < 1 || site_capacity > PILEUP_MAX_SITES) bad = "site_capacity outside 1 .. 2^30";
    else if (max_ins < 1 || max_ins > CALLS_MAX_INS) bad = "max_ins outside 1 .. 64";
    else if (max_del < 1 || max_del > CALLS_MAX_DEL) bad = "max_del outside 1 .. 4096";
    else if (!cost_ok(cost_match) || !cost_ok(cost_het) || !cost_ok(cost_error)) bad = "a cost outside 1 .. 2^20";
    else if (!(cost_match < cost_het && cost_het < cost_error)) bad = "the costs are not cost_match < cost_het < cost_error";
    else if (call_capacity < 0 || call_capacity > CALLS_MAX_CALLS) bad = "call_capacity outside 0 .. 2^30";
    else if (!d_calls_out && call_capacity > 0) bad = "null d_calls_out with a call_capacity above 0";
    else if (!d_ins_seq_out && d_ins && call_capacity > 0) bad = "null d_ins_seq_out with d_ins and a call_capacity above 0";
    if (bad) return refuse(ctx, "mgl_sw_genotype_sites_device", bad);
    if (!ctx) return no_context();
    Stage stage(ctx, stream);

    GenotypeArgs g{};
    g.counts = d_counts;
    g.ref = d_targets + region_beg;
    g.region_len = region_len;
    g.sites = d_sites;
    g.n_sites = d_n_sites;
    g.site_capacity = site_capacity;
    g.blocks = (site_capacity + CALLS_SITE_BLOCK - 1) / CALLS_SITE_BLOCK;
    g.ins = d_ins;
    g.max_ins = max_ins;
    g.max_del = max_del;
    g.cost_match = cost_match;
    g.cost_het = cost_het;
    g.cost_error = cost_error;
    g.calls = d_calls_out;
    g.call_capacity = call_capacity;
    g.n_calls = d_n_calls_out;
    g.ins_seq = call_capacity > 0 ? d_ins_seq_out : nullptr;
    // the workspace: the blocks' counts, their first places (one more of each: the total), the scan's storage
    hipError_t he = genotype_scan_bytes(g.blocks + 1, &g.scan_bytes);
    if (he != hipSuccess) return ctx_hip_fail(ctx, he, "genotype_scan_bytes");
    g.scan_bytes = std::max<size_t>(g.scan_bytes, 256);
    const int64_t part = ((g.blocks + 1) * (int64_t)sizeof(int64_t) + 255) / 256 * 256;
    const int64_t bytes = 2 * part + (int64_t)((g.scan_bytes + 255) / 256 * 256);
    if (bytes > stage.limit())
        return ctx_fail(ctx, MGL_SW_ERR_NOMEM, "mgl_sw_genotype_sites_device: the workspace limit does not hold 16 bytes per 256 site slots: lower site_capacity");
    unsigned char *ws = nullptr;
    const int rc = stage.borrow((size_t)bytes, &ws);
    if (rc != MGL_SW_OK) return rc;
    g.block_count = reinterpret_cast<int64_t *>(ws);
    g.block_start = reinterpret_cast<int64_t *>(ws + part);
    g.scan_tmp = ws + 2 * part;

    he = launch_genotype_count(g, stage.st);
    if (he != hipSuccess) return stage.fail(he, "launch_genotype_count");
    he = launch_genotype_scan(g, stage.st);
    if (he != hipSuccess) return stage.fail(he, "launch_genotype_scan");
    he = launch_genotype_write(g, stage.st);
    if (he != hipSuccess) return stage.fail(he, "launch_genotype_write");
    return stage.done();
}

} // extern "C"
