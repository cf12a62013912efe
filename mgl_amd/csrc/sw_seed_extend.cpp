// sw_seed_extend.cpp -- mgl_sw_extend_seed_batch_device (include/mgl_sw.h): a seed extended to both sides and joined into one alignment
// (DESIGN.md section 9e).  Host side only: argument checks, one workspace for the staging of a chunk of pairs and the extension
// kernels' slots, and per chunk four launches on the caller's stream -- sw_seed_split_kernel, the extension kernel over the left
// flanks and over the right ones (sw_extend.hip or sw_extend_adaptive.hip, as they are), sw_seed_join_kernel.  No synchronisation.
// The entry's frame is sw_stage_host.h's, the two sides' extension sw_band_host.h's.
#include "../../include/mgl_sw.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "sw_band_host.h"
#include "sw_seed_extend.h"

using namespace mgl_sw_dev;

static_assert(sizeof(mgl_sw_seed_alignment) == sizeof(SeedAlignment), "mgl_sw_seed_alignment and the kernel's record are one layout");

using namespace mgl_sw_host;

extern "C" {

int mgl_sw_extend_seed_batch_device(mgl_sw_ctx *ctx, void *stream, int64_t n, const uint8_t *d_targets, const int64_t *d_t_start,
                                    const int32_t *d_t_len, const uint8_t *d_queries, const int64_t *d_q_start, const int32_t *d_q_len,
                                    const int32_t *d_seed_t, const int32_t *d_seed_q, const int32_t *d_seed_len, int max_tl, int max_ql, int match,
                                    int mismatch, int gopen, int gext, int band, int zdrop, mgl_sw_seed_alignment *d_aln_out,
                                    mgl_sw_extension *d_left_out, mgl_sw_extension *d_right_out, char *d_cigar_out, int cigar_stride,
                                    int32_t *d_cigar_len_out, int32_t *d_status_out, int flags)
{
    const bool score_only = (flags & MGL_SW_FLAG_SCORE_ONLY) != 0, binary = (flags & MGL_SW_FLAG_BINARY_CIGAR) != 0;
    // ---- arguments first: nothing below touches a device before they are known good
    const char *bad = nullptr;
    if (n < 0) bad = "n < 0";
    else if (!d_targets || !d_t_start || !d_t_len || !d_queries || !d_q_start || !d_q_len) bad = "null sequence, start or length array";
    else if (!d_seed_t || !d_seed_q || !d_seed_len) bad = "null seed array";
    else if (!d_aln_out) bad = "null alignment array";
    else if (band < 0) bad = "band < 0";
    else if (max_tl < 1 || max_ql < 1) bad = "max_tl / max_ql < 1";
    else if (!score_only && (!d_cigar_out || !d_cigar_len_out || cigar_stride < (binary ? 4 : 2))) bad = "CIGAR array missing or cigar_stride too small";
    if (bad) return refuse(ctx, "mgl_sw_extend_seed_batch_device", bad);
    if (!ctx) return no_context();
    Stage stage(ctx, stream);
    if (n == 0) return MGL_SW_OK;
    mgl_sw_normalize_params(&match, &mismatch, &gopen, &gext);
    hipStream_t st = stage.st;

    // ---- the extension of one side (sw_band_host.h)
    ExtendArgs e{};
    const int64_t slot_bound = extend_sides_setup(stage, e, match, mismatch, gopen, gext, flags, band, zdrop, max_tl, max_ql);

    // ---- one workspace: the staging of a chunk of m pairs, then one slot per wave.  All n pairs are staged at once where that takes
    // at most half the limit (the slots, which set the number of waves, keep the other half).  Otherwise the batch is worked off in
    // chunks of m pairs, m the most whose staging half the limit holds: a pair's exact bytes, and 256 bytes of rounding for each part.
    // Where half the limit does not hold one pair, m is 1 and that pair's staging takes more than half; the slot gets what is left
    const int64_t limit = stage.limit();
    auto staged = [&](int64_t m) { return seed_staging(m, max_tl, max_ql, cigar_stride, binary, score_only).bytes; };
    const int64_t per_pair = seed_staging_pair_bytes(seed_staging(1, max_tl, max_ql, cigar_stride, binary, score_only));
    int64_t m = std::min(n, SEED_MAX_CHUNK);
    if (staged(m) > limit / 2) m = std::max<int64_t>(1, std::min(m, (limit / 2 - SEED_STAGING_PARTS * 256) / per_pair));
    const int64_t slot = std::min(slot_bound, (limit - staged(m)) / 256 * 256);
    if (slot < 256) return ctx_fail(ctx, MGL_SW_ERR_NOMEM, "mgl_sw_extend_seed_batch_device: the workspace limit does not hold the staging of one pair beside a slot");
    const SeedStaging sg = seed_staging(m, max_tl, max_ql, cigar_stride, binary, score_only);
    const int64_t waves = std::max<int64_t>(1, std::min<int64_t>({m, (int64_t)ctx_cus(ctx) * BANDED_WAVES_PER_CU, (limit - sg.bytes) / slot}));
    unsigned char *ws = nullptr;
    const int rc = stage.borrow((size_t)(sg.bytes + waves * slot), &ws);
    if (rc != MGL_SW_OK) return rc;
    e.ws = ws + sg.bytes;
    e.slot_bytes = slot;
    e.slots = (int)waves;
    e.cigar_stride = (int)sg.istride;

    SeedArgs s{};
    s.targets = d_targets;
    s.queries = d_queries;
    s.max_tl = max_tl;
    s.max_ql = max_ql;
    s.match = match;
    s.mismatch = mismatch;
    bind_seed_staging(s, ws, sg, score_only);
    s.cigar_stride = cigar_stride;
    s.binary_cigar = binary ? 1 : 0;
    s.score_only = score_only ? 1 : 0;

    for (int64_t c = 0; c < n; c += m) {
        s.n = e.n = std::min(m, n - c);
        s.t_start = d_t_start + c;
        s.t_len = d_t_len + c;
        s.q_start = d_q_start + c;
        s.q_len = d_q_len + c;
        s.seed_t = d_seed_t + c;
        s.seed_q = d_seed_q + c;
        s.seed_len = d_seed_len + c;
        s.aln = reinterpret_cast<SeedAlignment *>(d_aln_out) + c;
        s.left_out = d_left_out ? reinterpret_cast<Extension *>(d_left_out) + c : nullptr;
        s.right_out = d_right_out ? reinterpret_cast<Extension *>(d_right_out) + c : nullptr;
        s.cigar = d_cigar_out ? d_cigar_out + c * (int64_t)cigar_stride : nullptr;
        s.cigar_len = d_cigar_len_out ? d_cigar_len_out + c : nullptr;
        s.status = d_status_out ? d_status_out + c : nullptr;
        hipError_t he = launch_seed_split(s, st);
        if (he != hipSuccess) return stage.fail(he, "launch_seed_split");
        const int src = launch_extend_sides(stage, e, s, ws, sg);
        if (src != MGL_SW_OK) return src;
        he = launch_seed_join(s, st);
        if (he != hipSuccess) return stage.fail(he, "launch_seed_join");
    }
    return stage.done();
}

} // extern "C"
