// sw_band_host.h -- the host side that the band entries share.  mgl_sw_align_batch_device_banded (sw_banded.cpp) and
// mgl_sw_extend_batch_device (sw_extend.cpp): the clamp of the band and the launch of one wave per workspace slot.
// mgl_sw_extend_seed_batch_device (sw_seed_extend.cpp) and mgl_sw_align_chain_batch_device (sw_chain.cpp): the extension of a pair's two
// sides -- its arguments, the binding of the staging, the two launches.  Host code only, on the entries' frame (sw_stage_host.h); no
// .hip file includes this.
#ifndef MGL_SW_BAND_HOST_H
#define MGL_SW_BAND_HOST_H

#include <algorithm>

#include "sw_seed_extend.h"
#include "sw_stage_host.h"

namespace mgl_sw_host {

// a band of max(tl, ql) covers a pair's matrix, and no pair beyond BANDED_MAX_LEN passes the range guard
inline int clamp_band(int band, int max_tl, int max_ql) { return std::min({band, std::max(max_tl, max_ql), mgl_sw_dev::BANDED_MAX_LEN}); }

// a fixed band of max(tl, ql) covers a pair's matrix; one that follows the path does so wherever it stands only from tl + ql on, so
// the clamp that keeps the geometry in int32 (|d_k| <= max(tl, ql) <= BANDED_MAX_LEN, see sw_extend_adaptive.hip) is wider there
inline int clamp_extend_band(bool adaptive, int band, int max_tl, int max_ql)
{
    return adaptive ? (int)std::min<int64_t>({(int64_t)band, (int64_t)max_tl + max_ql, 2 * (int64_t)mgl_sw_dev::BANDED_MAX_LEN}) : clamp_band(band, max_tl, max_ql);
}

// the band does not widen with |ql - tl|, so a slot's formula is monotone in both lengths and the largest pair the bounds admit is
// the bounds themselves
inline int64_t extend_slot_bound(bool adaptive, int max_tl, int max_ql, int band, bool score_only)
{
    const int cap_tl = std::min(max_tl, mgl_sw_dev::BANDED_MAX_LEN), cap_ql = std::min(max_ql, mgl_sw_dev::BANDED_MAX_LEN);
    return adaptive ? mgl_sw_dev::extend_adaptive_pair_bytes(cap_tl, cap_ql, band, score_only) : mgl_sw_dev::extend_pair_bytes(cap_tl, cap_ql, band, score_only);
}

// One workspace slot per wave of the grid, of slot_bound bytes (the largest pair the bounds admit); where the workspace cannot hold
// that, one slot of all there is (a pair that does not fit its slot: MGL_SW_ERR_UNSUPPORTED).  A wave takes every slots-th pair: a
// batch larger than the grid is worked off inside the one launch.  Fills a.ws, a.slot_bytes and a.slots and launches
template <class Args>
int launch_on_slots(Stage &stage, Args &a, int64_t slot_bound, hipError_t (*launch)(const Args &, hipStream_t), const char *where, int kernel)
{
    const int64_t limit = stage.limit();
    const int64_t slot = std::min<int64_t>(slot_bound, limit);
    const int64_t waves = std::max<int64_t>(1, std::min<int64_t>({a.n, (int64_t)ctx_cus(stage.ctx) * mgl_sw_dev::BANDED_WAVES_PER_CU, limit / slot}));
    const int rc = stage.borrow((size_t)(waves * slot), &a.ws);
    if (rc != MGL_SW_OK) return rc;
    a.slot_bytes = slot;
    a.slots = (int)waves;
    stage.kernel = kernel;
    const hipError_t e = launch(a, stage.st);
    if (e != hipSuccess) return stage.fail(e, where);
    return stage.done(kernel, 1);
}

// ---- the two sides of a seed or a chain (sw_seed_extend.cpp, sw_chain.cpp)

// The extension of one side: the extend entry's arguments, band clamp and slot bound (sw_extend.cpp), on the normalised parameters; a
// flank is shorter than its pair, so the caller's bounds hold for it.  Sets stage.kernel to the extension that runs and returns the
// slot bound; e.ws, e.slot_bytes, e.slots, e.cigar_stride and e.n are the entry's to set once it has cut up its workspace
inline int64_t extend_sides_setup(Stage &stage, mgl_sw_dev::ExtendArgs &e, int match, int mismatch, int gopen, int gext, int flags, int band, int zdrop,
                                  int max_tl, int max_ql)
{
    const bool adaptive = (flags & MGL_SW_FLAG_EXTEND_ADAPTIVE_BAND) != 0, score_only = (flags & MGL_SW_FLAG_SCORE_ONLY) != 0;
    e.match = match;
    e.mismatch = mismatch;
    e.gopen = gopen;
    e.gext = gext;
    e.band = clamp_extend_band(adaptive, band, max_tl, max_ql);
    e.zdrop = zdrop;
    e.max_tl = max_tl;
    e.max_ql = max_ql;
    e.binary_cigar = 1; // the internal rows: the join reads elements, not text
    e.score_only = score_only ? 1 : 0;
    e.to_query_end = (flags & MGL_SW_FLAG_EXTEND_TO_QUERY_END) ? 1 : 0;
    stage.kernel = adaptive ? MGL_SW_KERNEL_EXTEND_ADAPTIVE : MGL_SW_KERNEL_EXTEND;
    return extend_slot_bound(adaptive, max_tl, max_ql, e.band, score_only);
}

// the per-pair staging (sw_seed_extend.h) at `ws`, as the fields SeedArgs and ChainArgs have in common
template <class Args>
void bind_seed_staging(Args &s, unsigned char *ws, const mgl_sw_dev::SeedStaging &sg, bool score_only)
{
    using namespace mgl_sw_dev;
    s.rev_t = ws + sg.rev_t;
    s.rev_q = ws + sg.rev_q;
    s.tstride = sg.tstride;
    s.qstride = sg.qstride;
    for (int x = 0; x < 4; ++x) {
        s.off[x] = reinterpret_cast<int64_t *>(ws + sg.off[x]);
        s.len[x] = reinterpret_cast<int32_t *>(ws + sg.len[x]);
    }
    s.flank = reinterpret_cast<int4 *>(ws + sg.flank);
    for (int x = 0; x < 2; ++x) {
        s.side_ext[x] = reinterpret_cast<const Extension *>(ws + sg.ext[x]);
        s.side_status[x] = reinterpret_cast<const int32_t *>(ws + sg.status[x]);
        s.side_clen[x] = reinterpret_cast<const int32_t *>(ws + sg.clen[x]);
        s.side_cigar[x] = score_only ? nullptr : reinterpret_cast<const uint32_t *>(ws + sg.cigar[x]);
    }
    s.istride = sg.istride;
}

// the extension kernel over the left flanks and over the right ones, behind the split that wrote their descriptors; counts its launches
template <class Args>
int launch_extend_sides(Stage &stage, mgl_sw_dev::ExtendArgs &e, const Args &s, unsigned char *ws, const mgl_sw_dev::SeedStaging &sg)
{
    using namespace mgl_sw_dev;
    const bool adaptive = stage.kernel == MGL_SW_KERNEL_EXTEND_ADAPTIVE;
    for (int side = 0; side < 2; ++side) { // 0: the reversed copies of the left flanks; 1: the right flanks in the caller's arrays
        e.t = SeqSet{side ? s.targets : s.rev_t, s.off[2 * side], s.len[2 * side], e.max_tl, 0};
        e.q = SeqSet{side ? s.queries : s.rev_q, s.off[2 * side + 1], s.len[2 * side + 1], e.max_ql, 0};
        e.ext = reinterpret_cast<Extension *>(ws + sg.ext[side]);
        e.status = reinterpret_cast<int32_t *>(ws + sg.status[side]);
        e.cigar = e.score_only ? nullptr : reinterpret_cast<char *>(ws + sg.cigar[side]);
        e.cigar_len = reinterpret_cast<int32_t *>(ws + sg.clen[side]);
        const hipError_t he = adaptive ? launch_extend_adaptive(e, stage.st) : launch_extend(e, stage.st);
        if (he != hipSuccess) return stage.fail(he, adaptive ? "launch_extend_adaptive" : "launch_extend");
        ++stage.launches;
    }
    return MGL_SW_OK;
}

} // namespace mgl_sw_host

#endif
