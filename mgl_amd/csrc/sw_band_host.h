// sw_band_host.h -- the host side that mgl_sw_align_batch_device_banded (sw_banded.cpp) and mgl_sw_extend_batch_device (sw_extend.cpp)
// share: the clamp of the band and the launch of one wave per workspace slot.  Host code only.
#ifndef MGL_SW_BAND_HOST_H
#define MGL_SW_BAND_HOST_H

#include <algorithm>

#include "sw_banded.h"
#include "sw_ctx_access.h"

namespace mgl_sw_host {

// a band of max(tl, ql) covers a pair's matrix, and no pair beyond BANDED_MAX_LEN passes the range guard
inline int clamp_band(int band, int max_tl, int max_ql) { return std::min({band, std::max(max_tl, max_ql), mgl_sw_dev::BANDED_MAX_LEN}); }

// One workspace slot per wave of the grid, of slot_bound bytes (the largest pair the bounds admit); where the workspace cannot hold
// that, one slot of all there is (a pair that does not fit its slot: MGL_SW_ERR_UNSUPPORTED).  A wave takes every slots-th pair: a
// batch larger than the grid is worked off inside the one launch.  Fills a.ws, a.slot_bytes and a.slots and launches
template <class Args>
int launch_on_slots(mgl_sw_ctx *ctx, hipStream_t st, Args &a, int64_t slot_bound, hipError_t (*launch)(const Args &, hipStream_t), const char *where, int kernel)
{
    const int64_t limit = std::max<int64_t>(ctx_workspace_limit(ctx), 256) / 256 * 256;
    const int64_t slot = std::min<int64_t>(slot_bound, limit);
    const int64_t waves = std::max<int64_t>(1, std::min<int64_t>({a.n, (int64_t)ctx_cus(ctx) * mgl_sw_dev::BANDED_WAVES_PER_CU, limit / slot}));
    void *ws = nullptr;
    const int rc = ctx_borrow_workspace(ctx, st, (size_t)(waves * slot), &ws);
    if (rc != MGL_SW_OK) return rc;
    a.ws = static_cast<unsigned char *>(ws);
    a.slot_bytes = slot;
    a.slots = (int)waves;
    const hipError_t e = launch(a, st);
    if (e != hipSuccess) return ctx_hip_fail(ctx, e, where);
    return ctx_return_workspace(ctx, st, kernel, 1);
}

} // namespace mgl_sw_host

#endif
