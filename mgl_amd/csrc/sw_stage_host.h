// sw_stage_host.h -- the frame of a device entry that lives in a translation unit of its own (sw_seed.cpp ... sw_describe.cpp, the
// band entries, sw_local.cpp), once: the refusal of a bad argument, the answer to a null context, the rounded workspace limit, and
// Stage -- the context's lock for the length of the entry, the workspace borrowed at most once, and the two ways out.  Host code
// only, on top of sw_ctx_access.h and nothing of the kernels, so it compiles against tests/cpp/fake_hip as that header does
// (tests/cpp/host_san_driver.cpp drives it there).  What an entry does between these steps, and in which order, is its own.
#ifndef MGL_SW_STAGE_HOST_H
#define MGL_SW_STAGE_HOST_H

#include <algorithm>
#include <string>

#include "sw_ctx_access.h"

namespace mgl_sw_host {

// "<entry>: <bad>" as the context's error text (under its lock), where there is a context
inline int refuse(mgl_sw_ctx *ctx, const char *entry, const char *bad)
{
    if (ctx) {
        std::lock_guard<std::mutex> lk(ctx_mutex(ctx));
        ctx_fail(ctx, MGL_SW_ERR_BAD_ARG, (std::string(entry) + ": " + bad).c_str());
    }
    return MGL_SW_ERR_BAD_ARG;
}

// a well-formed call without a context
inline int no_context() { return mgl_sw_device_count() <= 0 ? MGL_SW_ERR_DEVICE : MGL_SW_ERR_BAD_ARG; }

// the context's workspace limit as the entries cut it up: a multiple of 256, at least 256
inline int64_t workspace_limit(mgl_sw_ctx *ctx) { return std::max<int64_t>(ctx_workspace_limit(ctx), 256) / 256 * 256; }

// One entry's hold on its context, from the lock on.  `kernel` and `launches` are what the timing record is to say of the call:
// an entry sets the first where it has a MGL_SW_KERNEL_* id (kKeepFillKernel: the record keeps the fill_kernel it has -- the
// context's business, ctx_return_workspace) and counts the second as it launches.
class Stage {
public:
    Stage(mgl_sw_ctx *c, void *stream) : ctx(c), st(static_cast<hipStream_t>(stream)), lk_(ctx_mutex(c)) {}

    mgl_sw_ctx *const ctx;
    const hipStream_t st;
    int kernel = kKeepFillKernel, launches = 0;

    int64_t limit() const { return workspace_limit(ctx); }

    // the workspace, behind the previous call's kernels; once per entry
    int borrow(size_t bytes, unsigned char **ws)
    {
        void *p = nullptr;
        const int rc = ctx_borrow_workspace(ctx, st, bytes, &p);
        borrowed_ = rc == MGL_SW_OK;
        *ws = static_cast<unsigned char *>(p);
        return rc;
    }
    // a step that fails behind others of this call: those still use the workspace, so it is returned (the next call on another
    // stream waits for them) before the error is
    int fail(hipError_t e, const char *where)
    {
        if (borrowed_) ctx_return_workspace(ctx, st, kernel, launches);
        borrowed_ = false;
        return ctx_hip_fail(ctx, e, where);
    }
    // the entry's last kernel is enqueued.  An entry that borrowed nothing leaves the timing record as it is
    int done(int fill_kernel, int n_launches)
    {
        if (!borrowed_) return MGL_SW_OK;
        borrowed_ = false;
        return ctx_return_workspace(ctx, st, fill_kernel, n_launches);
    }
    int done() { return done(kernel, launches); }

private:
    std::lock_guard<std::mutex> lk_;
    bool borrowed_ = false;
};

} // namespace mgl_sw_host

#endif
