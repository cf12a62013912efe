// sw_ctx_access.h -- what the entries that live in translation units of their own (sw_local.cpp, sw_banded.cpp, sw_extend.cpp) need
// of a context: the accessors defined at the end of sw_capi.cpp, declared here once.  C++ names, hidden.  The caller holds
// ctx_mutex(ctx) around every other one.  sw_capi.cpp includes this too, so that the compiler checks each definition against its
// declaration; no kernel header is included here, so the host-sanitizer build of sw_capi.cpp (tests/cpp) needs nothing of the kernels.
// The frame of a stage entry on top of these -- the lock, the workspace, the way out -- is sw_stage_host.h.
#ifndef MGL_SW_CTX_ACCESS_H
#define MGL_SW_CTX_ACCESS_H

#include "../../include/mgl_sw.h"

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <mutex>

// library-internal entry points: not exported from the .so
#define MGL_SW_INTERNAL __attribute__((visibility("hidden")))

namespace mgl_sw_host {
// ctx_return_workspace's fill_kernel for a stage that has no MGL_SW_KERNEL_* id: the timing record keeps the one it has
constexpr int kKeepFillKernel = -1;

MGL_SW_INTERNAL std::mutex &ctx_mutex(mgl_sw_ctx *ctx);
MGL_SW_INTERNAL int ctx_device(mgl_sw_ctx *ctx);
MGL_SW_INTERNAL int ctx_cus(mgl_sw_ctx *ctx);
MGL_SW_INTERNAL int64_t ctx_workspace_limit(mgl_sw_ctx *ctx);
MGL_SW_INTERNAL int ctx_fail(mgl_sw_ctx *ctx, int status, const char *what);
MGL_SW_INTERNAL int ctx_hip_fail(mgl_sw_ctx *ctx, hipError_t e, const char *where);
MGL_SW_INTERNAL int ctx_stage_matrix(mgl_sw_ctx *ctx, hipStream_t st, const int8_t *matrix, const uint8_t *code, int8_t **d_matrix, uint8_t **d_code);
MGL_SW_INTERNAL int ctx_borrow_workspace(mgl_sw_ctx *ctx, hipStream_t st, size_t bytes, void **ws);
MGL_SW_INTERNAL int ctx_return_workspace(mgl_sw_ctx *ctx, hipStream_t st, int fill_kernel, int launches);
MGL_SW_INTERNAL int ctx_tile_counter(mgl_sw_ctx *ctx, hipStream_t st, unsigned **ctr, int32_t **fault);
MGL_SW_INTERNAL int ctx_tile_buffers(mgl_sw_ctx *ctx, hipStream_t st, size_t bytes, void **dev, void **host);
} // namespace mgl_sw_host

#endif
