// sw_local.cpp -- mgl_sw_local_batch_device_matrix (include/mgl_sw.h): local Smith-Waterman with a substitution matrix.  Host side only:
// argument checks, the planner rule, the workspace and the launches of the two kernels (sw_local_lane.hip: kernel A, the packed score
// pass over tiles that share their target; sw_local.hip: kernel B, any pair in int32 with ends, begin and CIGAR).  The entry's lock and
// refusals are sw_stage_host.h's; the two runs keep their own workspace calls (a failed step of theirs leaves the workspace as it is).
#include "../../include/mgl_sw.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sw_local.h"
#include "sw_stage_host.h"

using namespace mgl_sw_dev;

static_assert(sizeof(mgl_sw_local_hit) == 20 && sizeof(LocalHit) == sizeof(mgl_sw_local_hit), "mgl_sw_local_hit layout");

using namespace mgl_sw_host;

namespace {

#define LOCAL_HIP_TRY(ctx, call)                                     \
    do {                                                             \
        hipError_t e_ = (call);                                      \
        if (e_ != hipSuccess) return ctx_hip_fail(ctx, e_, #call);   \
    } while (0)
#define LOCAL_TRY(call)                  \
    do {                                 \
        const int rc_ = (call);          \
        if (rc_ != MGL_SW_OK) return rc_; \
    } while (0)

constexpr int64_t kMaxPairsPerLaunch = 1 << 20;

// kernel B over the whole batch, chunk by chunk: slots of the largest pair's size (a pair larger than a slot: MGL_SW_ERR_UNSUPPORTED)
int run_pairs(mgl_sw_ctx *ctx, hipStream_t st, LocalArgs a, int64_t n)
{
    const int64_t limit = ctx_workspace_limit(ctx);
    int64_t slot = local_pair_bytes(std::max(a.max_tl, 1), std::max(a.max_ql, 1), a.score_only != 0);
    slot = std::min<int64_t>(slot, std::max<int64_t>(limit, 256) / 256 * 256);
    const int64_t per_chunk = std::max<int64_t>(1, std::min<int64_t>({n, kMaxPairsPerLaunch, std::max<int64_t>(limit, 256) / slot}));
    void *ws = nullptr;
    LOCAL_TRY(ctx_borrow_workspace(ctx, st, (size_t)(per_chunk * slot), &ws));
    a.ws = static_cast<unsigned char *>(ws);
    a.slot_bytes = slot;
    int launches = 0;
    for (int64_t first = 0; first < n; first += per_chunk, ++launches) {
        a.first = first;
        a.count = std::min(per_chunk, n - first);
        LOCAL_HIP_TRY(ctx, launch_local_pairs(a, st));
    }
    return ctx_return_workspace(ctx, st, MGL_SW_KERNEL_LOCAL, launches);
}

constexpr int kNotTaken = -1000;

// kernel A: tiles of 128 pairs, the persistent grid draws them longest target first.  kNotTaken: the workspace cannot give every SIMD
// a wave slot (kernel B then takes the batch)
int run_lane(mgl_sw_ctx *ctx, hipStream_t st, LocalArgs a, int64_t n)
{
    const int64_t tiles = (n + 127) / 128;
    const int64_t region = local_lane_region_bytes(a.max_ql);
    const char *const slots_env = getenv("MGL_SW_DEBUG_LANE_SLOTS"); // (tests: a grid of this many wave slots, read per call)
    const int64_t forced = slots_env ? atoll(slots_env) : 0;
    const int64_t chip = forced > 0 ? forced : (int64_t)ctx_cus(ctx) * 12; // three waves per SIMD (167 registers)
    const int64_t slots = std::min<int64_t>({chip, tiles, ctx_workspace_limit(ctx) / region});
    if (slots < 1 || (forced <= 0 && slots < std::min<int64_t>(tiles, (int64_t)ctx_cus(ctx) * 4))) return kNotTaken;
    // ---- every tile's target length comes back (the one synchronisation of this path) and orders the tiles, longest first
    const size_t geo_bytes = (size_t)tiles * 8, order_off = (geo_bytes + 255) / 256 * 256, total = order_off + (size_t)tiles * 4;
    void *dev = nullptr, *host = nullptr;
    LOCAL_TRY(ctx_tile_buffers(ctx, st, total, &dev, &host));
    unsigned char *const dg = static_cast<unsigned char *>(dev), *const hp = static_cast<unsigned char *>(host);
    void *ws = nullptr;
    LOCAL_TRY(ctx_borrow_workspace(ctx, st, (size_t)(slots * region), &ws)); // (behind the previous call: its kernels read d_grid)
    LOCAL_HIP_TRY(ctx, launch_tile_geometry(a.t, a.q, 0, n, reinterpret_cast<int32_t *>(dg), st));
    LOCAL_HIP_TRY(ctx, hipMemcpyAsync(hp, dg, geo_bytes, hipMemcpyDeviceToHost, st));
    LOCAL_HIP_TRY(ctx, hipStreamSynchronize(st));
    const int32_t *const geo = reinterpret_cast<const int32_t *>(hp);
    int32_t *const order = reinterpret_cast<int32_t *>(hp + order_off);
    for (int64_t k = 0; k < tiles; ++k) order[k] = (int32_t)k;
    std::stable_sort(order, order + tiles, [&](int32_t x, int32_t y) { return geo[2 * (size_t)x] > geo[2 * (size_t)y]; });
    LOCAL_HIP_TRY(ctx, hipMemcpyAsync(dg + order_off, order, (size_t)tiles * 4, hipMemcpyHostToDevice, st));
    a.ws = static_cast<unsigned char *>(ws);
    a.first = 0;
    a.count = n;
    a.tile_order = reinterpret_cast<const int32_t *>(dg + order_off);
    a.lane_slots = (int)slots;
    if (tiles > slots) LOCAL_TRY(ctx_tile_counter(ctx, st, &a.tile_ctr, &a.grid_fault));
    LOCAL_HIP_TRY(ctx, launch_local_lane(a, st));
    return ctx_return_workspace(ctx, st, MGL_SW_KERNEL_LOCAL_LANE, 1);
}

} // namespace

extern "C" {

int mgl_sw_local_batch_device_matrix(mgl_sw_ctx *ctx, void *stream, int64_t n, const uint8_t *d_targets, const int64_t *d_t_start,
                                     const int32_t *d_t_len, const uint8_t *d_queries, const int64_t *d_q_start, const int32_t *d_q_len,
                                     int max_tl, int max_ql, const int8_t *matrix, const uint8_t *code, int gopen, int gext,
                                     mgl_sw_local_hit *d_hit_out, char *d_cigar_out, int cigar_stride, int32_t *d_cigar_len_out,
                                     int32_t *d_status_out, int flags)
{
    const bool score_only = (flags & MGL_SW_FLAG_SCORE_ONLY) != 0, binary = (flags & MGL_SW_FLAG_BINARY_CIGAR) != 0;
    // ---- arguments first: nothing below touches a device before they are known good
    const char *bad = nullptr;
    if (n < 0) bad = "n < 0";
    else if (!matrix || !code) bad = "null matrix or code table";
    else if (max_tl < 0 || max_ql < 0) bad = "max_tl / max_ql < 0";
    else if (!score_only && (!d_cigar_out || !d_cigar_len_out || cigar_stride < (binary ? 4 : 2))) bad = "CIGAR array missing or cigar_stride too small";
    else if (n > 0 && (!d_targets || !d_t_start || !d_t_len || !d_queries || !d_q_start || !d_q_len || !d_hit_out)) bad = "null sequence, length or hit array";
    if (!bad) {
        for (int k = 0; k < 256; ++k)
            if (code[k] >= MATRIX_DIM) bad = "code >= 32";
        if (gopen == INT32_MIN || gext == INT32_MIN || std::abs(gopen) > (1 << 24) || std::abs(gext) > (1 << 24)) bad = "gap penalty beyond 2^24";
    }
    if (bad) return refuse(ctx, "mgl_sw_local_batch_device_matrix", bad);
    if (!ctx) return no_context();
    Stage stage(ctx, stream);
    if (n == 0) return MGL_SW_OK;
    gopen = std::abs(gopen);
    gext = std::abs(gext);
    int smin = matrix[0], smax = matrix[0];
    for (int k = 0; k < MATRIX_DIM * MATRIX_DIM; ++k) {
        smin = std::min<int>(smin, matrix[k]);
        smax = std::max<int>(smax, matrix[k]);
    }
    hipStream_t st = stage.st;
    int8_t *dm = nullptr;
    uint8_t *dc = nullptr;
    LOCAL_TRY(ctx_stage_matrix(ctx, st, matrix, code, &dm, &dc));
    LocalArgs a{};
    a.t = SeqSet{d_targets, d_t_start, d_t_len, max_tl, 0};
    a.q = SeqSet{d_queries, d_q_start, d_q_len, max_ql, 0};
    a.gopen = gopen;
    a.gext = gext;
    a.smin = smin;
    a.smax = smax;
    a.max_tl = max_tl;
    a.max_ql = max_ql;
    a.matrix = dm;
    a.code = dc;
    a.hit = reinterpret_cast<LocalHit *>(d_hit_out);
    a.status = d_status_out;
    a.cigar = d_cigar_out;
    a.cigar_stride = cigar_stride;
    a.cigar_len = d_cigar_len_out;
    a.binary_cigar = binary ? 1 : 0;
    a.score_only = score_only ? 1 : 0;
    try { // (the tiles' order is sorted on the host: no C++ exception crosses the C ABI)
        // the planner rule: a score pass over tiles that share their target, with a status array for a broken promise, inside kernel
        // A's range guard -> kernel A; everything else -> kernel B
        if ((flags & MGL_SW_FLAG_SHARED_TARGET) && score_only && d_status_out && local_lane_ok(smin, smax, gopen, gext, max_tl, max_ql)) {
            const int rc = run_lane(ctx, st, a, n);
            if (rc != kNotTaken) return rc;
        }
        return run_pairs(ctx, st, a, n);
    } catch (const std::exception &) {
        return ctx_fail(ctx, MGL_SW_ERR_NOMEM, "mgl_sw_local_batch_device_matrix: out of host memory");
    }
}

} // extern "C"
