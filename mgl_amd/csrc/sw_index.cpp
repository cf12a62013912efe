// sw_index.cpp -- the minimizer index of one reference (mgl_sw_index_build_device, _build_contigs_device, _destroy, _get_info,
// _get_contigs, _export_device), the contig of an anchor (mgl_sw_index_contig_of_batch_device, and the window inside a contig,
// mgl_sw_locate_window_contigs_batch_device: DESIGN.md section 9m), the seed stage
// that probes it (mgl_sw_seed_index_batch_device) and the stage that turns a read's chain into a window of the reference
// (mgl_sw_locate_window_batch_device): include/mgl_sw.h, DESIGN.md section 9j.  Host side only: argument checks, the index's own
// allocations, one workspace for the seed stage, launches on the caller's stream.  The build synchronises the stream -- it has to
// learn the number of entries before it allocates them --; the two batch entries do not.  The batch entries' frame is sw_stage_host.h's.
#include "../../include/mgl_sw.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <mutex>
#include <new>
#include <vector>

#include "sw_index.h"
#include "sw_stage_host.h"

using namespace mgl_sw_dev;
using namespace mgl_sw_host;

struct mgl_sw_index {
    int device = 0;
    int64_t ref_len = 0, entries = 0, bytes = 0;
    int k = 0, w = 0, bucket_bits = 0;
    uint32_t *keys = nullptr;   // entries (at least one allocated)
    int32_t *pos = nullptr;
    uint32_t *bucket = nullptr; // 2^bucket_bits + 1
    // ---- the contig table (mgl_sw_index_build_contigs_device); n_contigs = 0: none, one contig [0, ref_len)
    int64_t n_contigs = 0;
    int32_t *contigs = nullptr;         // device: n_contigs starts, then n_contigs ends
    std::vector<int64_t> contig_start;  // host, as the caller gave them
    std::vector<int64_t> contig_len;
};

namespace {

// device memory that lives no longer than the build
struct Scratch {
    void *p = nullptr;
    ~Scratch()
    {
        if (p) (void)hipFree(p);
    }
    hipError_t get(size_t bytes) { return hipMalloc(&p, std::max<size_t>(bytes, 256)); }
};

int bucket_bits_for(int64_t entries, int k)
{
    int bits = INDEX_MIN_BUCKET_BITS;
    while (bits < INDEX_MAX_BUCKET_BITS && ((int64_t)1 << bits) < entries) ++bits;
    return std::min(bits, 2 * k);
}

IndexView view_of(const mgl_sw_index *idx)
{
    IndexView v{};
    v.keys = idx->keys;
    v.pos = idx->pos;
    v.bucket = idx->bucket;
    v.ref_len = idx->ref_len;
    v.entries = idx->entries;
    v.k = idx->k;
    v.w = idx->w;
    v.bucket_bits = idx->bucket_bits;
    return v;
}

ContigView contigs_of(const mgl_sw_index *idx)
{
    ContigView v{};
    v.start = idx->contigs;
    v.end = idx->contigs ? idx->contigs + idx->n_contigs : nullptr;
    v.n = (int32_t)idx->n_contigs;
    v.ref_len = (int32_t)idx->ref_len;
    return v;
}

} // namespace

extern "C" {

int mgl_sw_index_build_device(mgl_sw_ctx *ctx, void *stream, const uint8_t *d_ref, int64_t ref_len, int k, int w, mgl_sw_index **out)
{
    if (out) *out = nullptr;
    const char *bad = nullptr;
    if (!out) bad = "null out";
    else if (!d_ref) bad = "null reference";
    else if (ref_len < 1 || ref_len > INDEX_MAX_REF) bad = "ref_len outside 1 .. 2^31 - 1";
    else if (k < SEED_MIN_K || k > SEED_MAX_K) bad = "k outside 4 .. 16";
    else if (w < 1 || w > SEED_MAX_W) bad = "w outside 1 .. 32";
    if (bad) return refuse(ctx, "mgl_sw_index_build_device", bad);
    if (!ctx) return no_context();
    std::lock_guard<std::mutex> lk(ctx_mutex(ctx));
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t he = hipSetDevice(ctx_device(ctx));
    if (he != hipSuccess) return ctx_hip_fail(ctx, he, "hipSetDevice");

    mgl_sw_index *idx = new (std::nothrow) mgl_sw_index;
    if (!idx) return ctx_fail(ctx, MGL_SW_ERR_NOMEM, "mgl_sw_index_build_device: no memory for the handle");
    idx->device = ctx_device(ctx);
    idx->ref_len = ref_len;
    idx->k = k;
    idx->w = w;
    auto give_up = [&](hipError_t e, const char *where) {
        mgl_sw_index_destroy(idx);
        return ctx_hip_fail(ctx, e, where);
    };

    // ---- pass 1: a count per block of SEED_BLOCK positions, their prefix sum, and M comes back
    IndexBuildArgs a{};
    a.ref = d_ref;
    a.ref_len = ref_len;
    a.k = k;
    a.w = w;
    const int64_t nk = ref_len - k + 1;
    a.blocks = nk > 0 ? (nk + SEED_BLOCK - 1) / SEED_BLOCK : 0;
    Scratch counts, entries, sorted;
    if ((he = counts.get((size_t)(2 * a.blocks + 1) * 4)) != hipSuccess) return give_up(he, "hipMalloc (block counts)");
    a.block_count = static_cast<uint32_t *>(counts.p);
    a.block_start = a.block_count + a.blocks;
    if ((he = launch_index_count(a, st)) != hipSuccess) return give_up(he, "launch_index_count");
    if ((he = launch_index_scan(a, st)) != hipSuccess) return give_up(he, "launch_index_scan");
    uint32_t m32 = 0;
    if ((he = hipMemcpyAsync(&m32, a.block_start + a.blocks, 4, hipMemcpyDeviceToHost, st)) != hipSuccess) return give_up(he, "hipMemcpyAsync (entries)");
    if ((he = hipStreamSynchronize(st)) != hipSuccess) return give_up(he, "hipStreamSynchronize (entries)");
    const int64_t m = m32;
    idx->entries = m;
    idx->bucket_bits = bucket_bits_for(m, k);
    const size_t bucket_bytes = (((size_t)1 << idx->bucket_bits) + 1) * 4;
    idx->bytes = m * 8 + (int64_t)bucket_bytes;

    // ---- the index's own memory, exactly M entries; pass 2, the sort, the split, the buckets
    if ((he = hipMalloc(reinterpret_cast<void **>(&idx->keys), (size_t)std::max<int64_t>(m, 1) * 4)) != hipSuccess) return give_up(he, "hipMalloc (keys)");
    if ((he = hipMalloc(reinterpret_cast<void **>(&idx->pos), (size_t)std::max<int64_t>(m, 1) * 4)) != hipSuccess) return give_up(he, "hipMalloc (positions)");
    if ((he = hipMalloc(reinterpret_cast<void **>(&idx->bucket), bucket_bytes)) != hipSuccess) return give_up(he, "hipMalloc (buckets)");
    if (m > 0) {
        if ((he = entries.get((size_t)m * 8)) != hipSuccess) return give_up(he, "hipMalloc (entries)");
        if ((he = sorted.get((size_t)m * 8)) != hipSuccess) return give_up(he, "hipMalloc (sorted entries)");
        a.entries = static_cast<uint64_t *>(entries.p);
        if ((he = launch_index_write(a, st)) != hipSuccess) return give_up(he, "launch_index_write");
        if ((he = index_sort_entries(a.entries, static_cast<uint64_t *>(sorted.p), m, k, st)) != hipSuccess) return give_up(he, "index_sort_entries");
        if ((he = launch_index_split(static_cast<const uint64_t *>(sorted.p), m, idx->keys, idx->pos, st)) != hipSuccess) return give_up(he, "launch_index_split");
    }
    if ((he = launch_index_buckets(idx->keys, m, k, idx->bucket_bits, idx->bucket, st)) != hipSuccess) return give_up(he, "launch_index_buckets");
    if ((he = hipStreamSynchronize(st)) != hipSuccess) return give_up(he, "hipStreamSynchronize (build)"); // (the scratch is freed on return)
    *out = idx;
    return MGL_SW_OK;
}

void mgl_sw_index_destroy(mgl_sw_index *idx)
{
    if (!idx) return;
    int was = -1;
    const bool moved = hipGetDevice(&was) == hipSuccess && was != idx->device && hipSetDevice(idx->device) == hipSuccess;
    for (void *p : {static_cast<void *>(idx->keys), static_cast<void *>(idx->pos), static_cast<void *>(idx->bucket), static_cast<void *>(idx->contigs)})
        if (p) (void)hipFree(p);
    if (moved) (void)hipSetDevice(was);
    delete idx;
}

int mgl_sw_index_build_contigs_device(mgl_sw_ctx *ctx, void *stream, const uint8_t *d_ref, int64_t ref_len, const int64_t *contig_start,
                                      const int64_t *contig_len, int64_t n_contigs, int k, int w, mgl_sw_index **out)
{
    static const char *const entry = "mgl_sw_index_build_contigs_device";
    if (out) *out = nullptr;
    const char *bad = nullptr;
    if (!out) bad = "null out";
    else if (!d_ref) bad = "null reference";
    else if (ref_len < 1 || ref_len > INDEX_MAX_REF) bad = "ref_len outside 1 .. 2^31 - 1";
    else if (k < SEED_MIN_K || k > SEED_MAX_K) bad = "k outside 4 .. 16";
    else if (w < 1 || w > SEED_MAX_W) bad = "w outside 1 .. 32";
    else if (!contig_start || !contig_len) bad = "null contig array";
    else if (n_contigs < 1 || n_contigs > CONTIG_MAX) bad = "n_contigs outside 1 .. 2^20";
    else if (contig_start[0] != 0) bad = "the first contig does not start at 0";
    else {
        for (int64_t c = 0; c < n_contigs && !bad; ++c) {
            const int64_t s = contig_start[c], l = contig_len[c];
            if (s < 0 || s >= ref_len) bad = "a contig starts outside the reference";
            else if (l < 1 || l > ref_len - s) bad = "a contig's length is below 1 or leaves the reference";
            else if (c + 1 < n_contigs && s + l >= contig_start[c + 1]) bad = "no gap byte between two contigs";
            else if (c + 1 == n_contigs && s + l != ref_len) bad = "the last contig does not end at ref_len";
        }
    }
    if (bad) return refuse(ctx, entry, bad);
    if (!ctx) return no_context();

    // ---- the table on the device and the gap bytes looked at, under the context's lock; the build below takes it again
    std::vector<int32_t> table((size_t)(2 * n_contigs));
    for (int64_t c = 0; c < n_contigs; ++c) {
        table[(size_t)c] = (int32_t)contig_start[c];
        table[(size_t)(n_contigs + c)] = (int32_t)(contig_start[c] + contig_len[c]);
    }
    int32_t *d_table = nullptr;
    {
        std::lock_guard<std::mutex> lk(ctx_mutex(ctx));
        hipStream_t st = static_cast<hipStream_t>(stream);
        hipError_t he = hipSetDevice(ctx_device(ctx));
        if (he != hipSuccess) return ctx_hip_fail(ctx, he, "hipSetDevice");
        Scratch flag;
        if ((he = flag.get(4)) != hipSuccess) return ctx_hip_fail(ctx, he, "hipMalloc (gap flag)");
        if ((he = hipMalloc(reinterpret_cast<void **>(&d_table), table.size() * 4)) != hipSuccess) return ctx_hip_fail(ctx, he, "hipMalloc (contig table)");
        auto give_up = [&](hipError_t e, const char *where) {
            (void)hipFree(d_table);
            return ctx_hip_fail(ctx, e, where);
        };
        ContigView cv{d_table, d_table + n_contigs, (int32_t)n_contigs, (int32_t)ref_len};
        int32_t base_in_gap = 0;
        if ((he = hipMemcpyAsync(d_table, table.data(), table.size() * 4, hipMemcpyHostToDevice, st)) != hipSuccess) return give_up(he, "hipMemcpyAsync (contig table)");
        if ((he = hipMemsetAsync(flag.p, 0, 4, st)) != hipSuccess) return give_up(he, "hipMemsetAsync (gap flag)");
        if ((he = launch_contig_gaps(d_ref, cv, static_cast<int32_t *>(flag.p), st)) != hipSuccess) return give_up(he, "launch_contig_gaps");
        if ((he = hipMemcpyAsync(&base_in_gap, flag.p, 4, hipMemcpyDeviceToHost, st)) != hipSuccess) return give_up(he, "hipMemcpyAsync (gap flag)");
        if ((he = hipStreamSynchronize(st)) != hipSuccess) return give_up(he, "hipStreamSynchronize (gaps)");
        if (base_in_gap) {
            (void)hipFree(d_table);
            return ctx_fail(ctx, MGL_SW_ERR_BAD_ARG, "mgl_sw_index_build_contigs_device: a gap between two contigs holds a base");
        }
    }

    // ---- the existing build as it is; the handle takes the table
    mgl_sw_index *idx = nullptr;
    const int rc = mgl_sw_index_build_device(ctx, stream, d_ref, ref_len, k, w, &idx);
    if (rc != MGL_SW_OK) {
        (void)hipFree(d_table);
        return rc;
    }
    idx->n_contigs = n_contigs;
    idx->contigs = d_table;
    idx->contig_start.assign(contig_start, contig_start + n_contigs);
    idx->contig_len.assign(contig_len, contig_len + n_contigs);
    *out = idx;
    return MGL_SW_OK;
}

int mgl_sw_index_get_contigs(const mgl_sw_index *idx, int64_t capacity, int64_t *start_out, int64_t *len_out, int64_t *n_out)
{
    if (!idx || !n_out) return MGL_SW_ERR_BAD_ARG;
    const int64_t n = idx->n_contigs > 0 ? idx->n_contigs : 1;
    *n_out = n;
    if (!start_out && !len_out && capacity == 0) return MGL_SW_OK; // a sizing call
    if (!start_out || !len_out || capacity < n) return MGL_SW_ERR_BAD_ARG;
    if (idx->n_contigs == 0) {
        start_out[0] = 0;
        len_out[0] = idx->ref_len;
    } else {
        std::copy(idx->contig_start.begin(), idx->contig_start.end(), start_out);
        std::copy(idx->contig_len.begin(), idx->contig_len.end(), len_out);
    }
    return MGL_SW_OK;
}

int mgl_sw_index_get_info(const mgl_sw_index *idx, mgl_sw_index_info *out)
{
    if (!idx || !out) return MGL_SW_ERR_BAD_ARG;
    out->ref_len = idx->ref_len;
    out->entries = idx->entries;
    out->bytes = idx->bytes;
    out->k = idx->k;
    out->w = idx->w;
    return MGL_SW_OK;
}

int mgl_sw_index_export_device(const mgl_sw_index *idx, void *stream, uint32_t *d_keys_out, int32_t *d_pos_out, int64_t capacity)
{
    if (!idx || !d_keys_out || !d_pos_out || capacity < idx->entries) return MGL_SW_ERR_BAD_ARG;
    if (idx->entries == 0) return MGL_SW_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // no context here, so no lock and no error text; the caller's current device is put back, as mgl_sw_index_destroy does
    int was = -1;
    const bool moved = hipGetDevice(&was) == hipSuccess && was != idx->device;
    if (moved && hipSetDevice(idx->device) != hipSuccess) return MGL_SW_ERR_DEVICE;
    const bool ok = hipMemcpyAsync(d_keys_out, idx->keys, (size_t)idx->entries * 4, hipMemcpyDeviceToDevice, st) == hipSuccess &&
                    hipMemcpyAsync(d_pos_out, idx->pos, (size_t)idx->entries * 4, hipMemcpyDeviceToDevice, st) == hipSuccess;
    if (moved) (void)hipSetDevice(was);
    return ok ? MGL_SW_OK : MGL_SW_ERR_DEVICE;
}

int mgl_sw_seed_index_batch_device(mgl_sw_ctx *ctx, void *stream, const mgl_sw_index *idx, int64_t n, const uint8_t *d_queries, const int64_t *d_q_start,
                                   const int32_t *d_q_len, int strands, int max_occ, int max_occ_ref, int merge, int max_cand, int64_t cand_capacity,
                                   int64_t *d_cand_start_out, int32_t *d_cand_t_out, int32_t *d_cand_q_out, int32_t *d_cand_len_out,
                                   int32_t *d_row_t_len_out, int32_t *d_row_q_len_out, int32_t *d_status_out)
{
    // ---- arguments first: nothing below touches a device before they are known good
    const char *bad = nullptr;
    if (!idx) bad = "null index";
    else if (strands != 1 && strands != 2) bad = "strands is neither 1 nor 2";
    else if (n < 0 || n > SEED_MAX_PAIRS / strands) bad = "n outside 0 .. 2^30 / strands";
    else if (!d_queries || !d_q_start || !d_q_len) bad = "null query array";
    else if (!d_cand_start_out || !d_cand_t_out || !d_cand_q_out || !d_cand_len_out) bad = "null candidate array";
    else if (max_occ < 1 || max_occ > SEED_MAX_OCC) bad = "max_occ outside 1 .. 64";
    else if (max_occ_ref < 1 || max_occ_ref > INDEX_MAX_OCC_REF) bad = "max_occ_ref outside 1 .. 8192";
    else if (merge != 0 && merge != 1) bad = "merge is neither 0 nor 1";
    else if (max_cand < 1 || max_cand > SEED_MAX_CAND) bad = "max_cand outside 1 .. 8192";
    else if (cand_capacity < 0 || cand_capacity > SEED_MAX_PAIRS) bad = "cand_capacity outside 0 .. 2^30";
    if (bad) return refuse(ctx, "mgl_sw_seed_index_batch_device", bad);
    if (!ctx) return no_context();
    // there is no kernel id for this stage: the timing record keeps the fill_kernel it has (Stage's default)
    Stage stage(ctx, stream);
    hipStream_t st = stage.st;
    if (idx->device != ctx_device(ctx)) return ctx_fail(ctx, MGL_SW_ERR_BAD_ARG, "mgl_sw_seed_index_batch_device: the index lives on another device");

    // ---- one workspace: the counts and the staging of the rows, then one slot per workgroup
    const int64_t rows = strands * n;
    const int64_t limit = stage.limit();
    const SeedWorkspace sg = seed_workspace(rows, max_cand);
    const int64_t room = limit - sg.bytes;
    if (room < sg.slot_bytes)
        return ctx_fail(ctx, MGL_SW_ERR_NOMEM,
                        "mgl_sw_seed_index_batch_device: the workspace limit does not hold the staging of the batch's rows beside a slot: split the batch");
    const int64_t groups = std::min(std::min<int64_t>(std::max<int64_t>(n, 1), (int64_t)ctx_cus(ctx) * SEED_GROUPS_PER_CU), room / sg.slot_bytes);
    unsigned char *ws = nullptr;
    const int rc = stage.borrow((size_t)(sg.bytes + groups * sg.slot_bytes), &ws);
    if (rc != MGL_SW_OK) return rc;

    SeedIndexArgs aa{};
    aa.ix = view_of(idx);
    aa.strands = strands;
    aa.max_occ_ref = max_occ_ref;
    aa.row_t_len = d_row_t_len_out;
    aa.row_q_len = d_row_q_len_out;
    SeedStageArgs &a = aa.s;
    a.queries = d_queries;
    a.q_start = d_q_start;
    a.q_len = d_q_len;
    a.n = rows;
    a.cand_capacity = cand_capacity;
    a.k = idx->k;
    a.w = idx->w;
    a.max_occ = max_occ;
    a.merge = merge;
    a.max_cand = max_cand;
    a.ws = ws;
    a.groups = (int)groups;
    a.cand_start = d_cand_start_out;
    a.cand_t = d_cand_t_out;
    a.cand_q = d_cand_q_out;
    a.cand_len = d_cand_len_out;
    a.status = d_status_out;

    hipError_t he = launch_seed_index(aa, st);
    if (he != hipSuccess) return stage.fail(he, "launch_seed_index");
    // the scan and the pack of the seed stage read nothing but the rows' counts and staging: they serve these rows as they are
    he = launch_seed_scan(a, st);
    if (he != hipSuccess) return stage.fail(he, "launch_seed_scan");
    he = launch_seed_pack(a, st);
    if (he != hipSuccess) return stage.fail(he, "launch_seed_pack");
    return stage.done();
}

int mgl_sw_locate_window_batch_device(mgl_sw_ctx *ctx, void *stream, int64_t n, int64_t ref_len, const int32_t *d_q_len, const int64_t *d_anchor_start,
                                      const int32_t *d_anchor_t, const int32_t *d_anchor_q, const int32_t *d_anchor_len, int64_t total_anchors, int slack,
                                      int max_tl, int64_t *d_t_start_out, int32_t *d_t_len_out, int32_t *d_anchor_t_out, int32_t *d_status_out)
{
    const char *bad = nullptr;
    if (n < 0 || n > SEED_MAX_PAIRS) bad = "n outside 0 .. 2^30";
    else if (ref_len < 1 || ref_len > INDEX_MAX_REF) bad = "ref_len outside 1 .. 2^31 - 1";
    else if (!d_q_len || !d_anchor_start) bad = "null read array";
    else if (!d_anchor_t || !d_anchor_q || !d_anchor_len) bad = "null anchor array";
    else if (total_anchors < 0 || total_anchors > SEED_MAX_PAIRS) bad = "total_anchors outside 0 .. 2^30";
    else if (slack < 0) bad = "slack below 0";
    else if (max_tl < 1) bad = "max_tl below 1";
    else if (!d_t_start_out || !d_t_len_out || !d_anchor_t_out) bad = "null output array";
    if (bad) return refuse(ctx, "mgl_sw_locate_window_batch_device", bad);
    if (!ctx) return no_context();
    Stage stage(ctx, stream);
    hipError_t he = hipSetDevice(ctx_device(ctx));
    if (he != hipSuccess) return stage.fail(he, "hipSetDevice");

    LocateArgs a{};
    a.q_len = d_q_len;
    a.anchor_start = d_anchor_start;
    a.anchor_t = d_anchor_t;
    a.anchor_q = d_anchor_q;
    a.anchor_len = d_anchor_len;
    a.n = n;
    a.ref_len = ref_len;
    a.total_anchors = total_anchors;
    a.slack = slack;
    a.max_tl = max_tl;
    a.t_start = d_t_start_out;
    a.t_len = d_t_len_out;
    a.anchor_t_out = d_anchor_t_out;
    a.status = d_status_out;
    he = launch_locate_window(a, stage.st);
    if (he != hipSuccess) return stage.fail(he, "launch_locate_window");
    return stage.done(); // (no workspace: the timing record is not touched)
}

int mgl_sw_index_contig_of_batch_device(mgl_sw_ctx *ctx, void *stream, const mgl_sw_index *idx, int64_t total, const int32_t *d_t, const int32_t *d_len,
                                        int32_t *d_group_out)
{
    static const char *const entry = "mgl_sw_index_contig_of_batch_device";
    const char *bad = nullptr;
    if (!idx) bad = "null index";
    else if (total < 0 || total > SEED_MAX_PAIRS) bad = "total outside 0 .. 2^30";
    else if (!d_t || !d_len || !d_group_out) bad = "null array";
    if (bad) return refuse(ctx, entry, bad);
    if (!ctx) return no_context();
    Stage stage(ctx, stream);
    if (idx->device != ctx_device(ctx)) return ctx_fail(ctx, MGL_SW_ERR_BAD_ARG, "mgl_sw_index_contig_of_batch_device: the index lives on another device");
    hipError_t he = hipSetDevice(ctx_device(ctx));
    if (he != hipSuccess) return stage.fail(he, "hipSetDevice");
    ContigOfArgs a{};
    a.cv = contigs_of(idx);
    a.total = total;
    a.t = d_t;
    a.len = d_len;
    a.group = d_group_out;
    he = launch_contig_of(a, stage.st);
    if (he != hipSuccess) return stage.fail(he, "launch_contig_of");
    return stage.done(); // (no workspace: the timing record is not touched)
}

int mgl_sw_locate_window_contigs_batch_device(mgl_sw_ctx *ctx, void *stream, int64_t n, const mgl_sw_index *idx, const int32_t *d_q_len,
                                              const int64_t *d_anchor_start, const int32_t *d_anchor_t, const int32_t *d_anchor_q,
                                              const int32_t *d_anchor_len, int64_t total_anchors, int slack, int max_tl, int64_t *d_t_start_out,
                                              int32_t *d_t_len_out, int32_t *d_anchor_t_out, int32_t *d_rid_out, int32_t *d_status_out)
{
    static const char *const entry = "mgl_sw_locate_window_contigs_batch_device";
    const char *bad = nullptr;
    if (n < 0 || n > SEED_MAX_PAIRS) bad = "n outside 0 .. 2^30";
    else if (!idx) bad = "null index";
    else if (!d_q_len || !d_anchor_start) bad = "null read array";
    else if (!d_anchor_t || !d_anchor_q || !d_anchor_len) bad = "null anchor array";
    else if (total_anchors < 0 || total_anchors > SEED_MAX_PAIRS) bad = "total_anchors outside 0 .. 2^30";
    else if (slack < 0) bad = "slack below 0";
    else if (max_tl < 1) bad = "max_tl below 1";
    else if (!d_t_start_out || !d_t_len_out || !d_anchor_t_out || !d_rid_out) bad = "null output array";
    if (bad) return refuse(ctx, entry, bad);
    if (!ctx) return no_context();
    Stage stage(ctx, stream);
    if (idx->device != ctx_device(ctx)) return ctx_fail(ctx, MGL_SW_ERR_BAD_ARG, "mgl_sw_locate_window_contigs_batch_device: the index lives on another device");
    hipError_t he = hipSetDevice(ctx_device(ctx));
    if (he != hipSuccess) return stage.fail(he, "hipSetDevice");

    LocateContigsArgs aa{};
    LocateArgs &a = aa.l;
    a.q_len = d_q_len;
    a.anchor_start = d_anchor_start;
    a.anchor_t = d_anchor_t;
    a.anchor_q = d_anchor_q;
    a.anchor_len = d_anchor_len;
    a.n = n;
    a.ref_len = idx->ref_len;
    a.total_anchors = total_anchors;
    a.slack = slack;
    a.max_tl = max_tl;
    a.t_start = d_t_start_out;
    a.t_len = d_t_len_out;
    a.anchor_t_out = d_anchor_t_out;
    a.status = d_status_out;
    aa.cv = contigs_of(idx);
    aa.rid = d_rid_out;
    he = launch_locate_window_contigs(aa, stage.st);
    if (he != hipSuccess) return stage.fail(he, "launch_locate_window_contigs");
    return stage.done(); // (no workspace: the timing record is not touched)
}

} // extern "C"
