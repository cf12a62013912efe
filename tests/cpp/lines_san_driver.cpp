// lines_san_driver.cpp -- the host side of mgl_sw_expand_chains_batch_device and mgl_sw_classify_alignments_batch_device
// (mgl_amd/csrc/sw_lines.cpp) under -fsanitize=address,undefined against the fake HIP runtime (fake_hip/): every call-level refusal on
// both sides of its edge, with and without a context, and one accepted call of each entry, whose "launches" are the stand-ins below --
// they check the arguments the host side hands to the kernels (the workspace's parts inside the borrowed region and apart from one
// another, the grid) and touch every byte of the workspace.  TEST-ONLY; make -C tests/cpp -f lines_san.mk lines-san.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mgl_sw.h"
#include "../../mgl_amd/csrc/sw_lines.h"

#define CHECK(x)                                                                        \
    do {                                                                                \
        if (!(x)) {                                                                     \
            std::fprintf(stderr, "lines_san_driver.cpp:%d: CHECK failed: %s\n", __LINE__, #x); \
            std::exit(1);                                                               \
        }                                                                               \
    } while (0)

namespace mgl_sw_dev {

static int expand_launches = 0, classify_launches = 0;

hipError_t launch_expand_count(const ExpandArgs &a, hipStream_t)
{
    // the workspace: four parts, ascending, each holding its n entries
    CHECK(a.ws_jobs && a.ws_anchors && a.ws_strands && a.ws_anchor_at);
    CHECK(reinterpret_cast<unsigned char *>(a.ws_anchors) >= reinterpret_cast<unsigned char *>(a.ws_jobs + a.n));
    CHECK(reinterpret_cast<unsigned char *>(a.ws_strands) >= reinterpret_cast<unsigned char *>(a.ws_anchors + a.n));
    CHECK(reinterpret_cast<unsigned char *>(a.ws_anchor_at) >= reinterpret_cast<unsigned char *>(a.ws_strands + a.n));
    CHECK(reinterpret_cast<uintptr_t>(a.ws_anchor_at) % 8 == 0);
    for (int64_t p = 0; p < a.n; ++p) a.ws_jobs[p] = 1, a.ws_anchors[p] = 2, a.ws_strands[p] = 3, a.ws_anchor_at[p] = 2 * p; // (ASan: inside the borrowed region)
    ++expand_launches;
    return hipSuccess;
}
hipError_t launch_expand_scan(const ExpandArgs &a, hipStream_t)
{
    a.n_jobs[0] = a.n;
    for (int64_t p = 0; p <= a.n; ++p) a.job_start[p] = p;
    ++expand_launches;
    return hipSuccess;
}
hipError_t launch_expand_pack(const ExpandArgs &a, hipStream_t)
{
    for (int64_t j = 0; j < a.job_capacity; ++j) a.jobs[j] = mgl_sw_job{-1, 0, 0, 0, 0, 0, 0, 0}, a.job_q_start[j] = 0, a.job_q_len[j] = 0;
    for (int64_t j = 0; j <= a.job_capacity; ++j) a.job_anchor_start[j] = 0;
    ++expand_launches;
    return hipSuccess;
}
hipError_t launch_expand_orient(const ExpandArgs &a, hipStream_t)
{
    CHECK(a.groups >= 1 && a.groups <= 2 * (a.n > 0 ? a.n : 1));
    std::memset(a.oriented, 'N', (size_t)(2 * a.query_bytes));
    ++expand_launches;
    return hipSuccess;
}
hipError_t launch_classify(const ClassifyArgs &a, hipStream_t)
{
    for (int64_t p = 0; p < a.n; ++p) a.n_lines[p] = 0, a.primary_job[p] = -1;
    if (a.status)
        for (int64_t p = 0; p < a.n; ++p) a.status[p] = 0;
    ++classify_launches;
    return hipSuccess;
}

} // namespace mgl_sw_dev

namespace {

struct Buffers {
    static constexpr int64_t n = 3, cap = 12, total = 40, qbytes = 100;
    std::vector<uint8_t> queries = std::vector<uint8_t>(qbytes, 'A'), oriented = std::vector<uint8_t>(2 * qbytes);
    std::vector<int64_t> q_start = {0, 30, 60}, ranked_start = {0, 10, 20, 40}, n_jobs = {0}, job_start = std::vector<int64_t>(n + 1),
                         job_q_start = std::vector<int64_t>(cap), job_anchor_start = std::vector<int64_t>(cap + 1);
    std::vector<int32_t> q_len = {30, 30, 40}, rank_status = {0, 0, 0}, n_chains = {1, 1, 1}, ranked = std::vector<int32_t>(total), job_q_len = std::vector<int32_t>(cap),
                         anchors = std::vector<int32_t>(total), status = std::vector<int32_t>(n), aln_status = std::vector<int32_t>(cap),
                         n_lines = std::vector<int32_t>(n), primary = std::vector<int32_t>(n);
    std::vector<mgl_sw_ranked_chain> records = std::vector<mgl_sw_ranked_chain>(n * 4);
    std::vector<mgl_sw_job> jobs = std::vector<mgl_sw_job>(cap);
    std::vector<mgl_sw_chain_alignment> aln = std::vector<mgl_sw_chain_alignment>(cap);
    std::vector<mgl_sw_line> lines = std::vector<mgl_sw_line>(cap);
};

struct ExpandCall {
    int64_t n = Buffers::n, query_bytes = Buffers::qbytes, total = Buffers::total, cap = Buffers::cap;
    int max_chains = 4, keep = 1;
    int null_at = -1;            // which of the 19 required pointers is null
    bool rank_status = true, status = true;
    uint8_t *oriented = nullptr; // another place for the oriented buffer
};

int expand(mgl_sw_ctx *ctx, Buffers &b, const ExpandCall &c)
{
    int k = 0;
    auto p = [&](auto *x) { return k++ == c.null_at ? static_cast<decltype(x)>(nullptr) : x; };
    const uint8_t *queries = p(b.queries.data());
    const int64_t *q_start = p(b.q_start.data());
    const int32_t *q_len = p(b.q_len.data()), *n_chains = p(b.n_chains.data());
    const mgl_sw_ranked_chain *records = p(b.records.data());
    const int64_t *ranked_start = p(b.ranked_start.data());
    const int32_t *rt = p(b.ranked.data()), *rq = p(b.ranked.data()), *rl = p(b.ranked.data());
    int64_t *n_jobs = p(b.n_jobs.data()), *job_start = p(b.job_start.data());
    mgl_sw_job *jobs = p(b.jobs.data());
    int64_t *jqs = p(b.job_q_start.data());
    int32_t *jql = p(b.job_q_len.data());
    int64_t *jas = p(b.job_anchor_start.data());
    int32_t *jat = p(b.anchors.data()), *jaq = p(b.anchors.data()), *jal = p(b.anchors.data());
    uint8_t *oriented = p(c.oriented ? c.oriented : b.oriented.data());
    return mgl_sw_expand_chains_batch_device(ctx, nullptr, c.n, queries, q_start, q_len, c.query_bytes, c.rank_status ? b.rank_status.data() : nullptr, n_chains,
                                             records, c.max_chains, ranked_start, rt, rq, rl, c.total, c.keep, c.cap, n_jobs, job_start, jobs, jqs, jql, jas, jat,
                                             jaq, jal, oriented, c.status ? b.status.data() : nullptr);
}

struct ClassifyCall {
    int64_t n = Buffers::n, cap = Buffers::cap;
    int match = 200, min_score = 40, mask_level = 128;
    int null_at = -1; // which of the 7 required pointers is null
    bool status = true;
};

int classify(mgl_sw_ctx *ctx, Buffers &b, const ClassifyCall &c)
{
    int k = 0;
    auto p = [&](auto *x) { return k++ == c.null_at ? static_cast<decltype(x)>(nullptr) : x; };
    const int64_t *job_start = p(b.job_start.data());
    const mgl_sw_job *jobs = p(b.jobs.data());
    const mgl_sw_chain_alignment *aln = p(b.aln.data());
    const int32_t *aln_status = p(b.aln_status.data());
    mgl_sw_line *lines = p(b.lines.data());
    int32_t *n_lines = p(b.n_lines.data()), *primary = p(b.primary.data());
    return mgl_sw_classify_alignments_batch_device(ctx, nullptr, c.n, job_start, jobs, c.cap, aln, aln_status, c.match, c.min_score, c.mask_level, lines, n_lines,
                                                   primary, c.status ? b.status.data() : nullptr);
}

template <typename Call, typename Fn> void edges(mgl_sw_ctx *ctx, Buffers &b, Fn fn, int ok, std::vector<Call> good, std::vector<Call> bad)
{
    for (const Call &c : good) CHECK(fn(ctx, b, c) == ok);
    for (const Call &c : bad) CHECK(fn(ctx, b, c) == MGL_SW_ERR_BAD_ARG);
}

} // namespace

int main()
{
    Buffers b;
    mgl_sw_ctx *ctx = nullptr;
    CHECK(mgl_sw_ctx_create(0, &ctx) == 0);
    // without a context a well-formed call is refused as such (the fake runtime has devices), with one it is accepted
    for (mgl_sw_ctx *c : {(mgl_sw_ctx *)nullptr, ctx}) {
        const int ok = c ? MGL_SW_OK : MGL_SW_ERR_BAD_ARG;
        auto E = [](auto edit) { ExpandCall x; edit(x); return x; };
        std::vector<ExpandCall> good = {ExpandCall{}, E([](ExpandCall &x) { x.n = 0; }), E([](ExpandCall &x) { x.max_chains = 1; }),
                                        E([](ExpandCall &x) { x.max_chains = 16; }), E([](ExpandCall &x) { x.cap = 0; }), E([](ExpandCall &x) { x.total = 0; }),
                                        E([](ExpandCall &x) { x.keep = 0; }), E([](ExpandCall &x) { x.rank_status = false; }), E([](ExpandCall &x) { x.status = false; }),
                                        E([](ExpandCall &x) { x.query_bytes = 0; })};
        std::vector<ExpandCall> bad = {E([](ExpandCall &x) { x.n = -1; }), E([](ExpandCall &x) { x.n = ((int64_t)1 << 29) + 1; }), E([](ExpandCall &x) { x.max_chains = 0; }),
                                       E([](ExpandCall &x) { x.max_chains = 17; }), E([](ExpandCall &x) { x.cap = -1; }), E([](ExpandCall &x) { x.cap = ((int64_t)1 << 30) + 1; }),
                                       E([](ExpandCall &x) { x.total = -1; }), E([](ExpandCall &x) { x.total = ((int64_t)1 << 30) + 1; }),
                                       E([](ExpandCall &x) { x.query_bytes = -1; }), E([](ExpandCall &x) { x.query_bytes = ((int64_t)1 << 40) + 1; }),
                                       E([](ExpandCall &x) { x.keep = 2; })};
        for (int k = 0; k < 19; ++k) bad.push_back(E([k](ExpandCall &x) { x.null_at = k; }));
        // the oriented buffer over the reads': at their first byte, at their last, and ending inside them
        for (int64_t off : {(int64_t)0, Buffers::qbytes - 1}) bad.push_back(E([&b, off](ExpandCall &x) { x.oriented = b.queries.data() + off; }));
        edges<ExpandCall>(c, b, expand, ok, good, bad);

        auto C = [](auto edit) { ClassifyCall x; edit(x); return x; };
        std::vector<ClassifyCall> cgood = {ClassifyCall{}, C([](ClassifyCall &x) { x.n = 0; }), C([](ClassifyCall &x) { x.cap = 0; }),
                                           C([](ClassifyCall &x) { x.mask_level = 1; }), C([](ClassifyCall &x) { x.mask_level = 256; }),
                                           C([](ClassifyCall &x) { x.match = 1; }), C([](ClassifyCall &x) { x.min_score = 1; }), C([](ClassifyCall &x) { x.status = false; })};
        std::vector<ClassifyCall> cbad = {C([](ClassifyCall &x) { x.n = -1; }), C([](ClassifyCall &x) { x.n = ((int64_t)1 << 29) + 1; }), C([](ClassifyCall &x) { x.cap = -1; }),
                                          C([](ClassifyCall &x) { x.cap = ((int64_t)1 << 30) + 1; }), C([](ClassifyCall &x) { x.mask_level = 0; }),
                                          C([](ClassifyCall &x) { x.mask_level = 257; }), C([](ClassifyCall &x) { x.match = 0; }), C([](ClassifyCall &x) { x.min_score = 0; })};
        for (int k = 0; k < 7; ++k) cbad.push_back(C([k](ClassifyCall &x) { x.null_at = k; }));
        edges<ClassifyCall>(c, b, classify, ok, cgood, cbad);
    }
    // a refusal leaves its reason on the context
    ExpandCall x;
    x.max_chains = 17;
    CHECK(expand(ctx, b, x) == MGL_SW_ERR_BAD_ARG);
    CHECK(std::string(mgl_sw_last_error(ctx)) == "mgl_sw_expand_chains_batch_device: max_chains outside 1 .. 16");
    ClassifyCall y;
    y.mask_level = 257;
    CHECK(classify(ctx, b, y) == MGL_SW_ERR_BAD_ARG);
    CHECK(std::string(mgl_sw_last_error(ctx)) == "mgl_sw_classify_alignments_batch_device: mask_level outside 1 .. 256");
    // a workspace limit that does not hold the reads' counts: refused, nothing launched
    const int before = mgl_sw_dev::expand_launches;
    CHECK(mgl_sw_ctx_set_workspace(ctx, 1 << 20) == 0);
    ExpandCall big;
    big.n = 1 << 20; // 20 bytes a read against a limit of 2^20 (nothing is read: the call fails before any launch)
    CHECK(expand(ctx, b, big) == MGL_SW_ERR_NOMEM && mgl_sw_dev::expand_launches == before);
    CHECK(mgl_sw_dev::expand_launches >= 4 * 9 && mgl_sw_dev::classify_launches >= 7);
    mgl_sw_ctx_destroy(ctx);
    std::printf("lines-san ok: %d expand launches, %d classify launches\n", mgl_sw_dev::expand_launches, mgl_sw_dev::classify_launches);
    return 0;
}
