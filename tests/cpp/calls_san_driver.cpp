// calls_san_driver.cpp -- the host side of mgl_sw_pileup_insertions_batch_device and mgl_sw_genotype_sites_device
// (mgl_amd/csrc/sw_calls.cpp) under -fsanitize=address,undefined against the fake HIP runtime (fake_hip/): every call-level refusal on
// both sides of its edge, with and without a context, and accepted calls of each entry, whose "launches" are the stand-ins below --
// they check the arguments the host side hands to the kernels (the grid, the sites, the workspace's parts inside the borrowed region
// and apart from one another) and touch every byte of the workspace.  TEST-ONLY; make -C tests/cpp -f calls_san.mk calls-san.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mgl_sw.h"
#include "../../mgl_amd/csrc/sw_calls.h"

#define CHECK(x)                                                                        \
    do {                                                                                \
        if (!(x)) {                                                                     \
            std::fprintf(stderr, "calls_san_driver.cpp:%d: CHECK failed: %s\n", __LINE__, #x); \
            std::exit(1);                                                               \
        }                                                                               \
    } while (0)

namespace mgl_sw_dev {

static int insertions_launches = 0, genotype_launches = 0;
static const size_t kScanBytes = 1000; // (no multiple of 256: the host side rounds)

hipError_t launch_insertions(const InsertionsArgs &a, hipStream_t)
{
    CHECK(a.n >= 1 && a.groups >= 1 && a.groups <= (a.n + 3) / 4);
    CHECK(a.queries && a.t_start && a.q_start && a.t_len && a.q_len && a.aln && a.cigar && a.cigar_len && a.sites && a.n_sites && a.ins);
    CHECK(a.region_beg >= 0 && a.cigar_stride >= 1 && (a.binary == 0 || a.cigar_stride % 4 == 0));
    CHECK(a.site_capacity >= 1 && a.max_ins >= 1 && a.max_ins <= 64);
    const int64_t S = std::min(std::max<int64_t>(a.n_sites[0], 0), a.site_capacity), W = 6 * a.max_ins + 1;
    for (int64_t p = 0; p < a.n; ++p) {
        if (a.status_in && a.status_in[p]) continue;
        if (a.select && !a.select[p]) continue;
        if (S > 0) a.ins[(p % S) * W + W - 1] += (uint32_t)a.sites[p % S].pos; // (ASan: inside the caller's sites and table)
        if (a.status) a.status[p] = 0;
    }
    ++insertions_launches;
    return hipSuccess;
}

hipError_t genotype_scan_bytes(const int64_t entries, size_t *bytes)
{
    CHECK(entries >= 2 && bytes);
    *bytes = kScanBytes;
    return hipSuccess;
}

hipError_t launch_genotype_count(const GenotypeArgs &g, hipStream_t)
{
    CHECK(g.counts && g.ref && g.sites && g.n_sites && g.n_calls && g.block_count && g.block_start && g.scan_tmp);
    CHECK(g.blocks == (g.site_capacity + CALLS_SITE_BLOCK - 1) / CALLS_SITE_BLOCK && g.scan_bytes >= kScanBytes);
    CHECK(g.max_ins >= 1 && g.max_ins <= 64 && g.max_del >= 1 && g.max_del <= 4096 && 1 <= g.cost_match && g.cost_match < g.cost_het &&
          g.cost_het < g.cost_error && g.cost_error <= (1 << 20));
    // the workspace: three parts, ascending, each holding its entries, each on a 256-byte border
    const unsigned char *c = reinterpret_cast<unsigned char *>(g.block_count), *s = reinterpret_cast<unsigned char *>(g.block_start),
                        *t = static_cast<unsigned char *>(g.scan_tmp);
    CHECK(s >= c + (g.blocks + 1) * 8 && t >= s + (g.blocks + 1) * 8 && (s - c) % 256 == 0 && (t - c) % 256 == 0);
    for (int64_t b = 0; b <= g.blocks; ++b) g.block_count[b] = b < g.blocks ? 1 : 0; // (ASan: inside the borrowed region)
    CHECK(g.ref[0] == 'A' && g.ref[g.region_len - 1] == 'A');
    ++genotype_launches;
    return hipSuccess;
}

hipError_t launch_genotype_scan(const GenotypeArgs &g, hipStream_t)
{
    std::memset(g.scan_tmp, 0x5a, g.scan_bytes);
    int64_t sum = 0;
    for (int64_t b = 0; b <= g.blocks; ++b) g.block_start[b] = sum, sum += g.block_count[b];
    ++genotype_launches;
    return hipSuccess;
}

hipError_t launch_genotype_write(const GenotypeArgs &g, hipStream_t)
{
    CHECK(g.call_capacity == 0 || g.calls);
    CHECK(g.call_capacity == 0 || !g.ins || g.ins_seq);
    g.n_calls[0] = g.block_start[g.blocks];
    for (int64_t k = 0; k < g.call_capacity && k < g.blocks; ++k) {
        mgl_sw_call o{};
        o.pos = (int32_t)(k * CALLS_SITE_BLOCK);
        o.kind = 1;
        g.calls[k] = o;
        if (g.ins_seq) std::memset(g.ins_seq + k * g.max_ins, 0, g.max_ins);
    }
    ++genotype_launches;
    return hipSuccess;
}

} // namespace mgl_sw_dev

namespace {

struct Buffers {
    static constexpr int64_t n = 3, region = 1000, stride = 64, cap = 600, call_cap = 10;
    static constexpr int max_ins = 16;
    std::vector<uint8_t> targets = std::vector<uint8_t>(2 * region, 'A'), queries = std::vector<uint8_t>(300, 'C'),
                         seq = std::vector<uint8_t>(call_cap * 64);
    std::vector<int64_t> t_start = {0, 100, 200}, q_start = {0, 100, 200}, n_sites = {7}, n_calls = {-1};
    std::vector<int32_t> t_len = {100, 100, 100}, q_len = {100, 100, 100}, cigar_len = {4, 4, 4}, status_in = {0, 1, 0}, select = {1, 1, 0},
                         status = std::vector<int32_t>(n);
    std::vector<mgl_sw_chain_alignment> aln = std::vector<mgl_sw_chain_alignment>(n);
    std::vector<char> cigar = std::vector<char>(n * stride, 'M');
    std::vector<uint32_t> counts = std::vector<uint32_t>(8 * region), ins = std::vector<uint32_t>(cap * (6 * 64 + 1));
    std::vector<mgl_sw_site> sites = std::vector<mgl_sw_site>(cap, mgl_sw_site{5, 0, 0, 0, 0, 0, 0, 0});
    std::vector<mgl_sw_call> calls = std::vector<mgl_sw_call>(call_cap);
};

struct InsertionsCall {
    int64_t n = Buffers::n, beg = 0, cap = Buffers::cap;
    int stride = Buffers::stride, flags = 0, max_ins = Buffers::max_ins;
    int null_at = -1; // which of the 12 required pointers is null
    bool status_in = true, select = true, status = true;
};

int insertions(mgl_sw_ctx *ctx, Buffers &b, const InsertionsCall &c)
{
    int k = 0;
    auto p = [&](auto *x) { return k++ == c.null_at ? static_cast<decltype(x)>(nullptr) : x; };
    const uint8_t *targets = p(b.targets.data());
    const int64_t *t_start = p(b.t_start.data());
    const int32_t *t_len = p(b.t_len.data());
    const uint8_t *queries = p(b.queries.data());
    const int64_t *q_start = p(b.q_start.data());
    const int32_t *q_len = p(b.q_len.data());
    const mgl_sw_chain_alignment *aln = p(b.aln.data());
    const char *cigar = p(b.cigar.data());
    const int32_t *cigar_len = p(b.cigar_len.data());
    const mgl_sw_site *sites = p(b.sites.data());
    const int64_t *n_sites = p(b.n_sites.data());
    uint32_t *ins = p(b.ins.data());
    return mgl_sw_pileup_insertions_batch_device(ctx, nullptr, c.n, targets, t_start, t_len, queries, q_start, q_len, aln, cigar, c.stride, cigar_len,
                                                 c.status_in ? b.status_in.data() : nullptr, c.select ? b.select.data() : nullptr, c.beg, sites, n_sites,
                                                 c.cap, c.max_ins, ins, c.status ? b.status.data() : nullptr, c.flags);
}

struct GenotypeCall {
    int64_t len = Buffers::region, beg = 0, cap = Buffers::cap, call_cap = Buffers::call_cap;
    int max_ins = Buffers::max_ins, max_del = 64, cost_match = 11, cost_het = 778, cost_error = 6341;
    int null_at = -1; // which of the 5 required pointers is null
    bool ins = true, calls = true, seq = true;
};

int genotype(mgl_sw_ctx *ctx, Buffers &b, const GenotypeCall &c)
{
    int k = 0;
    auto p = [&](auto *x) { return k++ == c.null_at ? static_cast<decltype(x)>(nullptr) : x; };
    const uint32_t *counts = p(b.counts.data());
    const uint8_t *targets = p(b.targets.data());
    const mgl_sw_site *sites = p(b.sites.data());
    const int64_t *n_sites = p(b.n_sites.data());
    int64_t *n_calls = p(b.n_calls.data());
    return mgl_sw_genotype_sites_device(ctx, nullptr, counts, c.len, targets, c.beg, sites, n_sites, c.cap, c.ins ? b.ins.data() : nullptr, c.max_ins, c.max_del,
                                        c.cost_match, c.cost_het, c.cost_error, c.calls ? b.calls.data() : nullptr, c.call_cap, n_calls,
                                        c.seq ? b.seq.data() : nullptr);
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
    const int64_t kMaxRegion = 0x7fffffff;
    // without a context a well-formed call is refused as such (the fake runtime has devices), with one it is accepted
    for (mgl_sw_ctx *c : {(mgl_sw_ctx *)nullptr, ctx}) {
        const int ok = c ? MGL_SW_OK : MGL_SW_ERR_BAD_ARG;
        auto I = [](auto edit) { InsertionsCall x; edit(x); return x; };
        // (capacities and max_ins that stay inside the buffers: the stand-in adds into the table)
        std::vector<InsertionsCall> good = {InsertionsCall{}, I([](InsertionsCall &x) { x.n = 0; }), I([](InsertionsCall &x) { x.stride = 1; }),
                                            I([](InsertionsCall &x) { x.flags = MGL_SW_FLAG_BINARY_CIGAR; }), I([](InsertionsCall &x) { x.cap = 1; }),
                                            I([](InsertionsCall &x) { x.max_ins = 1; }), I([](InsertionsCall &x) { x.max_ins = 64; }),
                                            I([](InsertionsCall &x) { x.beg = (int64_t)1 << 40; }), I([](InsertionsCall &x) { x.status_in = false; }),
                                            I([](InsertionsCall &x) { x.select = false; }), I([](InsertionsCall &x) { x.status = false; })};
        std::vector<InsertionsCall> bad = {I([](InsertionsCall &x) { x.n = -1; }), I([](InsertionsCall &x) { x.n = ((int64_t)1 << 30) + 1; }),
                                           I([](InsertionsCall &x) { x.stride = 0; }), I([](InsertionsCall &x) { x.stride = 62, x.flags = MGL_SW_FLAG_BINARY_CIGAR; }),
                                           I([](InsertionsCall &x) { x.beg = -1; }), I([](InsertionsCall &x) { x.cap = 0; }),
                                           I([](InsertionsCall &x) { x.cap = ((int64_t)1 << 30) + 1; }), I([](InsertionsCall &x) { x.max_ins = 0; }),
                                           I([](InsertionsCall &x) { x.max_ins = 65; }), I([](InsertionsCall &x) { x.n = 0, x.max_ins = 65; })};
        for (int k = 0; k < 12; ++k) bad.push_back(I([k](InsertionsCall &x) { x.null_at = k; }));
        edges<InsertionsCall>(c, b, insertions, ok, good, bad);

        auto G = [](auto edit) { GenotypeCall x; edit(x); return x; };
        std::vector<GenotypeCall> ggood = {GenotypeCall{}, G([](GenotypeCall &x) { x.len = 1; }), G([](GenotypeCall &x) { x.beg = Buffers::region; }),
                                           G([](GenotypeCall &x) { x.cap = 1; }), G([](GenotypeCall &x) { x.cap = 255; }), G([](GenotypeCall &x) { x.cap = 256; }),
                                           G([](GenotypeCall &x) { x.cap = 257; }), G([](GenotypeCall &x) { x.max_ins = 1; }), G([](GenotypeCall &x) { x.max_ins = 64; }),
                                           G([](GenotypeCall &x) { x.max_del = 1; }), G([](GenotypeCall &x) { x.max_del = 4096; }),
                                           G([](GenotypeCall &x) { x.cost_match = 1, x.cost_het = 2, x.cost_error = 3; }),
                                           G([](GenotypeCall &x) { x.cost_match = (1 << 20) - 2, x.cost_het = (1 << 20) - 1, x.cost_error = 1 << 20; }),
                                           G([](GenotypeCall &x) { x.call_cap = 0; }), G([](GenotypeCall &x) { x.call_cap = 0, x.calls = false, x.seq = false; }),
                                           G([](GenotypeCall &x) { x.ins = false; }), G([](GenotypeCall &x) { x.ins = false, x.seq = false; })};
        std::vector<GenotypeCall> gbad = {G([](GenotypeCall &x) { x.len = 0; }), G([kMaxRegion](GenotypeCall &x) { x.len = kMaxRegion + 1; }),
                                          G([](GenotypeCall &x) { x.beg = -1; }), G([](GenotypeCall &x) { x.cap = 0; }),
                                          G([](GenotypeCall &x) { x.cap = ((int64_t)1 << 30) + 1; }), G([](GenotypeCall &x) { x.max_ins = 0; }),
                                          G([](GenotypeCall &x) { x.max_ins = 65; }), G([](GenotypeCall &x) { x.max_del = 0; }), G([](GenotypeCall &x) { x.max_del = 4097; }),
                                          G([](GenotypeCall &x) { x.cost_match = 0; }), G([](GenotypeCall &x) { x.cost_error = (1 << 20) + 1; }),
                                          G([](GenotypeCall &x) { x.cost_het = x.cost_match; }), G([](GenotypeCall &x) { x.cost_het = x.cost_error; }),
                                          G([](GenotypeCall &x) { x.cost_match = 6341, x.cost_error = 11; }), G([](GenotypeCall &x) { x.call_cap = -1; }),
                                          G([](GenotypeCall &x) { x.call_cap = ((int64_t)1 << 30) + 1; }), G([](GenotypeCall &x) { x.calls = false; }),
                                          G([](GenotypeCall &x) { x.seq = false; })};
        for (int k = 0; k < 5; ++k) gbad.push_back(G([k](GenotypeCall &x) { x.null_at = k; }));
        edges<GenotypeCall>(c, b, genotype, ok, ggood, gbad);
    }
    // what an accepted call leaves: the total, the statuses of the counted alignments
    CHECK(genotype(ctx, b, GenotypeCall{}) == MGL_SW_OK && b.n_calls[0] == 3 && b.calls[2].pos == 512);
    std::fill(b.ins.begin(), b.ins.end(), 0u);
    CHECK(insertions(ctx, b, InsertionsCall{}) == MGL_SW_OK);
    const int W = 6 * Buffers::max_ins + 1;
    CHECK(b.ins[W - 1] == 5 && b.ins[2 * W - 1] == 0 && b.ins[3 * W - 1] == 0); // a status going in, a zero select
    // the active sites are read where the kernel reads them: a count above the capacity, and one below zero
    b.n_sites[0] = Buffers::cap + 9;
    CHECK(insertions(ctx, b, InsertionsCall{}) == MGL_SW_OK);
    b.n_sites[0] = -4;
    CHECK(insertions(ctx, b, InsertionsCall{}) == MGL_SW_OK);
    // a refusal leaves its reason on the context
    InsertionsCall x;
    x.max_ins = 65;
    CHECK(insertions(ctx, b, x) == MGL_SW_ERR_BAD_ARG);
    CHECK(std::string(mgl_sw_last_error(ctx)) == "mgl_sw_pileup_insertions_batch_device: max_ins outside 1 .. 64");
    GenotypeCall y;
    y.cost_het = y.cost_error;
    CHECK(genotype(ctx, b, y) == MGL_SW_ERR_BAD_ARG);
    CHECK(std::string(mgl_sw_last_error(ctx)) == "mgl_sw_genotype_sites_device: the costs are not cost_match < cost_het < cost_error");
    // a workspace limit that does not hold the blocks' counts: refused, nothing launched (nothing is read: the call fails before any launch)
    const int before = mgl_sw_dev::genotype_launches;
    CHECK(mgl_sw_ctx_set_workspace(ctx, 1 << 20) == 0);
    GenotypeCall big;
    big.cap = (int64_t)1 << 30;
    big.call_cap = 0;
    CHECK(genotype(ctx, b, big) == MGL_SW_ERR_NOMEM && mgl_sw_dev::genotype_launches == before);
    CHECK(mgl_sw_dev::insertions_launches >= 10 && mgl_sw_dev::genotype_launches >= 3 * 17);
    mgl_sw_ctx_destroy(ctx);
    std::printf("calls-san ok: %d insertions launches, %d genotype launches\n", mgl_sw_dev::insertions_launches, mgl_sw_dev::genotype_launches);
    return 0;
}
