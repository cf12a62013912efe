// pileup_san_driver.cpp -- the host side of mgl_sw_pileup_alignments_batch_device and mgl_sw_pileup_sites_device
// (mgl_amd/csrc/sw_pileup.cpp) under -fsanitize=address,undefined against the fake HIP runtime (fake_hip/): every call-level refusal on
// both sides of its edge, with and without a context, and accepted calls of each entry, whose "launches" are the stand-ins below --
// they check the arguments the host side hands to the kernels (the grid, the region, the workspace's parts inside the borrowed region
// and apart from one another) and touch every byte of the workspace.  TEST-ONLY; make -C tests/cpp -f pileup_san.mk pileup-san.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mgl_sw.h"
#include "../../mgl_amd/csrc/sw_pileup.h"

#define CHECK(x)                                                                        \
    do {                                                                                \
        if (!(x)) {                                                                     \
            std::fprintf(stderr, "pileup_san_driver.cpp:%d: CHECK failed: %s\n", __LINE__, #x); \
            std::exit(1);                                                               \
        }                                                                               \
    } while (0)

namespace mgl_sw_dev {

static int pileup_launches = 0, sites_launches = 0;
static const size_t kScanBytes = 1000; // (no multiple of 256: the host side rounds)

hipError_t launch_pileup(const PileupArgs &a, hipStream_t)
{
    CHECK(a.n >= 1 && a.groups >= 1 && a.groups <= (a.n + 3) / 4);
    CHECK(a.queries && a.t_start && a.q_start && a.t_len && a.q_len && a.aln && a.cigar && a.cigar_len && a.counts);
    CHECK(a.region_beg >= 0 && a.region_len >= 1 && a.cigar_stride >= 1 && (a.binary == 0 || a.cigar_stride % 4 == 0));
    for (int64_t p = 0; p < a.n; ++p) {
        if (a.status_in && a.status_in[p]) continue;
        if (a.select && !a.select[p]) continue;
        a.counts[p % (8 * a.region_len)] += 1; // (ASan: inside the caller's table)
        if (a.status) a.status[p] = 0;
    }
    ++pileup_launches;
    return hipSuccess;
}

hipError_t pileup_scan_bytes(const int64_t entries, size_t *bytes)
{
    CHECK(entries >= 2 && bytes);
    *bytes = kScanBytes;
    return hipSuccess;
}

hipError_t launch_pileup_flag(const PileupSitesArgs &a, hipStream_t)
{
    CHECK(a.counts && a.ref && a.n_sites && a.block_count && a.block_start && a.scan_tmp);
    CHECK(a.blocks == (a.region_len + PILEUP_SITE_BLOCK - 1) / PILEUP_SITE_BLOCK && a.scan_bytes >= kScanBytes);
    // the workspace: three parts, ascending, each holding its entries, each on a 256-byte border
    const unsigned char *c = reinterpret_cast<unsigned char *>(a.block_count), *s = reinterpret_cast<unsigned char *>(a.block_start),
                        *t = static_cast<unsigned char *>(a.scan_tmp);
    CHECK(s >= c + (a.blocks + 1) * 8 && t >= s + (a.blocks + 1) * 8 && (s - c) % 256 == 0 && (t - c) % 256 == 0);
    for (int64_t b = 0; b <= a.blocks; ++b) a.block_count[b] = b < a.blocks ? 1 : 0; // (ASan: inside the borrowed region)
    for (int64_t i = 0; i < a.region_len; ++i) {
        CHECK(a.ref[i] == 'A');
        if (a.call) a.call[i] = 'N';
        if (a.flags) a.flags[i] = 0;
    }
    ++sites_launches;
    return hipSuccess;
}

hipError_t launch_pileup_scan(const PileupSitesArgs &a, hipStream_t)
{
    std::memset(a.scan_tmp, 0x5a, a.scan_bytes);
    int64_t sum = 0;
    for (int64_t b = 0; b <= a.blocks; ++b) a.block_start[b] = sum, sum += a.block_count[b];
    ++sites_launches;
    return hipSuccess;
}

hipError_t launch_pileup_write(const PileupSitesArgs &a, hipStream_t)
{
    CHECK(a.site_capacity == 0 || a.sites);
    a.n_sites[0] = a.block_start[a.blocks];
    for (int64_t k = 0; k < a.site_capacity && k < a.blocks; ++k) a.sites[k] = mgl_sw_site{(int32_t)(k * PILEUP_SITE_BLOCK), 2, 0, 0, 0, 0, 0, 0};
    ++sites_launches;
    return hipSuccess;
}

} // namespace mgl_sw_dev

namespace {

struct Buffers {
    static constexpr int64_t n = 3, region = 1000, stride = 64, cap = 10;
    std::vector<uint8_t> targets = std::vector<uint8_t>(2 * region, 'A'), queries = std::vector<uint8_t>(300, 'C'), call = std::vector<uint8_t>(region),
                         flags = std::vector<uint8_t>(region);
    std::vector<int64_t> t_start = {0, 100, 200}, q_start = {0, 100, 200}, n_sites = {-1};
    std::vector<int32_t> t_len = {100, 100, 100}, q_len = {100, 100, 100}, cigar_len = {4, 4, 4}, status_in = {0, 1, 0}, select = {1, 1, 0},
                         status = std::vector<int32_t>(n);
    std::vector<mgl_sw_chain_alignment> aln = std::vector<mgl_sw_chain_alignment>(n);
    std::vector<char> cigar = std::vector<char>(n * stride, 'M');
    std::vector<uint32_t> counts = std::vector<uint32_t>(8 * region);
    std::vector<mgl_sw_site> sites = std::vector<mgl_sw_site>(cap);
};

struct PileupCall {
    int64_t n = Buffers::n, beg = 0, len = Buffers::region;
    int stride = Buffers::stride, flags = 0;
    int null_at = -1; // which of the 10 required pointers is null
    bool status_in = true, select = true, status = true;
};

int pileup(mgl_sw_ctx *ctx, Buffers &b, const PileupCall &c)
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
    uint32_t *counts = p(b.counts.data());
    return mgl_sw_pileup_alignments_batch_device(ctx, nullptr, c.n, targets, t_start, t_len, queries, q_start, q_len, aln, cigar, c.stride, cigar_len,
                                                 c.status_in ? b.status_in.data() : nullptr, c.select ? b.select.data() : nullptr, c.beg, c.len, counts,
                                                 c.status ? b.status.data() : nullptr, c.flags);
}

struct SitesCall {
    int64_t len = Buffers::region, beg = 0, cap = Buffers::cap;
    int min_depth = 4, min_alt = 2, min_frac = 64;
    int null_at = -1; // which of the 3 required pointers is null
    bool call = true, flags = true, sites = true;
};

int sites(mgl_sw_ctx *ctx, Buffers &b, const SitesCall &c)
{
    int k = 0;
    auto p = [&](auto *x) { return k++ == c.null_at ? static_cast<decltype(x)>(nullptr) : x; };
    const uint32_t *counts = p(b.counts.data());
    const uint8_t *targets = p(b.targets.data());
    int64_t *n_sites = p(b.n_sites.data());
    return mgl_sw_pileup_sites_device(ctx, nullptr, counts, c.len, targets, c.beg, c.min_depth, c.min_alt, c.min_frac, c.call ? b.call.data() : nullptr,
                                      c.flags ? b.flags.data() : nullptr, c.sites ? b.sites.data() : nullptr, c.cap, n_sites);
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
        auto P = [](auto edit) { PileupCall x; edit(x); return x; };
        // (regions that end inside the table: the stand-in adds into it)
        std::vector<PileupCall> good = {PileupCall{}, P([](PileupCall &x) { x.n = 0; }), P([](PileupCall &x) { x.stride = 1; }),
                                        P([](PileupCall &x) { x.flags = MGL_SW_FLAG_BINARY_CIGAR; }), P([](PileupCall &x) { x.len = 1; }),
                                        P([](PileupCall &x) { x.beg = (int64_t)1 << 40; }), P([](PileupCall &x) { x.status_in = false; }),
                                        P([](PileupCall &x) { x.select = false; }), P([](PileupCall &x) { x.status = false; })};
        std::vector<PileupCall> bad = {P([](PileupCall &x) { x.n = -1; }), P([](PileupCall &x) { x.n = ((int64_t)1 << 30) + 1; }), P([](PileupCall &x) { x.stride = 0; }),
                                       P([](PileupCall &x) { x.stride = 62, x.flags = MGL_SW_FLAG_BINARY_CIGAR; }), P([](PileupCall &x) { x.beg = -1; }),
                                       P([](PileupCall &x) { x.len = 0; }), P([kMaxRegion](PileupCall &x) { x.len = kMaxRegion + 1; })};
        for (int k = 0; k < 10; ++k) bad.push_back(P([k](PileupCall &x) { x.null_at = k; }));
        edges<PileupCall>(c, b, pileup, ok, good, bad);

        auto S = [](auto edit) { SitesCall x; edit(x); return x; };
        std::vector<SitesCall> sgood = {SitesCall{}, S([](SitesCall &x) { x.len = 1; }), S([](SitesCall &x) { x.len = 255; }), S([](SitesCall &x) { x.len = 256; }),
                                        S([](SitesCall &x) { x.len = 257; }), S([](SitesCall &x) { x.beg = Buffers::region; }), S([](SitesCall &x) { x.min_depth = 1; }),
                                        S([](SitesCall &x) { x.min_alt = 1; }), S([](SitesCall &x) { x.min_frac = 1; }), S([](SitesCall &x) { x.min_frac = 256; }),
                                        S([](SitesCall &x) { x.cap = 0; }), S([](SitesCall &x) { x.cap = 0, x.sites = false; }), S([](SitesCall &x) { x.call = false; }),
                                        S([](SitesCall &x) { x.flags = false; })};
        std::vector<SitesCall> sbad = {S([](SitesCall &x) { x.len = 0; }), S([kMaxRegion](SitesCall &x) { x.len = kMaxRegion + 1; }), S([](SitesCall &x) { x.beg = -1; }),
                                       S([](SitesCall &x) { x.min_depth = 0; }), S([](SitesCall &x) { x.min_alt = 0; }), S([](SitesCall &x) { x.min_frac = 0; }),
                                       S([](SitesCall &x) { x.min_frac = 257; }), S([](SitesCall &x) { x.cap = -1; }), S([](SitesCall &x) { x.cap = ((int64_t)1 << 30) + 1; }),
                                       S([](SitesCall &x) { x.sites = false; })};
        for (int k = 0; k < 3; ++k) sbad.push_back(S([k](SitesCall &x) { x.null_at = k; }));
        edges<SitesCall>(c, b, sites, ok, sgood, sbad);
    }
    // what an accepted call leaves: the total, the statuses of the counted alignments
    CHECK(sites(ctx, b, SitesCall{}) == MGL_SW_OK && b.n_sites[0] == 4 && b.sites[3].pos == 768);
    std::fill(b.counts.begin(), b.counts.end(), 0u);
    CHECK(pileup(ctx, b, PileupCall{}) == MGL_SW_OK);
    CHECK(b.counts[0] == 1 && b.counts[1] == 0 && b.counts[2] == 0); // a status going in, a zero select
    // a refusal leaves its reason on the context
    PileupCall x;
    x.len = 0;
    CHECK(pileup(ctx, b, x) == MGL_SW_ERR_BAD_ARG);
    CHECK(std::string(mgl_sw_last_error(ctx)) == "mgl_sw_pileup_alignments_batch_device: region_len outside 1 .. 2^31 - 1");
    SitesCall y;
    y.min_frac = 257;
    CHECK(sites(ctx, b, y) == MGL_SW_ERR_BAD_ARG);
    CHECK(std::string(mgl_sw_last_error(ctx)) == "mgl_sw_pileup_sites_device: min_frac outside 1 .. 256");
    // a workspace limit that does not hold the blocks' counts: refused, nothing launched (nothing is read: the call fails before any launch)
    const int before = mgl_sw_dev::sites_launches;
    CHECK(mgl_sw_ctx_set_workspace(ctx, 1 << 20) == 0);
    SitesCall big;
    big.len = kMaxRegion;
    big.cap = 0;
    CHECK(sites(ctx, b, big) == MGL_SW_ERR_NOMEM && mgl_sw_dev::sites_launches == before);
    CHECK(mgl_sw_dev::pileup_launches >= 8 && mgl_sw_dev::sites_launches >= 3 * 14);
    mgl_sw_ctx_destroy(ctx);
    std::printf("pileup-san ok: %d pileup launches, %d sites launches\n", mgl_sw_dev::pileup_launches, mgl_sw_dev::sites_launches);
    return 0;
}
