// sw_seed.h -- mgl_sw_seed_batch_device: the seed stage of seed - chain - extend.  The minimizer sketches of a read and of its own
// window, their common keys as raw hits, the hits on one diagonal merged into maximal exact runs, and the candidates of the batch written
// as the CSR arrays that mgl_sw_chain_anchors_batch_device reads (the definition is tests/seed_textbook.py's).  The
// arguments of the three kernels and the layout of the workspace, shared by sw_seed.hip and the host side (sw_seed.cpp).
//
// The workspace, every part on a multiple of 256:
//   per pair         `count`, N_p: the pair's candidates (0 for a refused pair; the scan zeroes it behind the capacity cut)
//   per pair         `stage`: 3 max_cand int32, the pair's candidates ascending by (t, q): their t, then their q, then their l
//   per workgroup    a slot of `slot_bytes` for what a pair needs beyond the workgroup's LDS: the query's sorted sketch above
//                    SEED_LDS_TAB entries (SEED_SLOT_TAB bytes), and -- only where max_cand is above SEED_LDS_HITS -- the raw hits (at
//                    SEED_SLOT_TAB) and the merged runs' lengths (at SEED_SLOT_LEN): SEED_SLOT_BIG bytes in all
#ifndef MGL_SW_SEED_H
#define MGL_SW_SEED_H

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mgl_sw_dev {

constexpr int64_t SEED_MAX_PAIRS = (int64_t)1 << 30; // pairs of one call, and the candidates' capacity
constexpr int SEED_MIN_K = 4, SEED_MAX_K = 16;
constexpr int SEED_MAX_W = 32;
constexpr int SEED_MAX_OCC = 64;
constexpr int SEED_MAX_QUERY_SEEDS = 8192; // a query's sketch: what the sorted table holds
constexpr int SEED_MAX_CAND = 8192;        // a pair's raw hits: what is held and sorted
constexpr int SEED_THREADS = 256;          // a workgroup: one pair at a time
constexpr int SEED_BLOCK = 1024;           // k-mer positions a workgroup sketches at once: 4 per thread
constexpr int SEED_LDS_TAB = 4096;         // entries of the query's table kept in LDS
constexpr int SEED_LDS_HITS = 2048;        // raw hits kept in LDS
constexpr int SEED_GROUPS_PER_CU = 2;      // the grid: at most this many workgroups per CU (60 KiB of LDS each)
constexpr int SEED_SLOT_TAB = SEED_MAX_QUERY_SEEDS * 8;         // a slot: the table ...
constexpr int SEED_SLOT_LEN = SEED_SLOT_TAB + SEED_MAX_CAND * 8; // ... the raw hits behind it ...
constexpr int SEED_SLOT_BIG = SEED_SLOT_LEN + SEED_MAX_CAND * 4; // ... and the runs' lengths

__host__ __device__ inline int64_t seed_ws_round(int64_t bytes, int64_t to) { return (bytes + to - 1) / to * to; }

struct SeedWorkspace {
    int64_t count, stage; // int32 per pair; 3 max_cand int32 per pair
    int64_t bytes;        // the slots begin here
    int slot_bytes;
};
__host__ __device__ inline SeedWorkspace seed_workspace(int64_t n, int max_cand)
{
    SeedWorkspace s{};
    s.count = 0;
    s.stage = seed_ws_round(n * 4, 256);
    s.bytes = s.stage + seed_ws_round(n * max_cand * 12, 256);
    s.slot_bytes = max_cand > SEED_LDS_HITS ? SEED_SLOT_BIG : SEED_SLOT_TAB;
    return s;
}

struct SeedStageArgs {
    const uint8_t *targets, *queries;          // the caller's
    const int64_t *t_start, *q_start;
    const int32_t *t_len, *q_len;
    int64_t n, cand_capacity;
    int k, w, max_occ, merge, max_cand;
    // ---- workspace
    unsigned char *ws;                         // laid out by seed_workspace(n, max_cand), `groups` slots at its end
    int groups;
    // ---- the caller's outputs
    int64_t *cand_start;                       // n + 1
    int32_t *cand_t, *cand_q, *cand_len;       // cand_capacity each
    int32_t *status;                           // optional, per pair
};

hipError_t launch_seed(const SeedStageArgs &a, hipStream_t stream);      // sw_seed_kernel: count, the staging, status
hipError_t launch_seed_scan(const SeedStageArgs &a, hipStream_t stream); // cand_start = the prefix sum of count, cut at the capacity
hipError_t launch_seed_pack(const SeedStageArgs &a, hipStream_t stream); // the candidates into their CSR place

} // namespace mgl_sw_dev

#endif
