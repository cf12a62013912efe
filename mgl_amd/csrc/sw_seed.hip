// sw_seed.hip -- the three kernels of mgl_sw_seed_batch_device (the function is tests/seed_textbook.py's).
// sw_seed.h describes the workspace they share with the host side.
//
// sw_seed_kernel, the hot path: one workgroup of 256 threads per pair, persistent over the pairs.  A sequence is sketched SEED_BLOCK
// k-mer positions at a time: the bytes of the block and of the w - 1 positions to either side go to LDS as 2-bit codes, a thread forms key
// and hash of a position from its k codes, a thread per window takes the window's minimum from LDS (strict `<` while the position
// ascends: ties to the smallest position) and flags it, and the flagged positions of the block are compacted in order by a prefix count
// (a thread owns four neighbouring positions).
//   (a) the query's sketch, as (key << 32 | position), bitonic-sorted;
//   (b) the window's sketch, never stored: a selected position looks its key up in the table (binary search, then the run of equal keys,
//       dropped above max_occ) and a prefix sum over the run lengths says where its hits go -- ascending by (t, q) without a sort;
//   (c) the merge: the hits re-keyed (diagonal << 32 | t) and sorted; a hit is a run's head iff it is the first of its diagonal or
//       starts beyond the end of the one before it, which says the same as "beyond the end of the run so far" because all hits are k
//       long; the r-th head and the r-th tail are one run's, so heads and tails are compacted by one prefix count; the runs are sorted
//       back by (t, q) with their lengths;
//   (d) N_p and the candidates go to the pair's staging.
// The table and the hits live in LDS while they fit (SEED_LDS_TAB, SEED_LDS_HITS) and move to the workgroup's workspace slot when a pair
// outgrows that; the code reads either through one pointer.
//
// sw_seed_scan_kernel: one block, the exclusive prefix sum of the counts into d_cand_start_out with a running carry, 1024 pairs a step,
// cut at the capacity.  sw_seed_pack_kernel: one wave per pair, the staging into the pair's CSR place.
#include "sw_seed_dev.h"

namespace mgl_sw_dev {

namespace {

constexpr int SEED_ST_BAD_ARG = 1, SEED_ST_NOMEM = 3, SEED_ST_UNSUPPORTED = 5; // mgl_sw_status
constexpr int SEED_SPAN = SEED_BLOCK + 2 * SEED_MAX_W;                        // positions staged for one block (B + 2 w - 2 at most)

struct SeedLds {
    uint64_t tab[SEED_LDS_TAB];
    uint64_t hits[SEED_LDS_HITS];
    uint32_t key[SEED_SPAN];
    uint32_t hash[SEED_SPAN];
    uint32_t flag[SEED_BLOCK / 4]; // a byte per position of the block
    uint8_t code[SEED_SPAN + SEED_MAX_K];
    uint8_t valid[SEED_SPAN];
    int wave_sum[SEED_THREADS / 64];
};
static_assert(sizeof(SeedLds) <= 64 * 1024, "a workgroup's LDS");
__shared__ SeedLds s; // sw_seed_kernel's alone: the other two kernels reach nothing that names it

// the exclusive prefix sum of v over the workgroup, and the sum
__device__ inline int seed_block_scan(const int v, int &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    if (lane == 63) s.wave_sum[wave] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int x = 0; x < SEED_THREADS / 64; ++x) {
        const int ws = s.wave_sum[x];
        before += x < wave ? ws : 0;
        all += ws;
    }
    __syncthreads();
    total = all;
    return before + incl - v;
}

// Positions [p0, p0 + SEED_BLOCK) of a sequence of nk k-mer positions: key, hash and validity of every position a window over them can
// see, from `lo` on (returned), and flag[] set for the selected ones among them.  Not inlined, nor is the sort: the kernel with all of its
// phases inlined keeps more wave-uniform values alive than there are scalar registers.
__device__ __noinline__ int64_t seed_sketch_block(const uint8_t *seq, const int64_t nk, const int k, const int w, const int64_t p0)
{
    const int tid = threadIdx.x;
    const int64_t lo = p0 - w + 1 > 0 ? p0 - w + 1 : 0;
    const int64_t hi = p0 + SEED_BLOCK + w - 2 < nk - 1 ? p0 + SEED_BLOCK + w - 2 : nk - 1; // the last position a window sees
    const int npos = (int)(hi - lo + 1), nbytes = npos + k - 1;
    for (int i = tid; i < nbytes; i += SEED_THREADS) s.code[i] = seed_code(seq[lo + i]);
    s.flag[tid] = 0;
    __syncthreads();
    for (int i = tid; i < npos; i += SEED_THREADS) {
        uint32_t key = 0, bad = 0;
        for (int j = 0; j < k; ++j) {
            const uint32_t c = s.code[i + j];
            bad |= c >> 2;
            key = key << 2 | (c & 3);
        }
        s.key[i] = key;
        s.hash[i] = seed_hash(key);
        s.valid[i] = !bad;
    }
    __syncthreads();
    const int64_t last_win = nk - w > 0 ? nk - w : 0;
    const int64_t a_hi = p0 + SEED_BLOCK - 1 < last_win ? p0 + SEED_BLOCK - 1 : last_win;
    uint8_t *const flag = reinterpret_cast<uint8_t *>(s.flag);
    for (int64_t a = lo + tid; a <= a_hi; a += SEED_THREADS) {
        const int from = (int)(a - lo), to = (int)((a + w < nk ? a + w : nk) - lo);
        int best = -1;
        uint32_t best_h = 0;
        for (int i = from; i < to; ++i) {
            const uint32_t h = s.hash[i];
            const bool take = s.valid[i] && (best < 0 || h < best_h);
            best = take ? i : best;
            best_h = take ? h : best_h;
        }
        const int64_t at = best + lo - p0;
        if (best >= 0 && at >= 0 && at < SEED_BLOCK) flag[at] = 1;
    }
    __syncthreads();
    return lo;
}

__global__ __launch_bounds__(SEED_THREADS) void sw_seed_kernel(const SeedStageArgs a)
{
    const int tid = threadIdx.x;
    const int k = a.k, w = a.w;
    const SeedWorkspace sg = seed_workspace(a.n, a.max_cand);
    int32_t *const count = reinterpret_cast<int32_t *>(a.ws + sg.count), *const stage = reinterpret_cast<int32_t *>(a.ws + sg.stage);
    unsigned char *const slot = a.ws + sg.bytes + (int64_t)blockIdx.x * sg.slot_bytes;
    uint64_t *const slot_tab = reinterpret_cast<uint64_t *>(slot);
    uint64_t *const slot_hits = reinterpret_cast<uint64_t *>(slot + SEED_SLOT_TAB); // (both only where max_cand is above SEED_LDS_HITS)
    uint32_t *const slot_len = reinterpret_cast<uint32_t *>(slot + SEED_SLOT_LEN);
    const uint8_t *const flag = reinterpret_cast<const uint8_t *>(s.flag);

    for (int p = blockIdx.x; p < (int)a.n; p += a.groups) { // (n <= 2^30)
        __syncthreads(); // (the pair before this one is done with LDS)
        const int tl = a.t_len[p], ql = a.q_len[p];
        auto finish = [&](const int n_cand, const int status) {
            if (tid != 0) return;
            count[p] = n_cand;
            if (a.status) a.status[p] = status;
        };
        if (tl < 1 || ql < 1) {
            finish(0, SEED_ST_BAD_ARG);
            continue;
        }
        const uint8_t *const T = a.targets + a.t_start[p], *const Q = a.queries + a.q_start[p];
        const int nkq = ql - k + 1, nkt = tl - k + 1;

        // ---- (a) the query's sketch, sorted by (key, position)
        uint64_t *tab = s.tab;
        int nq = 0;
        bool refused = false;
        for (uint32_t p0 = 0; (int64_t)p0 < nkq; p0 += SEED_BLOCK) { // (unsigned: the step past a sequence of nearly 2^31 bytes)
            const int64_t lo = seed_sketch_block(Q, nkq, k, w, p0);
            const uint32_t f = s.flag[tid];
            int total;
            int at = nq + seed_block_scan(__popc(f), total);
            if (nq + total > SEED_MAX_QUERY_SEEDS) {
                refused = true;
                break;
            }
            if (tab == s.tab && nq + total > SEED_LDS_TAB) { // the table leaves LDS
                for (int i = tid; i < nq; i += SEED_THREADS) slot_tab[i] = s.tab[i];
                tab = slot_tab;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (flag[tid * 4 + j]) {
                    const int64_t pos = p0 + tid * 4 + j;
                    tab[at++] = (uint64_t)s.key[pos - lo] << 32 | (uint64_t)pos;
                }
            nq += total;
            __syncthreads();
        }
        if (refused) {
            finish(0, SEED_ST_UNSUPPORTED);
            continue;
        }
        if (nq == 0) { // (no key to meet: no hit)
            finish(0, 0);
            continue;
        }
        {
            const int n2 = seed_pow2(nq);
            for (int i = nq + tid; i < n2; i += SEED_THREADS) tab[i] = ~0ull;
            __syncthreads();
            seed_bitonic(tab, nullptr, n2);
        }

        // ---- (b) the window's sketch against the table: the raw hits (t << 32 | q), ascending
        uint64_t *hits = s.hits;
        int R = 0;
        for (uint32_t p0 = 0; (int64_t)p0 < nkt; p0 += SEED_BLOCK) {
            const int64_t lo = seed_sketch_block(T, nkt, k, w, p0);
            int first[4], cnt[4], sum = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                first[j] = cnt[j] = 0;
                if (flag[tid * 4 + j]) {
                    const uint32_t key = s.key[p0 + tid * 4 + j - lo];
                    const uint64_t want = (uint64_t)key << 32;
                    int b = 0, e = nq; // the first entry not below `want`
                    while (b < e) {
                        const int m = (b + e) >> 1;
                        if (tab[m] < want) b = m + 1;
                        else e = m;
                    }
                    int c = 0;
                    while (b + c < nq && c <= a.max_occ && (uint32_t)(tab[b + c] >> 32) == key) ++c;
                    first[j] = b;
                    cnt[j] = c <= a.max_occ ? c : 0;
                    sum += cnt[j];
                }
            }
            int total;
            int at = R + seed_block_scan(sum, total);
            if (R + total > a.max_cand) {
                refused = true;
                break;
            }
            if (hits == s.hits && R + total > SEED_LDS_HITS) { // the hits leave LDS (max_cand is above SEED_LDS_HITS: the slot has the room)
                for (int i = tid; i < R; i += SEED_THREADS) slot_hits[i] = s.hits[i];
                hits = slot_hits;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint64_t t = (uint64_t)(p0 + tid * 4 + j) << 32;
                for (int c = 0; c < cnt[j]; ++c) hits[at++] = t | (uint32_t)tab[first[j] + c];
            }
            R += total;
            __syncthreads();
        }
        if (refused) {
            finish(0, SEED_ST_UNSUPPORTED);
            continue;
        }

        int32_t *const st = stage + (int64_t)p * 3 * a.max_cand, *const sq = st + a.max_cand, *const sl = sq + a.max_cand;
        if (!a.merge || R == 0) {
            for (int i = tid; i < R; i += SEED_THREADS) {
                const uint64_t h = hits[i];
                st[i] = (int32_t)(h >> 32);
                sq[i] = (int32_t)(uint32_t)h;
                sl[i] = k;
            }
            finish(R, 0);
            continue;
        }

        // ---- (c) the merge: by (diagonal, t); heads and tails of the runs; back by (t, q)
        const int n2 = seed_pow2(R);
        for (int i = tid; i < n2; i += SEED_THREADS) {
            const uint64_t h = hits[i];
            const uint32_t t = (uint32_t)(h >> 32), q = (uint32_t)h;
            hits[i] = i < R ? (uint64_t)(t - q + 0x80000000u) << 32 | t : ~0ull;
        }
        __syncthreads();
        seed_bitonic(hits, nullptr, n2);
        // the runs go where the table was: it is not read again
        const bool in_lds = hits == s.hits;
        uint64_t *const run = in_lds ? s.tab : slot_tab;
        uint32_t *const len = in_lds ? reinterpret_cast<uint32_t *>(s.tab + SEED_LDS_HITS) : slot_len;
        int N = 0;
        for (int base = 0; base < R; base += SEED_THREADS) {
            const int i = base + tid;
            bool head = false, tail = false;
            uint64_t me = 0;
            if (i < R) {
                me = hits[i];
                const uint64_t prev = i > 0 ? hits[i - 1] : 0, next = i + 1 < R ? hits[i + 1] : 0;
                head = i == 0 || (prev >> 32) != (me >> 32) || me > prev + (uint64_t)k;          // (the same diagonal: the difference is t's)
                tail = i + 1 == R || (next >> 32) != (me >> 32) || next > me + (uint64_t)k;
            }
            int total;
            const int r = N + seed_block_scan(head ? 1 : 0, total) + (head ? 1 : 0) - 1; // the run this hit belongs to
            const uint32_t t = (uint32_t)me, d = (uint32_t)(me >> 32);
            if (head) run[r] = (uint64_t)t << 32 | (uint32_t)(t - d + 0x80000000u);
            if (tail) len[r] = t + (uint32_t)k; // the run's end; its length once the head is known to all
            N += total;
        }
        __syncthreads();
        const int m2 = seed_pow2(N);
        for (int i = tid; i < m2; i += SEED_THREADS) {
            if (i < N) len[i] -= (uint32_t)(run[i] >> 32);
            else run[i] = ~0ull, len[i] = 0;
        }
        __syncthreads();
        seed_bitonic(run, len, m2);

        // ---- (d) the pair's staging
        for (int i = tid; i < N; i += SEED_THREADS) {
            const uint64_t h = run[i];
            st[i] = (int32_t)(h >> 32);
            sq[i] = (int32_t)(uint32_t)h;
            sl[i] = (int32_t)len[i];
        }
        finish(N, 0);
    }
}

__global__ __launch_bounds__(1024) void sw_seed_scan_kernel(const SeedStageArgs a)
{
    __shared__ int64_t wave_sum[16];
    __shared__ int64_t cut_at; // S_(P*), or -1 while every pair fits
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int32_t *const count = reinterpret_cast<int32_t *>(a.ws + seed_workspace(a.n, a.max_cand).count);
    if (tid == 0) cut_at = -1;
    __syncthreads();
    int64_t carry = 0;
    for (int64_t base = 0; base < a.n; base += 1024) {
        const int64_t p = base + tid;
        const int64_t own = p < a.n ? count[p] : 0;
        int64_t incl = own;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        int64_t before = carry, all = 0;
        for (int x = 0; x < 16; ++x) {
            const int64_t sum = wave_sum[x];
            before += x < wave ? sum : 0;
            all += sum;
        }
        const int64_t excl = before + incl - own, end = excl + own;
        // the sums ascend: P* is the one pair that begins inside the capacity and ends beyond it
        if (p < a.n && end > a.cand_capacity && excl <= a.cand_capacity) cut_at = excl;
        __syncthreads();
        if (p < a.n) {
            if (end <= a.cand_capacity) a.cand_start[p] = excl;
            else {
                a.cand_start[p] = cut_at;
                count[p] = 0;
                if (a.status && a.status[p] == 0) a.status[p] = SEED_ST_NOMEM;
            }
        }
        carry += all;
    }
    if (tid == 0) a.cand_start[a.n] = carry <= a.cand_capacity ? carry : cut_at;
}

__global__ __launch_bounds__(64) void sw_seed_pack_kernel(const SeedStageArgs a)
{
    const int lane = threadIdx.x;
    const SeedWorkspace sg = seed_workspace(a.n, a.max_cand);
    const int32_t *const count = reinterpret_cast<const int32_t *>(a.ws + sg.count), *const stage = reinterpret_cast<const int32_t *>(a.ws + sg.stage);
    for (int64_t p = blockIdx.x; p < a.n; p += gridDim.x) {
        const int cnt = count[p];
        if (cnt == 0) continue;
        const int64_t at = a.cand_start[p];
        const int32_t *const st = stage + p * 3 * a.max_cand, *const sq = st + a.max_cand, *const sl = sq + a.max_cand;
        if (at < 0 || at + cnt > a.cand_capacity) continue; // (the scan kept the pair: this holds)
        for (int m = lane; m < cnt; m += 64) {
            a.cand_t[at + m] = st[m];
            a.cand_q[at + m] = sq[m];
            a.cand_len[at + m] = sl[m];
        }
    }
}

} // namespace

hipError_t launch_seed(const SeedStageArgs &a, hipStream_t stream)
{
    if (a.n < 1) return hipSuccess;
    if (a.n > SEED_MAX_PAIRS || a.groups < 1 || a.k < SEED_MIN_K || a.k > SEED_MAX_K || a.w < 1 || a.w > SEED_MAX_W) return hipErrorInvalidValue;
    if (a.max_occ < 1 || a.max_occ > SEED_MAX_OCC || a.max_cand < 1 || a.max_cand > SEED_MAX_CAND) return hipErrorInvalidValue;
    if (!a.ws) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_seed_kernel, dim3((unsigned)a.groups), dim3(SEED_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_seed_scan(const SeedStageArgs &a, hipStream_t stream)
{
    if (a.n < 0 || a.n > SEED_MAX_PAIRS || !a.cand_start || (a.n > 0 && !a.ws)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_seed_scan_kernel, dim3(1), dim3(1024), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_seed_pack(const SeedStageArgs &a, hipStream_t stream)
{
    if (a.n < 1 || a.cand_capacity < 1) return hipSuccess;
    if (!a.ws || !a.cand_start || !a.cand_t || !a.cand_q || !a.cand_len) return hipErrorInvalidValue;
    const int64_t grid = a.n < 65536 ? a.n : 65536;
    hipLaunchKernelGGL(sw_seed_pack_kernel, dim3((unsigned)grid), dim3(64), 0, stream, a);
    return hipGetLastError();
}

} // namespace mgl_sw_dev
