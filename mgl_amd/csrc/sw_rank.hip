// sw_rank.hip -- the two kernels of mgl_sw_rank_chains_batch_device (the function is tests/rank_textbook.py's).
// sw_rank.h describes the workspace they share with the host side.
//
// sw_rank_chains_kernel, the hot path: one workgroup of 256 threads per READ, persistent over the reads.  A read is checked first --
// its rows' lengths and ranges, then every pred of every row that is read, straight from the caller's array -- so a refused read writes
// nothing but its count and status and no walk starts over a pred that was not checked.  Then the rows one after the other:
//   (a) f (4 bytes), i - pred(i) (a byte, 0 for -1) and the key (~f's order << 32 | index) of every candidate go to LDS, coalesced;
//       the used bitmap is cleared;
//   (b) the keys are bitonic-sorted, as sw_seed_index_kernel sorts its table: ascending keys are (f descending, index ascending);
//   (c) wave 0 visits the sorted keys 64 at a time: a ballot of the lanes whose candidate is unused, the first set bit, and the walk
//       along pred out of LDS, the same in every lane.  Every step of a walk marks a candidate used, and every turn of the visit either
//       starts a walk or leaves the block of 64: N marks and N + N / 64 ballots bound the serial part, whatever f and pred hold;
//   (d) a kept chain goes into the read's list, entry j in lane j, by insertion on (score descending, strand ascending, end_index
//       ascending): the entries ahead of it are counted with a ballot, the others move up a lane and the last falls off.  That is
//       sort-then-cut.
// The pred bytes of BOTH rows stay in LDS, so that the chains can be walked once more at the end.  After the last row thread 0 finds
// the parents over the at most 16 chains, and thread c writes the record of chain c -- its spans from the candidates of its two ends,
// its mapping quality in 64-bit integers -- and, where anchors are wanted, walks chain c again and writes its K candidate indices
// ascending into the read's staging.
// The LDS is static and sized by the template argument: rows up to RANK_CAP_SMALL candidates run the small form, two workgroups to a
// CU; above it (to RANK_MAX_CAND) the large form, one workgroup to a CU.
//
// sw_rank_pack_kernel: one wave per read, 64 staged indices a step, their candidates into the read's CSR place.
#include "sw_band_wave.h"
#include "sw_rank.h"
#include "sw_seed_dev.h"

namespace mgl_sw_dev {

namespace {

static_assert(SEED_THREADS == RANK_THREADS, "seed_bitonic sorts with the workgroup sw_rank_chains_kernel runs");
static_assert(RANK_MAX_CAND == SEED_MAX_CAND, "the seed stages' ceiling");

template <int CAP> struct RankLds {
    uint64_t key[CAP];      // (b)
    int32_t f[CAP];
    uint8_t back[2][CAP];   // per row: i - pred(i), 0 for -1
    uint32_t used[CAP / 32];
    // the read's list, after the last row
    int32_t score[RANK_MAX_CHAINS], strand[RANK_MAX_CHAINS], end[RANK_MAX_CHAINS], k[RANK_MAX_CHAINS], first[RANK_MAX_CHAINS];
    int32_t beg_fwd[RANK_MAX_CHAINS], end_fwd[RANK_MAX_CHAINS]; // the interval on the forward read
    int32_t parent[RANK_MAX_CHAINS], n_sub[RANK_MAX_CHAINS], subsc[RANK_MAX_CHAINS], off[RANK_MAX_CHAINS];
    int32_t m, anchors;
};
static_assert(sizeof(RankLds<RANK_CAP_SMALL>) <= 80 * 1024, "rows up to 4 096 candidates: two workgroups share a CU's 160 KiB of LDS");
static_assert(sizeof(RankLds<RANK_MAX_CAND>) <= 160 * 1024, "rows up to 8 192 candidates: one workgroup per CU");

// log2(x) in 1/256 units with a linear mantissa, x >= 1
__device__ inline int64_t rank_lg8(const int x)
{
    const int e = 31 - __clz(x);
    return ((int64_t)e << 8) + ((((int64_t)x << 8) >> e) - 256);
}

template <int CAP> __global__ __launch_bounds__(RANK_THREADS) void sw_rank_chains_kernel(const RankArgs a)
{
    __shared__ RankLds<CAP> s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    volatile uint32_t *const used = s.used; // (wave 0 reads what it has just written)
    const int two = a.strands == 2;

    for (int64_t p = blockIdx.x; p < a.n; p += a.groups) {
        const int64_t row = p * a.strands;
        auto finish = [&](const int m, const int anchors, const int status) {
            if (tid != 0) return;
            a.n_chains[p] = m;
            a.count[p] = anchors;
            if (a.status) a.status[p] = status;
        };
        // ---- the read's rows: lengths and ranges.  Row 1 of a one-strand read is an empty row that is not read
        const int64_t c00 = a.cand_start[row], c01 = a.cand_start[row + 1], c11 = two ? a.cand_start[row + 2] : c01;
        const int ql0 = a.row_q_len[row], ql1 = two ? a.row_q_len[row + 1] : 1;
        const int st0 = a.row_status ? a.row_status[row] : 0, st1 = !two ? 1 : a.row_status ? a.row_status[row + 1] : 0;
        if (ql0 < 1 || ql1 < 1 || c00 < 0 || c01 < c00 || c11 < c01 || c11 > a.total_cand) {
            finish(0, 0, ST_BAD_ARG);
            continue;
        }
        // ---- every pred of every row that is read
        bool mine = false;
#pragma nounroll
        for (int r = 0; r < a.strands; ++r) {
            if (r ? st1 : st0) continue;
            const int64_t c0 = r ? c01 : c00, cnt = (r ? c11 : c01) - c0;
            for (int64_t i = tid; i < cnt; i += RANK_THREADS) {
                const int64_t pr = a.pred[c0 + i];
                mine |= !(pr == -1 || (pr >= 0 && pr < i && i - pr <= RANK_MAX_PRED));
            }
        }
        if (__syncthreads_or(mine)) { // (a barrier too: the read before this one is done with LDS)
            finish(0, 0, ST_BAD_ARG);
            continue;
        }
        if (c01 - c00 > a.max_cand || c11 - c01 > a.max_cand || a.max_cand > CAP) {
            finish(0, 0, ST_UNSUPPORTED);
            continue;
        }

        // the list: entry j in lane j of wave 0, cnt of them
        int cnt = 0, l_score = 0, l_strand = 0, l_end = 0, l_k = 0, l_first = 0;
#pragma nounroll
        for (int r = 0; r < a.strands; ++r) {
            const int64_t c0 = r ? c01 : c00;
            const int N = (int)((r ? c11 : c01) - c0);
            if ((r ? st1 : st0) || N == 0) continue;
            uint8_t *const back = s.back[r];
            // ---- (a)
            const int n2 = seed_pow2(N);
            for (int i = tid; i < n2; i += RANK_THREADS) {
                if (i < N) {
                    const int fi = a.f[c0 + i], pr = a.pred[c0 + i];
                    s.f[i] = fi;
                    back[i] = (uint8_t)(pr < 0 ? 0 : i - pr);
                    s.key[i] = (uint64_t)(~((uint32_t)fi ^ 0x80000000u)) << 32 | (uint32_t)i;
                } else {
                    s.key[i] = ~0ull;
                }
            }
            for (int i = tid; i < (N + 31) / 32; i += RANK_THREADS) s.used[i] = 0;
            __syncthreads();
            // ---- (b)
            seed_bitonic(s.key, nullptr, n2);
            // ---- (c), (d)
            if (wave == 0) {
                bool done = false;
                for (int base = 0; base < N && !done; base += 64) {
                    const bool have = base + lane < N;
                    const int my_e = have ? (int)(uint32_t)s.key[base + lane] : 0;
                    const int my_f = have ? s.f[my_e] : 0;
                    for (;;) {
                        const bool unused = have && !((used[my_e >> 5] >> (my_e & 31)) & 1u);
                        const uint64_t open = __ballot(unused);
                        if (!open) break;
                        const int src = __ffsll((unsigned long long)open) - 1;
                        const int e = __shfl(my_e, src), fe = __shfl(my_f, src);
                        if (fe < a.min_score) {
                            done = true;
                            break;
                        }
                        // the walk, the same in every lane: i descends strictly (0 < back <= i was checked), every step marks one
                        int i = e, K = 0, first = e;
                        while (i >= 0) {
                            const uint32_t word = used[i >> 5], bit = 1u << (i & 31);
                            if (word & bit) break;
                            used[i >> 5] = word | bit;
                            ++K;
                            first = i;
                            const int b = back[i];
                            i = b == 0 ? -1 : i - b;
                        }
                        const int score = i < 0 ? fe : (int)((uint32_t)fe - (uint32_t)s.f[i]);
                        if (score < a.min_score || K < a.min_cnt) continue;
                        const bool ahead = lane < cnt && (l_score > score || (l_score == score && (l_strand < r || (l_strand == r && l_end < e))));
                        const int at = __popcll(__ballot(ahead));
                        if (at >= a.max_chains) continue;
                        const int u_score = __shfl_up(l_score, 1), u_strand = __shfl_up(l_strand, 1), u_end = __shfl_up(l_end, 1);
                        const int u_k = __shfl_up(l_k, 1), u_first = __shfl_up(l_first, 1);
                        if (lane > at) l_score = u_score, l_strand = u_strand, l_end = u_end, l_k = u_k, l_first = u_first;
                        if (lane == at) l_score = score, l_strand = r, l_end = e, l_k = K, l_first = first;
                        cnt = cnt + 1 < a.max_chains ? cnt + 1 : a.max_chains;
                    }
                }
            }
            __syncthreads(); // (the next row's keys, f and bitmap go where this row's are)
        }

        // ---- the list to LDS; the spans from the candidates of each chain's two ends
        if (wave == 0 && lane < RANK_MAX_CHAINS) {
            s.score[lane] = l_score;
            s.strand[lane] = l_strand;
            s.end[lane] = l_end;
            s.k[lane] = l_k;
            s.first[lane] = l_first;
            if (lane == 0) s.m = cnt;
        }
        __syncthreads();
        const int m = s.m;
        int strand = 0, t_beg = 0, t_end = 0, q_beg = 0, q_end = 0;
        if (tid < m) {
            strand = s.strand[tid];
            const int64_t c0 = strand ? c01 : c00;
            const int64_t ie = c0 + s.end[tid], ib = c0 + s.first[tid];
            const int le = a.cand_len[ie], ql = strand ? ql1 : ql0;
            t_beg = a.cand_t[ib];
            t_end = (int)((uint32_t)a.cand_t[ie] + (uint32_t)le);
            q_beg = a.cand_q[ib];
            q_end = (int)((uint32_t)a.cand_q[ie] + (uint32_t)le);
            s.beg_fwd[tid] = strand ? (int)((uint32_t)ql - (uint32_t)q_end) : q_beg;
            s.end_fwd[tid] = strand ? (int)((uint32_t)ql - (uint32_t)q_beg) : q_end;
        }
        __syncthreads();
        // ---- the parents: chain c against the earlier chains that are their own parent, in rank order
        if (tid == 0) {
            int off = 0;
            for (int c = 0; c < m; ++c) {
                s.parent[c] = c;
                s.n_sub[c] = 0;
                s.subsc[c] = 0;
                s.off[c] = off;
                off += s.k[c];
                const int64_t bc = s.beg_fwd[c], ec = s.end_fwd[c];
                for (int o = 0; o < c; ++o) {
                    if (s.parent[o] != o) continue;
                    const int64_t bo = s.beg_fwd[o], eo = s.end_fwd[o];
                    const int64_t span = (ec < eo ? ec : eo) - (bc > bo ? bc : bo), ov = span > 0 ? span : 0;
                    const int64_t lc = ec - bc, lo = eo - bo;
                    if (ov * 256 >= (int64_t)a.mask_level * (lc < lo ? lc : lo)) {
                        s.parent[c] = o;
                        s.n_sub[o] += 1;
                        s.subsc[o] = s.subsc[o] > s.score[c] ? s.subsc[o] : s.score[c];
                        break;
                    }
                }
            }
            s.anchors = off;
        }
        __syncthreads();
        // ---- the records, and the chains' candidates into the staging
        if (tid < m) {
            const int score = s.score[tid], K = s.k[tid], parent = s.parent[tid], e = s.end[tid];
            const bool primary = parent == tid;
            const int n_sub = primary ? s.n_sub[tid] : 0, subsc = primary ? s.subsc[tid] : 0;
            int mapq = 0;
            if (primary) { // (score >= min_score >= 1; the numerator is below 2^63 for every score below 2^31)
                const int floor = subsc > a.min_score ? subsc : a.min_score, sub = score < floor ? score : floor;
                const int64_t raw = (40 * (int64_t)(K < 10 ? K : 10) * (score - sub) * rank_lg8(score) * 177) / (10 * (int64_t)score * 65536);
                const int64_t q = raw - ((3 * rank_lg8(n_sub + 1) + 128) >> 8);
                mapq = (int)(q < 0 ? 0 : q > 60 ? 60 : q);
            }
            mgl_sw_ranked_chain rec;
            rec.score = score;
            rec.strand = strand;
            rec.n_anchors = K;
            rec.t_beg = t_beg;
            rec.t_end = t_end;
            rec.q_beg = q_beg;
            rec.q_end = q_end;
            rec.parent = parent;
            rec.n_sub = n_sub;
            rec.subsc = subsc;
            rec.mapq = mapq;
            rec.end_index = e;
            a.records[p * a.max_chains + tid] = rec;
            if (a.stage) { // K steps from the end: the chains of a read are disjoint, so the read's own range holds them all
                const uint8_t *const back = s.back[strand];
                const int64_t c0 = strand ? c01 : c00;
                int32_t *const stage = a.stage + c00 + s.off[tid];
                int i = e;
                for (int x = K - 1; x >= 0; --x) {
                    stage[x] = (int32_t)(c0 + i);
                    i -= back[i];
                }
            }
        }
        finish(m, a.stage ? s.anchors : 0, 0);
    }
}

__global__ __launch_bounds__(64) void sw_rank_pack_kernel(const RankArgs a)
{
    const int lane = threadIdx.x;
    for (int64_t p = blockIdx.x; p < a.n; p += gridDim.x) {
        const int64_t at = a.ranked_start[p];
        const int k = a.count[p];
        if (k == 0) continue;
        const int32_t *const stage = a.stage + a.cand_start[p * a.strands]; // (a read with a chain passed the range check)
        for (int x = lane; x < k; x += 64) {
            const int64_t src = stage[x], dst = at + x;
            if (src < 0 || src >= a.total_cand || dst >= a.total_cand) continue; // (ranges that overlap: sw_rank.h)
            a.ranked_t[dst] = a.cand_t[src];
            a.ranked_q[dst] = a.cand_q[src];
            a.ranked_len[dst] = a.cand_len[src];
        }
    }
}

} // namespace

hipError_t launch_rank_chains(const RankArgs &a, hipStream_t stream)
{
    if (a.n < 1) return hipSuccess;
    if ((a.strands != 1 && a.strands != 2) || a.n * a.strands > RANK_MAX_CHUNK || a.total_cand < 0 || a.total_cand > RANK_MAX_CHUNK || a.groups < 1)
        return hipErrorInvalidValue;
    if (a.max_cand < 0 || a.max_cand > RANK_MAX_CAND || a.max_chains < 1 || a.max_chains > RANK_MAX_CHAINS || a.min_score < 1 || a.min_cnt < 1 ||
        a.mask_level < 1 || a.mask_level > 256)
        return hipErrorInvalidValue;
    if (!a.row_q_len || !a.cand_start || !a.cand_t || !a.cand_q || !a.cand_len || !a.f || !a.pred || !a.count || !a.n_chains || !a.records)
        return hipErrorInvalidValue;
    if (a.max_cand <= RANK_CAP_SMALL) hipLaunchKernelGGL(sw_rank_chains_kernel<RANK_CAP_SMALL>, dim3((unsigned)a.groups), dim3(RANK_THREADS), 0, stream, a);
    else hipLaunchKernelGGL(sw_rank_chains_kernel<RANK_MAX_CAND>, dim3((unsigned)a.groups), dim3(RANK_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_rank_pack(const RankArgs &a, hipStream_t stream)
{
    if (a.n < 1 || a.total_cand < 1) return hipSuccess;
    if (!a.count || !a.stage || !a.cand_start || !a.ranked_start || !a.ranked_t || !a.ranked_q || !a.ranked_len) return hipErrorInvalidValue;
    const int64_t grid = a.n < 65536 ? a.n : 65536;
    hipLaunchKernelGGL(sw_rank_pack_kernel, dim3((unsigned)grid), dim3(64), 0, stream, a);
    return hipGetLastError();
}

} // namespace mgl_sw_dev
