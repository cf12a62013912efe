// sw_lines.hip -- the kernels of mgl_sw_expand_chains_batch_device and mgl_sw_classify_alignments_batch_device (the
// functions are tests/lines_textbook.py's).  sw_lines.h describes the workspace the first four share with the host side.
//
// sw_expand_count_kernel: a thread per read.  The read is checked -- its place in the query buffer, its chain count, every record, its
// range of ranked anchors against the records' sum -- and its jobs, their anchors and their strands are counted into the workspace.
// sw_expand_scan_kernel: one block, 1024 reads a step, two running sums (jobs, anchors).  While a step's reads all fit the capacities
// it is a prefix sum; in a step where they do not, thread 0 walks the step's 1024 counts in LDS, read after read, and drops the reads
// that do not fit (the rule is greedy, so it is serial: only a batch that overflows pays for it), and the sums are taken again.
// sw_expand_pack_kernel: a wave per read, lane c on chain c: the job records, the three per-job arrays, then the anchors of job after
// job, 64 a step; behind the reads the whole grid writes the empty tail.
// sw_expand_orient_kernel: a workgroup per (read, strand) that has a job.  Bytes up to the first 16-byte border of the DESTINATION,
// 16-byte blocks, bytes behind the last border; a block of the reverse half is the block of the read that mirrors it, loaded whole,
// its bytes reversed and complemented in registers.  The loads are as aligned as the read's place in the caller's buffer is.
//
// sw_classify_kernel: a quarter wave per read, lane j of the quarter on job j, no LDS.  The place of a live job among the read's lines
// comes from counting the jobs ahead of it (16 lane reads); the lines then sit in the quarter's lanes in line order, the parent loop
// is at most 15 serial steps of one ballot each, and every job fetches its line's record from the lane that holds it.
// All writes are plain vector stores.
#include "sw_lines.h"

#include <algorithm>

namespace mgl_sw_dev {

namespace {

constexpr int ST_BAD_ARG = 1, ST_NOMEM = 3; // mgl_sw_status

static_assert(sizeof(mgl_sw_job) == 32 && sizeof(mgl_sw_line) == 32, "eight int32 each");

// ---------------------------------------------------------------------------------------------------------------- expand: count

__global__ __launch_bounds__(256) void sw_expand_count_kernel(const ExpandArgs a)
{
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < a.n; p += (int64_t)gridDim.x * 256) {
        int jobs = 0, anchors = 0, strands = 0, status = a.rank_status ? a.rank_status[p] : 0;
        if (status == 0) {
            const int64_t ql = a.q_len[p], qs = a.q_start[p], r0 = a.ranked_start[p], r1 = a.ranked_start[p + 1];
            const int nc = a.n_chains[p];
            bool bad = ql < 1 || qs < 0 || qs > a.query_bytes - ql || nc < 0 || nc > a.max_chains || r0 < 0 || r1 < r0 || r1 > a.total_anchors;
            int64_t sum = 0, kept = 0;
            if (!bad) {
                const mgl_sw_ranked_chain *const rec = a.records + p * a.max_chains;
                for (int c = 0; c < nc; ++c) {
                    const int strand = rec[c].strand, k = rec[c].n_anchors;
                    if ((strand != 0 && strand != 1) || k < 1) {
                        bad = true;
                        break;
                    }
                    sum += k;
                    if (a.keep_secondary || rec[c].parent == c) {
                        ++jobs;
                        kept += k;
                        strands |= 1 << strand;
                    }
                }
                bad = bad || sum != r1 - r0; // (so kept <= total_anchors <= 2^30: it fits the int32)
            }
            if (bad) jobs = 0, kept = 0, strands = 0, status = ST_BAD_ARG;
            anchors = (int)kept;
        }
        a.ws_jobs[p] = jobs;
        a.ws_anchors[p] = anchors;
        a.ws_strands[p] = strands;
        if (a.status) a.status[p] = status;
    }
}

// ---------------------------------------------------------------------------------------------------------------- expand: scan

__device__ inline int64_t lines_wave_sum(int64_t v, const int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t up = __shfl_up(v, d);
        if (lane >= d) v += up;
    }
    return v;
}

__global__ __launch_bounds__(1024) void sw_expand_scan_kernel(const ExpandArgs a)
{
    __shared__ int64_t wave_jobs[16], wave_anchors[16];
    __shared__ int32_t step_jobs[1024], step_anchors[1024];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t carry_j = 0, carry_a = 0;
    for (int64_t base = 0; base < a.n; base += 1024) {
        const int64_t p = base + tid;
        int own_j = p < a.n ? a.ws_jobs[p] : 0, own_a = p < a.n ? a.ws_anchors[p] : 0;
        int64_t excl_j = 0, excl_a = 0, all_j = 0, all_a = 0;
        auto sums = [&]() {
            const int64_t incl_j = lines_wave_sum(own_j, lane), incl_a = lines_wave_sum(own_a, lane);
            if (lane == 63) wave_jobs[wave] = incl_j, wave_anchors[wave] = incl_a;
            __syncthreads();
            int64_t before_j = 0, before_a = 0;
            all_j = 0, all_a = 0;
            for (int x = 0; x < 16; ++x) {
                const int64_t sj = wave_jobs[x], sa = wave_anchors[x];
                before_j += x < wave ? sj : 0;
                before_a += x < wave ? sa : 0;
                all_j += sj;
                all_a += sa;
            }
            excl_j = carry_j + before_j + incl_j - own_j;
            excl_a = carry_a + before_a + incl_a - own_a;
            __syncthreads(); // (the sums may be taken again)
        };
        sums();
        if (carry_j + all_j > a.job_capacity || carry_a + all_a > a.total_anchors) { // (the same in every thread)
            step_jobs[tid] = own_j;
            step_anchors[tid] = own_a;
            __syncthreads();
            if (tid == 0) {
                int64_t run_j = carry_j, run_a = carry_a;
                for (int i = 0; i < 1024; ++i) {
                    const int j = step_jobs[i], k = step_anchors[i];
                    if (run_j + j > a.job_capacity || run_a + k > a.total_anchors) step_jobs[i] = -1;
                    else run_j += j, run_a += k;
                }
            }
            __syncthreads();
            if (step_jobs[tid] < 0) { // (p < n: a read beyond n has no jobs and is never dropped)
                own_j = 0, own_a = 0;
                a.ws_jobs[p] = 0;
                a.ws_anchors[p] = 0;
                a.ws_strands[p] = 0;
                if (a.status) a.status[p] = ST_NOMEM;
            }
            sums();
        }
        if (p < a.n) {
            a.job_start[p] = excl_j;
            a.ws_anchor_at[p] = excl_a;
        }
        carry_j += all_j;
        carry_a += all_a;
    }
    if (tid == 0) {
        a.job_start[a.n] = carry_j;
        a.n_jobs[0] = carry_j;
        a.job_anchor_start[carry_j] = carry_a; // (carry_j <= job_capacity: the array has job_capacity + 1 entries)
    }
}

// ---------------------------------------------------------------------------------------------------------------- expand: pack

__global__ __launch_bounds__(64) void sw_expand_pack_kernel(const ExpandArgs a)
{
    const int lane = threadIdx.x;
    for (int64_t p = blockIdx.x; p < a.n; p += gridDim.x) {
        const int jobs = a.ws_jobs[p];
        if (jobs == 0) continue; // (a read that was refused or cut, or one without chains)
        // the read passed the checks: nc <= max_chains <= 16, its records and its range are good, and the scan kept it inside both
        // capacities
        const int nc = a.n_chains[p], ql = a.q_len[p];
        const int64_t qs = a.q_start[p], j0 = a.job_start[p], at0 = a.ws_anchor_at[p], r0 = a.ranked_start[p];
        mgl_sw_ranked_chain rec{};
        if (lane < nc) rec = a.records[p * a.max_chains + lane];
        const bool kept = lane < nc && (a.keep_secondary || rec.parent == lane);
        const int k = lane < nc ? rec.n_anchors : 0;
        // where the chain's anchors lie behind the read's first (all chains count) and where the job's go (the kept ones do)
        int src = k, dst = kept ? k : 0;
#pragma unroll
        for (int d = 1; d < LINES_MAX_CHAINS; d <<= 1) {
            const int us = __shfl_up(src, d), ud = __shfl_up(dst, d);
            if (lane >= d) src += us, dst += ud;
        }
        src -= k;
        dst -= kept ? k : 0;
        const int at = __popcll(__ballot(kept) & ((1ull << lane) - 1)); // the job's place among the read's
        if (kept && j0 + at < a.job_capacity) {
            const int64_t j = j0 + at;
            mgl_sw_job job;
            job.read = (int32_t)p;
            job.rank = lane;
            job.strand = rec.strand;
            job.n_anchors = k;
            job.chain_score = rec.score;
            job.chain_parent = rec.parent;
            job.q_len = ql;
            job.reserved = 0;
            a.jobs[j] = job;
            a.job_q_start[j] = qs + (rec.strand ? a.query_bytes : 0);
            a.job_q_len[j] = ql;
            a.job_anchor_start[j] = at0 + dst;
        }
        for (int c = 0; c < nc; ++c) {
            if (!__shfl((int)kept, c)) continue;
            const int kc = __shfl(k, c);
            const int64_t from = r0 + __shfl(src, c), to = at0 + __shfl(dst, c);
            if (from < 0 || from + kc > a.total_anchors || to < 0 || to + kc > a.total_anchors) continue; // (the checks and the scan: this holds)
            for (int x = lane; x < kc; x += 64) {
                a.job_anchor_t[to + x] = a.ranked_t[from + x];
                a.job_anchor_q[to + x] = a.ranked_q[from + x];
                a.job_anchor_len[to + x] = a.ranked_len[from + x];
            }
        }
    }
    // ---- the empty tail: jobs n_jobs .. job_capacity, and the anchor starts behind the one the scan wrote
    const int64_t n_jobs = a.job_start[a.n];
    if (n_jobs < 0 || n_jobs > a.job_capacity) return;
    const int64_t end = a.n > 0 ? a.ws_anchor_at[a.n - 1] + a.ws_anchors[a.n - 1] : 0;
    for (int64_t j = n_jobs + (int64_t)blockIdx.x * 64 + lane; j < a.job_capacity; j += (int64_t)gridDim.x * 64) {
        mgl_sw_job job{};
        job.read = -1;
        a.jobs[j] = job;
        a.job_q_start[j] = 0;
        a.job_q_len[j] = 0;
        a.job_anchor_start[j + 1] = end;
    }
}

// ---------------------------------------------------------------------------------------------------------------- expand: orient

__device__ inline uint32_t lines_comp(const uint32_t b) { return b == 'A' ? 'T' : b == 'T' ? 'A' : b == 'C' ? 'G' : b == 'G' ? 'C' : b; }

// the four bytes of a word reversed and complemented
__device__ inline uint32_t lines_rc_word(const uint32_t w)
{
    return lines_comp(w >> 24) | lines_comp((w >> 16) & 255u) << 8 | lines_comp((w >> 8) & 255u) << 16 | lines_comp(w & 255u) << 24;
}

__global__ __launch_bounds__(LINES_ORIENT_THREADS) void sw_expand_orient_kernel(const ExpandArgs a)
{
    const int tid = threadIdx.x;
    for (int64_t work = blockIdx.x; work < 2 * a.n; work += a.groups) {
        const int64_t p = work >> 1;
        const int strand = (int)(work & 1);
        if (!((a.ws_strands[p] >> strand) & 1)) continue; // (0 for a read that was refused or cut)
        // the read passed the checks: 1 <= ql and [qs, qs + ql) lies in [0, query_bytes)
        const int ql = a.q_len[p];
        const int64_t qs = a.q_start[p];
        const uint8_t *const src = a.queries + qs;
        uint8_t *const dst = a.oriented + (strand ? a.query_bytes : 0) + qs;
        const int to_border = (int)(-reinterpret_cast<uintptr_t>(dst) & 15);
        const int head = to_border < ql ? to_border : ql, blocks = (ql - head) >> 4, tail = head + 16 * blocks;
        // bytes [0, head) and [tail, ql): fewer than 16 each
        for (int i = tid; i < head + (ql - tail); i += LINES_ORIENT_THREADS) {
            const int at = i < head ? i : tail + (i - head);
            dst[at] = strand ? (uint8_t)lines_comp(src[ql - 1 - at]) : src[at];
        }
        for (int b = tid; b < blocks; b += LINES_ORIENT_THREADS) {
            const int at = head + 16 * b; // at + 16 <= tail <= ql
            uint4 v;
            if (strand) { // oriented[at + x] = comp(src[ql - 1 - at - x]): the block src[ql - 16 - at .. ql - at), backwards
                uint4 u;
                __builtin_memcpy(&u, src + (ql - 16 - at), 16); // ql - 16 - at >= ql - tail >= 0
                v.x = lines_rc_word(u.w);
                v.y = lines_rc_word(u.z);
                v.z = lines_rc_word(u.y);
                v.w = lines_rc_word(u.x);
            } else {
                __builtin_memcpy(&v, src + at, 16);
            }
            *reinterpret_cast<uint4 *>(dst + at) = v; // (dst + head is on a 16-byte border)
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- classify

// log2(x) in 1/256 units with a linear mantissa, x >= 1 (sw_rank.hip's)
__device__ inline int64_t lines_lg8(const int x)
{
    const int e = 31 - __clz(x);
    return ((int64_t)e << 8) + ((((int64_t)x << 8) >> e) - 256);
}

__global__ __launch_bounds__(256) void sw_classify_kernel(const ClassifyArgs a)
{
    const int lane = threadIdx.x & 63, q = lane & 15, qbase = lane & 48; // the quarter's lane 0 in the wave
    const int64_t quarters = (int64_t)gridDim.x * 16, first = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    // every lane of a wave runs the same number of turns: the shuffles and ballots below want the whole wave
    const int64_t turns = (a.n + quarters - 1) / quarters;
    for (int64_t turn = 0; turn < turns; ++turn) {
        const int64_t p = first + turn * quarters;
        const bool read = p < a.n;
        const int64_t j0 = read ? a.job_start[p] : 0, j1 = read ? a.job_start[p + 1] : 0;
        bool bad = j0 < 0 || j1 < j0 || j1 > a.job_capacity || j1 - j0 > LINES_MAX_CHAINS;
        const int m = read && !bad ? (int)(j1 - j0) : 0;
        const bool mine = q < m;
        mgl_sw_job job{};
        if (mine) job = a.jobs[j0 + q];
        // a job of another read: the whole read is refused
        const int wrong = (int)((__ballot(mine && job.read != p) >> qbase) & 0xffffu);
        bad = bad || wrong != 0;
        // ---- live jobs and their place among the read's lines
        int score = 0, beg = 0, end = 0;
        bool live = false;
        if (mine && !bad && a.aln_status[j0 + q] == 0) {
            const mgl_sw_chain_alignment al = a.aln[j0 + q];
            live = al.q_end > al.q_beg && al.score >= 1;
            if (live) {
                score = al.score;
                beg = job.strand ? (int)((uint32_t)job.q_len - (uint32_t)al.q_end) : al.q_beg;
                end = job.strand ? (int)((uint32_t)job.q_len - (uint32_t)al.q_beg) : al.q_end;
            }
        }
        int order = 0;
#pragma unroll
        for (int k = 0; k < LINES_MAX_CHAINS; ++k) {
            const int o_live = __shfl((int)live, qbase + k), o_score = __shfl(score, qbase + k), o_rank = __shfl(job.rank, qbase + k);
            order += o_live && (o_score > score || (o_score == score && (o_rank < job.rank || (o_rank == job.rank && k < q))));
        }
        const int L = __popc((unsigned)((__ballot(live) >> qbase) & 0xffffu));
        if (!live) order = -1;
        // ---- the lines in line order: lane c of the quarter takes line c from the job that has it
        int from = 0;
#pragma unroll
        for (int k = 0; k < LINES_MAX_CHAINS; ++k)
            if (__shfl(order, qbase + k) == q) from = k;
        const bool line = q < L;
        const int l_score = __shfl(score, qbase + from), l_beg = __shfl(beg, qbase + from), l_end = __shfl(end, qbase + from);
        const int l_strand = __shfl(job.strand, qbase + from), l_k = __shfl(job.n_anchors, qbase + from), l_chain = __shfl(job.chain_score, qbase + from);
        // ---- parents: line c against the earlier lines that are their own parent; the first that fits wins
        int parent = q, n_sub = 0, subsc = 0, csub = 0;
#pragma unroll 1
        for (int c = 1; c < LINES_MAX_CHAINS; ++c) {
            const int64_t bc = __shfl(l_beg, qbase + c), ec = __shfl(l_end, qbase + c);
            const int sc = __shfl(l_score, qbase + c), cc = __shfl(l_chain, qbase + c);
            const int64_t span = (ec < l_end ? ec : (int64_t)l_end) - (bc > l_beg ? bc : (int64_t)l_beg), ov = span > 0 ? span : 0;
            const int64_t lc = ec - bc, lo = (int64_t)l_end - l_beg;
            const bool fits = c < L && q < c && parent == q && ov * 256 >= (int64_t)a.mask_level * (lc < lo ? lc : lo);
            const int found = (int)((__ballot(fits) >> qbase) & 0xffffu);
            const int o = __ffs(found) - 1; // -1: no line fits
            if (q == c && o >= 0) parent = o;
            if (q == o) {
                ++n_sub;
                if (sc > subsc) subsc = sc, csub = cc;
            }
        }
        // ---- flags and mapping quality, per line
        const bool own = parent == q;
        int flag = 0, mapq = 0;
        if (line) {
            flag = (l_strand ? 0x10 : 0) | (!own ? 0x100 : q > 0 ? 0x800 : 0);
            if (own) {
                const int64_t c1 = l_chain > 1 ? l_chain : 1, floor = csub > a.min_score ? csub : a.min_score;
                const int64_t r_chain = ((c1 < floor ? c1 : floor) << 16) / c1;
                const int64_t r_aln = n_sub > 0 ? ((int64_t)subsc << 16) / l_score : 65536;
                const int64_t x = (r_chain * r_aln) >> 16;
                const int per = l_score / a.match;
                const int64_t raw = (40 * (int64_t)(l_k < 10 ? l_k : 10) * (65536 - x) * lines_lg8(per > 1 ? per : 1) * 177) / (10 * (int64_t)65536 * 65536);
                const int64_t mq = raw - ((3 * lines_lg8(n_sub + 1) + 128) >> 8);
                mapq = (int)(mq < 0 ? 0 : mq > 60 ? 60 : mq);
            } else {
                n_sub = 0, subsc = 0;
            }
        }
        // ---- back to the jobs: job q fetches the record of its line, and the job index of that line's parent
        const int at = qbase + (live ? order : 0);
        const int j_flag = __shfl(flag, at), j_mapq = __shfl(mapq, at), j_parent = __shfl(parent, at), j_nsub = __shfl(n_sub, at), j_subsc = __shfl(subsc, at);
        const int j_pjob = __shfl(from, qbase + (live ? j_parent : 0)); // the job that holds the parent line
        const int prim = __shfl(from, qbase);
        if (mine && !bad) {
            mgl_sw_line out{};
            out.order = -1;
            out.parent = -1;
            if (live) {
                out.order = order;
                out.flag = j_flag;
                out.mapq = j_mapq;
                out.parent = (int32_t)(j0 + j_pjob);
                out.n_sub = j_nsub;
                out.subsc = j_subsc;
                out.fwd_q_beg = beg;
                out.fwd_q_end = end;
            }
            a.lines[j0 + q] = out;
        }
        if (read && q == 0) {
            a.n_lines[p] = bad ? 0 : L;
            a.primary_job[p] = !bad && L > 0 ? (int32_t)(j0 + prim) : -1;
            if (a.status) a.status[p] = bad ? ST_BAD_ARG : 0;
        }
    }
}

} // namespace

hipError_t launch_expand_count(const ExpandArgs &a, hipStream_t stream)
{
    if (a.n < 1) return hipSuccess;
    if (a.n > LINES_MAX_READS || a.max_chains < 1 || a.max_chains > LINES_MAX_CHAINS || a.total_anchors < 0 || a.query_bytes < 0) return hipErrorInvalidValue;
    if (!a.q_start || !a.q_len || !a.n_chains || !a.records || !a.ranked_start || !a.ws_jobs || !a.ws_anchors || !a.ws_strands) return hipErrorInvalidValue;
    const int64_t blocks = (a.n + 255) / 256;
    hipLaunchKernelGGL(sw_expand_count_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_expand_scan(const ExpandArgs &a, hipStream_t stream)
{
    if (a.n < 0 || a.n > LINES_MAX_READS || a.job_capacity < 0 || a.job_capacity > LINES_MAX_JOBS || a.total_anchors < 0) return hipErrorInvalidValue;
    if (!a.n_jobs || !a.job_start || !a.job_anchor_start || (a.n > 0 && (!a.ws_jobs || !a.ws_anchors || !a.ws_strands || !a.ws_anchor_at))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_expand_scan_kernel, dim3(1), dim3(1024), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_expand_pack(const ExpandArgs &a, hipStream_t stream)
{
    if (a.n < 0 || a.job_capacity < 0 || a.job_capacity > LINES_MAX_JOBS) return hipErrorInvalidValue;
    if (a.n < 1 && a.job_capacity < 1) return hipSuccess;
    if (!a.jobs || !a.job_q_start || !a.job_q_len || !a.job_anchor_start || !a.job_start) return hipErrorInvalidValue;
    if (a.n > 0 && (!a.ws_jobs || !a.ws_anchors || !a.ws_anchor_at || !a.job_anchor_t || !a.job_anchor_q || !a.job_anchor_len || !a.ranked_t || !a.ranked_q || !a.ranked_len))
        return hipErrorInvalidValue;
    const int64_t want = std::max<int64_t>(a.n, (a.job_capacity + 63) / 64), grid = want < 65536 ? want : 65536;
    hipLaunchKernelGGL(sw_expand_pack_kernel, dim3((unsigned)std::max<int64_t>(grid, 1)), dim3(64), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_expand_orient(const ExpandArgs &a, hipStream_t stream)
{
    if (a.n < 1) return hipSuccess;
    if (!a.queries || !a.oriented || !a.ws_strands || !a.q_start || !a.q_len || a.groups < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_expand_orient_kernel, dim3((unsigned)a.groups), dim3(LINES_ORIENT_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_classify(const ClassifyArgs &a, hipStream_t stream)
{
    if (a.n < 1) return hipSuccess;
    if (a.n > LINES_MAX_READS || a.job_capacity < 0 || a.job_capacity > LINES_MAX_JOBS || a.match < 1 || a.min_score < 1 || a.mask_level < 1 || a.mask_level > 256)
        return hipErrorInvalidValue;
    if (!a.job_start || !a.jobs || !a.aln || !a.aln_status || !a.lines || !a.n_lines || !a.primary_job) return hipErrorInvalidValue;
    const int64_t blocks = (a.n + 15) / 16;
    hipLaunchKernelGGL(sw_classify_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

} // namespace mgl_sw_dev
