// sw_describe.hip -- sw_describe_kernel (the definition is tests/describe_textbook.py's).  One wave per
// alignment, persistent over the batch; the four waves of a workgroup share nothing, each has its own part of LDS, and there is no
// workgroup barrier.
//
// Pass (a), the check: the CIGAR slot is read 64 bytes (text) or 64 words (binary) a step, a lane each.  In text the operation bytes
// are found by a ballot, and an operation's lane forms its number from the digits between the previous operation and itself -- the
// step's bytes lie in LDS for that -- or, where there is no operation in front of it in the step, behind the digits carried over from
// the steps before.  The lanes add up what their elements spend in 64 bits.  Nothing of the sequences is read before the slot has
// passed: every element M / I / D with 1 <= len < 2^31, no byte left over, and both sums equal to the spans.
// Pass (b): the slot is parsed again, now into LDS, DESCRIBE_CHUNK elements at a time (a step never yields more than 64, so a chunk is
// closed while 64 still fit): len, op and the element's offsets in the two spans, from a wave prefix scan.  The elements of a chunk are
// then taken in turn by the whole wave.  An M element goes 64 columns a step: one byte of either sequence a lane, the mismatches a
// 64-bit ballot, the counts its population count.  A mismatch lane finds the run in front of it from the previous set bit, or from the
// run carried into the step, and the = / X element that ends on a lane finds its length from the previous change of the mask.  Both
// token sizes go through one exclusive scan (packed 16 : 16) that places them behind the running offsets.  A D element is copied 64
// bases a step.  Every byte written is checked against its stride; the lengths run on regardless.
// The sequences are read a byte a lane, 64 consecutive bytes a load: nothing outside the spans.
#include "sw_describe.h"

#include "sw_cigar_wave.h"

namespace mgl_sw_dev {

namespace {

using namespace cigar_wave; // the check, the parse and the wave's part of LDS: sw_cigar_wave.h

__device__ __forceinline__ int ndigits(int v)
{
    int d = 1;
    for (unsigned x = (unsigned)v; x >= 10u; x /= 10u) ++d;
    return d;
}

// the decimal digits of v >= 0, the last one in front of byte `end`; bytes at or beyond `cap` are not written
__device__ __forceinline__ void put_number(char *const out, const int64_t end, int v, const int64_t cap)
{
    int64_t pos = end;
    do {
        --pos;
        if (pos < cap) out[pos] = (char)('0' + v % 10);
        v /= 10;
    } while (v > 0);
}

// what pass (b) carries from column to column; the same in every lane
struct Walk {
    char *md, *xc;       // this alignment's rows (or null)
    int64_t md_cap, xc_cap; // bytes that may be written: the stride, 0 for a null row
    bool binary, xwords;
    int64_t md_pos, xc_pos;
    int run;             // matches since the last MD token
    int cur_op, cur_len; // the extended CIGAR's element that is still open
    int n_match, n_mismatch, n_ins, n_del, n_ins_runs, n_del_runs;
};

__device__ __forceinline__ int xc_width(const Walk &w, const int len) { return w.binary ? 4 : ndigits(len) + 1; }

// one element of the extended CIGAR at byte `at`
__device__ __forceinline__ void put_xc(const Walk &w, const int64_t at, const int len, const int op)
{
    if (w.binary) {
        if (at + 4 > w.xc_cap) return; // whole words
        const uint32_t v = (uint32_t)len << 4 | (uint32_t)op;
        if (w.xwords) {
            *reinterpret_cast<uint32_t *>(w.xc + at) = v;
        } else {
            w.xc[at] = (char)(v & 0xff);
            w.xc[at + 1] = (char)((v >> 8) & 0xff);
            w.xc[at + 2] = (char)((v >> 16) & 0xff);
            w.xc[at + 3] = (char)(v >> 24);
        }
    } else {
        const int64_t end = at + ndigits(len) + 1;
        if (end - 1 < w.xc_cap) w.xc[end - 1] = op == OP_EQ ? '=' : op == OP_X ? 'X' : op == OP_I ? 'I' : 'D';
        put_number(w.xc, end - 1, len, w.xc_cap);
    }
}

// the open element is closed: written behind what stands, by lane 0
__device__ __forceinline__ void flush_xc(Walk &w, const int lane)
{
    if (w.cur_op != OP_NONE && w.cur_len > 0) {
        if (lane == 0) put_xc(w, w.xc_pos, w.cur_len, w.cur_op);
        w.xc_pos += xc_width(w, w.cur_len);
    }
    w.cur_op = OP_NONE;
    w.cur_len = 0;
}

__device__ __forceinline__ void gap_xc(Walk &w, const int lane, const int len, const int op)
{
    if (w.cur_op != op) {
        flush_xc(w, lane);
        w.cur_op = op;
    }
    w.cur_len += len;
}

// an M element of `len` columns: T[0 .. len) against Q[0 .. len)
__device__ __forceinline__ void walk_match(Walk &w, const int lane, const uint8_t *const T, const uint8_t *const Q, const int len)
{
    const uint64_t lt = ((uint64_t)1 << lane) - 1;
    for (int c0 = 0; c0 < len; c0 += 64) {
        const int cnt = min(64, len - c0);
        const bool in = lane < cnt;
        const uint8_t tb = in ? T[c0 + lane] : (uint8_t)0, qb = in ? Q[c0 + lane] : (uint8_t)0;
        const uint64_t mm = __ballot(in && tb != qb);
        const uint64_t valid = cnt == 64 ? ~(uint64_t)0 : ((uint64_t)1 << cnt) - 1;
        const int nmm = __popcll(mm);
        w.n_mismatch += nmm;
        w.n_match += cnt - nmm;
        // ---- MD: a mismatch lane's token is the run in front of it and the target byte
        const bool ismm = (mm >> lane) & 1;
        const uint64_t below = mm & lt;
        const int myrun = below ? lane - top_bit(below) - 1 : w.run + lane;
        const int mdw = ismm ? ndigits(myrun) + 1 : 0;
        // ---- = / X: the step's first column closes the open element or goes on with it; an element ends on the lane in front of a change
        const int f0 = (mm & 1) ? OP_X : OP_EQ;
        if (w.cur_op != f0) {
            flush_xc(w, lane);
            w.cur_op = f0;
        }
        const uint64_t ends = (mm ^ (mm >> 1)) & (valid >> 1);
        const bool isend = (ends >> lane) & 1;
        const uint64_t ebelow = ends & lt;
        const int start = ebelow ? top_bit(ebelow) + 1 : 0;
        const int elen = lane - start + 1 + (start == 0 ? w.cur_len : 0);
        const int xw = isend ? xc_width(w, elen) : 0;
        // ---- one scan places both kinds of token
        int incl = mdw | xw << 16;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        if (ismm) {
            const int64_t end = w.md_pos + (incl & 0xffff);
            if (end - 1 < w.md_cap) w.md[end - 1] = (char)tb;
            put_number(w.md, end - 1, myrun, w.md_cap);
        }
        if (isend) put_xc(w, w.xc_pos + (incl >> 16) - xw, elen, ismm ? OP_X : OP_EQ);
        const int tot = __shfl(incl, 63);
        w.md_pos += tot & 0xffff;
        w.xc_pos += tot >> 16;
        w.run = mm ? cnt - 1 - top_bit(mm) : w.run + cnt;
        if (ends) {
            w.cur_len = cnt - (top_bit(ends) + 1);
            w.cur_op = ((mm >> (cnt - 1)) & 1) ? OP_X : OP_EQ;
        } else {
            w.cur_len += cnt;
        }
    }
}

// a D element: the run in front of it, `^`, its target bytes
__device__ __forceinline__ void walk_deletion(Walk &w, const int lane, const uint8_t *const T, const int len)
{
    const int dg = ndigits(w.run);
    if (lane == 0) {
        put_number(w.md, w.md_pos + dg, w.run, w.md_cap);
        if (w.md_pos + dg < w.md_cap) w.md[w.md_pos + dg] = '^';
    }
    const int64_t at = w.md_pos + dg + 1;
    for (int c = lane; c < len; c += 64)
        if (at + c < w.md_cap) w.md[at + c] = (char)T[c];
    w.md_pos = at + len;
    w.run = 0;
}

__global__ __launch_bounds__(64 * DESCRIBE_WAVES) void sw_describe_kernel(const DescribeArgs a)
{
    __shared__ WaveLds lds[DESCRIBE_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    WaveLds &L = lds[wave];
    const int64_t waves = (int64_t)gridDim.x * DESCRIBE_WAVES;
    for (int64_t p = (int64_t)blockIdx.x * DESCRIBE_WAVES + wave; p < a.n; p += waves) {
        auto finish = [&](const int status, const Walk &w) {
            if (lane == 0) {
                mgl_sw_alignment_stats s;
                s.n_match = w.n_match;
                s.n_mismatch = w.n_mismatch;
                s.n_ins = w.n_ins;
                s.n_del = w.n_del;
                s.n_ins_runs = w.n_ins_runs;
                s.n_del_runs = w.n_del_runs;
                s.md_len = (int)min(w.md_pos, (int64_t)0x7fffffff);
                s.xcigar_len = (int)min(w.xc_pos, (int64_t)0x7fffffff);
                a.stats[p] = s;
                if (a.status) a.status[p] = status;
            }
        };
        Walk w{};
        w.cur_op = OP_NONE;
        const int sin = a.status_in ? a.status_in[p] : 0;
        if (sin != 0) { // nothing of the alignment is read
            finish(sin, w);
            continue;
        }
        const mgl_sw_chain_alignment r = a.aln[p];
        Parser P{};
        // ---- pass (a): the slot alone
        const bool ok = check_alignment(P, L, lane, r, a.t_len[p], a.q_len[p], a.cigar_len[p], a.cigar + p * (int64_t)a.cigar_stride, a.cigar_stride, a.binary);
        if (!ok) {
            finish(MGL_SW_ERR_BAD_ARG, w);
            continue;
        }
        // ---- pass (b): chunk by chunk
        const uint8_t *const T = a.targets + a.t_start[p] + r.t_beg, *const Q = a.queries + a.q_start[p] + r.q_beg;
        w.md = a.md ? a.md + p * (int64_t)a.md_stride : nullptr;
        w.xc = a.xcigar ? a.xcigar + p * (int64_t)a.xcigar_stride : nullptr;
        w.md_cap = a.md ? a.md_stride : 0;
        w.xc_cap = a.xcigar ? a.xcigar_stride : 0;
        w.binary = P.binary;
        w.xwords = (reinterpret_cast<uintptr_t>(w.xc) & 3) == 0;
        rewind(P);
        while (P.pos < P.bytes) {
            int count = 0;
            while (P.pos < P.bytes && count + 64 <= DESCRIBE_CHUNK) count += parse_step<true>(P, L, lane, count);
            wave_sync();
            for (int e = 0; e < count; ++e) {
                const int len = L.len[e], op = L.op[e], to = L.toff[e], qo = L.qoff[e];
                if (op == OP_M) {
                    walk_match(w, lane, T + to, Q + qo, len);
                } else if (op == OP_I) {
                    w.n_ins += len;
                    w.n_ins_runs += 1;
                    gap_xc(w, lane, len, OP_I);
                } else {
                    w.n_del += len;
                    w.n_del_runs += 1;
                    gap_xc(w, lane, len, OP_D);
                    walk_deletion(w, lane, T + to, len);
                }
            }
            wave_sync(); // the chunk is written again
        }
        if (lane == 0) put_number(w.md, w.md_pos + ndigits(w.run), w.run, w.md_cap);
        w.md_pos += ndigits(w.run);
        flush_xc(w, lane);
        const bool over = (a.md && w.md_pos > w.md_cap) || (a.xcigar && w.xc_pos > w.xc_cap);
        finish(over ? MGL_SW_ERR_CIGAR_OVERFLOW : MGL_SW_OK, w);
    }
}

} // namespace

hipError_t launch_describe(const DescribeArgs &a, hipStream_t stream)
{
    if (a.n < 1) return hipSuccess;
    if (a.n > DESCRIBE_MAX_CHUNK || a.groups < 1 || a.cigar_stride < 0) return hipErrorInvalidValue;
    if (!a.targets || !a.queries || !a.t_start || !a.q_start || !a.t_len || !a.q_len || !a.aln || !a.cigar || !a.cigar_len || !a.stats)
        return hipErrorInvalidValue;
    if ((a.md && a.md_stride < 1) || (a.xcigar && (a.xcigar_stride < 1 || (a.binary && (a.xcigar_stride & 3))))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_describe_kernel, dim3((unsigned)a.groups), dim3(64 * DESCRIBE_WAVES), 0, stream, a);
    return hipGetLastError();
}

} // namespace mgl_sw_dev
