// sw_chain.hip -- the three kernels that mgl_sw_align_chain_batch_device puts around the extension kernels (the
// function is tests/chain_textbook.py's): sw_chain_split_kernel in front of them, sw_gap_fill_kernel and sw_chain_join_kernel behind.
// sw_chain.h describes the staging they share with the host side.
//
// The split, one wave per pair, checks the pair's range of d_anchor_start and its anchors 64 at a time, claims the range's anchors,
// and then does what sw_seed_split_kernel does for a seed: the four flank descriptors -- the left flank is what lies in front of the
// first anchor, the right one what lies behind the last -- and the reversed copies of the left flanks, 64 bytes a step.
//
// The fill is the hot path: one wave per gap, persistent on workspace slots like sw_banded_kernel and built from the same parts
// (sw_band_wave.h): gap-penalty borders on both axes, the banded entry's band rule, sweep_strip<false> strip by strip, and the walk from
// the fixed start cell (gt, gq).  There are no end-cell scans: the one value it keeps is H(gt, gq), h_last of the lane on row gt in the
// last strip.  It writes the score, a status, the length and a binary row per gap.  Gaps with gt = 0 or gq = 0 are skipped, as are
// the anchors that have no gap behind them: the join works those out itself and reads nothing the fill did not write.
//
// The join, one wave per pair, adds the anchors' scores up (64 columns a step), the gaps' and the sides' contributions, and writes the
// joined CIGAR in two passes of the same code, one that counts and one that writes, so that a pair that overflows writes nothing.  A
// pass runs over the segments in order with one running M: an anchor adds its length to it, a segment's leading M joins it, and it
// is written out in front of the first element that is not an M; a segment's trailing M starts the next one.  What lies between a
// segment's first and last element is copied 64 elements a step, a prefix sum of their widths placing each lane's.  The per-anchor
// values of 64 anchors are loaded by 64 lanes at once and handed round with readlane.
#include "sw_band_wave.h"
#include "sw_chain.h"

namespace mgl_sw_dev {

namespace {

__global__ __launch_bounds__(64) void sw_chain_split_kernel(const ChainArgs a)
{
    const int lane = threadIdx.x;
    const int64_t p = blockIdx.x;
    const int tl = a.t_len[p], ql = a.q_len[p];
    const int64_t a0 = a.anchor_start[p], a1 = a.anchor_start[p + 1];
    const bool range = a0 >= 0 && a1 > a0 && a1 <= a.total_anchors;
    bool ok = range && tl >= 1 && ql >= 1 && tl <= a.max_tl && ql <= a.max_ql;
    int st0 = 0, sq0 = 0, tend = 0, qend = 0; // the first anchor's start, the last one's end
    if (range) {
        bool bad = false;
        for (int64_t i = a0 + lane; i < a1; i += 64) {
            atomicMin(&a.owner[i], (int)p);
            const int st = a.anchor_t[i], sq = a.anchor_q[i], sl = a.anchor_len[i];
            const bool last = i + 1 == a1;
            const int64_t nt = last ? tl : a.anchor_t[i + 1], nq = last ? ql : a.anchor_q[i + 1]; // what the anchor must end in front of
            bad |= !(sl >= 1 && st >= 0 && sq >= 0 && (int64_t)st + sl <= nt && (int64_t)sq + sl <= nq);
        }
        ok = ok && __ballot(bad) == 0;
        st0 = a.anchor_t[a0];
        sq0 = a.anchor_q[a0];
        tend = a.anchor_t[a1 - 1] + a.anchor_len[a1 - 1];
        qend = a.anchor_q[a1 - 1] + a.anchor_len[a1 - 1];
    }
    const int status = !ok ? ST_BAD_ARG
                           : (tl > BANDED_MAX_LEN || ql > BANDED_MAX_LEN || !chain_sum_ok(tl, ql, a1 - a0, a.match, a.mismatch, a.gopen, a.gext)) ? ST_UNSUPPORTED : 0;
    const bool live = status == 0;
    const int lt = live ? st0 : -1, lq = live ? sq0 : -1, rt = live ? tl - tend : -1, rq = live ? ql - qend : -1;
    const bool left = lt >= 1 && lq >= 1, right = rt >= 1 && rq >= 1;
    const int64_t ts = a.t_start[p], qs = a.q_start[p];
    if (lane == 0) {
        a.pstat[p] = status;
        a.flank[p] = make_int4(lt, lq, rt, rq);
        a.off[0][p] = p * a.tstride;
        a.off[1][p] = p * a.qstride;
        a.off[2][p] = right ? ts + tend : 0;
        a.off[3][p] = right ? qs + qend : 0;
        a.len[0][p] = left ? lt : 0;
        a.len[1][p] = left ? lq : 0;
        a.len[2][p] = right ? rt : 0;
        a.len[3][p] = right ? rq : 0;
    }
    if (!left) return; // (a live pair is within BANDED_MAX_LEN: its flanks fit their staging rows)
    const uint8_t *const tsrc = a.targets + ts, *const qsrc = a.queries + qs;
    uint8_t *const tdst = a.rev_t + p * a.tstride, *const qdst = a.rev_q + p * a.qstride;
    for (int k = lane; k < lt; k += 64) tdst[k] = tsrc[lt - 1 - k];
    for (int k = lane; k < lq; k += 64) qdst[k] = qsrc[lq - 1 - k];
}

__global__ __launch_bounds__(64) void sw_gap_fill_kernel(const ChainArgs a)
{
    const int lane = threadIdx.x;
    const int o = a.gopen, e = a.gext;
    unsigned char *const slot = a.ws + (int64_t)blockIdx.x * a.slot_bytes;

    for (int64_t g = blockIdx.x; g < a.total_anchors; g += a.slots) {
        const int p = a.owner[g];
        if (p == CHAIN_NO_OWNER) continue;
        if (a.pstat[p] != 0 || g + 1 >= a.anchor_start[p + 1]) continue;
        const int st = a.anchor_t[g], sq = a.anchor_q[g], sl = a.anchor_len[g];
        const int tl = a.anchor_t[g + 1] - st - sl, ql = a.anchor_q[g + 1] - sq - sl; // the gap's lengths gt, gq
        if (tl < 1 || ql < 1) continue;
        auto finish = [&](const int status, const int score, const int cigar_len) {
            if (lane != 0) return;
            a.gstatus[g] = status;
            a.gscore[g] = score;
            a.gclen[g] = cigar_len;
        };
        if (tl > a.max_gap_tl || ql > a.max_gap_ql || !banded_range_ok(tl, ql, a.match, a.mismatch, o, e) ||
            banded_pair_bytes(tl, ql, a.band, a.score_only != 0) > a.slot_bytes) {
            finish(ST_UNSUPPORTED, 0, 0);
            continue;
        }
        __threadfence_block(); // (the slot's last gap is done with it)
        __builtin_amdgcn_wave_barrier();
        const int lo = banded_lo(tl, ql, a.band), hi = banded_hi(tl, ql, a.band);
        int2 *const carry = reinterpret_cast<int2 *>(slot);
        uint32_t *const elems = reinterpret_cast<uint32_t *>(slot + banded_carry_bytes(ql));
        uint32_t *const dir = reinterpret_cast<uint32_t *>(slot + banded_carry_bytes(ql) + banded_elem_bytes(tl, ql));
        const int64_t strip_words = (int64_t)banded_strip_steps(tl, ql, a.band) * 8;
        const unsigned char *const tt = a.targets + a.t_start[p] + st + sl, *const tq = a.queries + a.q_start[p] + sq + sl;

        // row 0: the border's H and the E that enters row 1, minus infinity beyond the band
        for (int j = lane; j <= ql; j += 64) {
            const int b = border(j, o, e, true);
            carry[j] = j <= hi ? make_int2(b, b - o) : make_int2(NEG, NEG);
        }
        __threadfence_block();
        __builtin_amdgcn_wave_barrier();

        int h_last = NEG;
        const int strips = (tl + 63) / 64;
        for (int k = 0; k < strips; ++k) {
            Swept sw;
            const Strip s = strip_setup(k, lane, tl, ql, lo, hi, o, e, true, tt, tq, carry, dir + (int64_t)k * strip_words);
            sweep_strip<false>(s, lane, a.match, a.mismatch, o, e, !a.score_only, sw);
            h_last = sw.h_last;
            __threadfence_block(); // the carry row before the next strip reads it, the decisions before the walk does
            __builtin_amdgcn_wave_barrier();
        }
        // H(gt, gq): row gt reaches column gq (gt + hi >= gq), in the last strip
        const int corner = __shfl(h_last, (tl - 1) & 63);
        if (a.score_only) {
            finish(0, corner, 0);
            continue;
        }

        // ---- the walk from (gt, gq) back to row 0 or column 0, which one closing run then leaves for (0, 0)
        const Dirs dv{dir, lo, hi, strip_words};
        Elems el{elems, lane, 1, 0, 0};
        const Walked w = walk(dv, lane, tl, ql, 0, el);
        el.push(w.state, w.seg);
        if (w.I > 0) el.push(OP_D, w.I);
        else if (w.J > 0) el.push(OP_I, w.J);
        if (el.size > a.gstride) {
            finish(ST_CIGAR_OVERFLOW, 0, 0);
            continue;
        }
        el.write<false>(reinterpret_cast<char *>(a.grow + g * (a.gstride / 4)));
        finish(0, corner, el.size);
    }
}

__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

// the score of a gap with an empty side: one run of g = gt + gq bases, or nothing
__device__ __forceinline__ int run_score(const int g, const int o, const int e) { return g > 0 ? -o - (g - 1) * e : 0; }

// element v ends at byte `end` of the row `out`
__device__ __forceinline__ void put_element(char *const out, const int64_t end, const uint32_t v, const bool binary, const bool words)
{
    if (binary && words) {
        *reinterpret_cast<uint32_t *>(out + end - 4) = v;
    } else if (binary) { // a row that does not start on a multiple of four: byte by byte, little endian
        out[end - 4] = (char)(v & 0xff);
        out[end - 3] = (char)((v >> 8) & 0xff);
        out[end - 2] = (char)((v >> 16) & 0xff);
        out[end - 1] = (char)(v >> 24);
    } else {
        const unsigned op = v & 15u;
        int64_t pos = end;
        out[--pos] = op == OP_M ? 'M' : op == OP_I ? 'I' : 'D';
        for (int x = (int)(v >> 4); x > 0; x /= 10) out[--pos] = (char)('0' + x % 10);
    }
}

// one pass over a pair's joined CIGAR: `at` bytes so far, `carry` the running M that is not written yet.  Every lane calls every member
template <bool WRITE>
struct Joiner {
    char *out;
    int lane;
    bool binary, words;
    int64_t at;
    int carry;
    __device__ __forceinline__ void one(const uint32_t v)
    {
        const int w = binary ? 4 : digits((int)(v >> 4)) + 1;
        if (WRITE && lane == 0) put_element(out, at + w, v, binary, words);
        at += w;
    }
    __device__ __forceinline__ void flush()
    {
        if (carry > 0) one((uint32_t)carry << 4 | OP_M);
        carry = 0;
    }
    // a segment of n >= 1 elements in a binary row, read back to front where `rev`; first, last: its first and last element in the
    // order they are read
    __device__ __forceinline__ void segment(const uint32_t *const row, const int n, const bool rev, const uint32_t first, const uint32_t last)
    {
        int from = 0, to = n;
        if ((first & 15u) == OP_M) {
            carry += (int)(first >> 4);
            from = 1;
        }
        if (from >= to) return; // one M: all of it in the running M
        flush();
        int tail = 0;
        if ((last & 15u) == OP_M) {
            tail = (int)(last >> 4);
            to = n - 1;
        }
        for (int base = from; base < to; base += 64) {
            if (!WRITE && binary) {
                at += 4 * min(64, to - base);
                continue;
            }
            const int m = base + lane;
            const bool in = m < to;
            const uint32_t v = in ? row[rev ? n - 1 - m : m] : 0;
            const int w = in ? (binary ? 4 : digits((int)(v >> 4)) + 1) : 0;
            int incl = w;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int up = __shfl_up(incl, d);
                if (lane >= d) incl += up;
            }
            if (WRITE && in) put_element(out, at + incl, v, binary, words);
            at += __shfl(incl, 63);
        }
        carry = tail;
    }
};

// the joined CIGAR of pair p, anchors a0 .. a1 - 1: the left side's nl elements back to front, anchor, gap, anchor, ..., the right
// side's nr elements; -> its bytes
template <bool WRITE>
__device__ __forceinline__ int64_t chain_cigar(const ChainArgs &a, const int lane, const int64_t a0, const int64_t a1, const uint32_t *const lrow, const int nl,
                                               const uint32_t *const rrow, const int nr, char *const out)
{
    Joiner<WRITE> j{out, lane, a.binary_cigar != 0, (reinterpret_cast<uintptr_t>(out) & 3) == 0, 0, 0};
    const int64_t gwords = a.gstride / 4;
    if (nl > 0) j.segment(lrow, nl, true, lrow[nl - 1], lrow[0]);
    for (int64_t base = a0; base < a1; base += 64) {
        const int64_t i = base + lane;
        const bool valid = i < a1, next = i + 1 < a1;
        const int st = valid ? a.anchor_t[i] : 0, sq = valid ? a.anchor_q[i] : 0, sl = valid ? a.anchor_len[i] : 0;
        const int gt = next ? a.anchor_t[i + 1] - st - sl : 0, gq = next ? a.anchor_q[i + 1] - sq - sl : 0;
        const int gn = gt > 0 && gq > 0 ? a.gclen[i] / 4 : 0;
        const uint32_t gf = gn > 0 ? a.grow[i * gwords] : 0, gl = gn > 0 ? a.grow[i * gwords + gn - 1] : 0;
        const int cnt = (int)min((int64_t)64, a1 - base);
        for (int x = 0; x < cnt; ++x) {
            j.carry += __builtin_amdgcn_readlane(sl, x);
            const int gtx = __builtin_amdgcn_readlane(gt, x), gqx = __builtin_amdgcn_readlane(gq, x), gnx = __builtin_amdgcn_readlane(gn, x);
            if (gnx > 0) {
                j.segment(a.grow + (base + x) * gwords, gnx, false, (uint32_t)__builtin_amdgcn_readlane((int)gf, x), (uint32_t)__builtin_amdgcn_readlane((int)gl, x));
            } else if (gqx > 0) {
                j.flush();
                j.one((uint32_t)gqx << 4 | OP_I);
            } else if (gtx > 0) {
                j.flush();
                j.one((uint32_t)gtx << 4 | OP_D);
            }
        }
    }
    if (nr > 0) j.segment(rrow, nr, false, rrow[0], rrow[nr - 1]);
    j.flush();
    return j.at;
}

__global__ __launch_bounds__(64) void sw_chain_join_kernel(const ChainArgs a)
{
    const int lane = threadIdx.x;
    const Extension zero{0, 0, 0, 0, 0, 0, 0, 0};
    const int64_t p = blockIdx.x;
    auto finish = [&](const int status, const ChainAlignment &r, const Extension &l, const Extension &rr, const int cigar_len) {
        if (lane != 0) return;
        a.aln[p] = r;
        if (a.left_out) a.left_out[p] = l;
        if (a.right_out) a.right_out[p] = rr;
        if (a.status) a.status[p] = status;
        if (a.cigar_len) a.cigar_len[p] = cigar_len;
    };
    auto fail = [&](const int status) { finish(status, ChainAlignment{0, 0, 0, 0, 0, 0, 0, 0}, zero, zero, 0); };
    const int ps = a.pstat[p];
    if (ps) {
        fail(ps);
        return;
    }
    const int64_t a0 = a.anchor_start[p], a1 = a.anchor_start[p + 1];
    const int o = a.gopen, e = a.gext;
    const int64_t ts = a.t_start[p], qs = a.q_start[p];

    // ---- the anchors: whose they are, their scores, and the gaps behind them
    int same = 0, cols = 0, gsum = 0;
    bool stolen = false, unsup = false, over = false;
    for (int64_t base = a0; base < a1; base += 64) {
        const int64_t i = base + lane;
        const bool valid = i < a1, next = i + 1 < a1;
        stolen |= valid && a.owner[i] != (int)p;
        const int st = valid ? a.anchor_t[i] : 0, sq = valid ? a.anchor_q[i] : 0, sl = valid ? a.anchor_len[i] : 0;
        const int gt = next ? a.anchor_t[i + 1] - st - sl : 0, gq = next ? a.anchor_q[i + 1] - sq - sl : 0;
        const bool real = gt > 0 && gq > 0;
        const int gs = real ? a.gstatus[i] : 0;
        unsup |= gs == ST_UNSUPPORTED;
        over |= gs != 0;
        gsum += real ? (gs ? 0 : a.gscore[i]) : run_score(gt + gq, o, e);
        cols += sl;
        const int cnt = (int)min((int64_t)64, a1 - base);
        for (int x = 0; x < cnt; ++x) {
            const uint8_t *const ta = a.targets + ts + __builtin_amdgcn_readlane(st, x), *const qa = a.queries + qs + __builtin_amdgcn_readlane(sq, x);
            const int slx = __builtin_amdgcn_readlane(sl, x);
            for (int c = lane; c < slx; c += 64) same += ta[c] == qa[c];
        }
    }
    // (a range another pair claimed first: its gaps may be that pair's.  Refused before anything of them is used)
    if (__ballot(stolen)) {
        fail(ST_BAD_ARG);
        return;
    }
    const int4 f = a.flank[p];
    const bool la = f.x >= 1 && f.y >= 1, ra = f.z >= 1 && f.w >= 1;
    const int ls = la ? a.side_status[0][p] : 0, rs = ra ? a.side_status[1][p] : 0;
    if (ls == ST_UNSUPPORTED || rs == ST_UNSUPPORTED || __ballot(unsup)) {
        fail(ST_UNSUPPORTED);
        return;
    }
    if (ls || rs || __ballot(over)) { // an internal row is too small: so is the caller's (sw_chain.h, sw_seed_extend.h)
        fail(ST_CIGAR_OVERFLOW);
        return;
    }
    same = wave_sum(same);
    cols = wave_sum(cols);
    gsum = wave_sum(gsum);
    const int anchor_score = same * a.match + (cols - same) * a.mismatch;

    // ---- the sides, as sw_seed_join_kernel reads them: one that never reached the extension kernel has an empty query flank (the
    // empty extension ends on column ql = 0) or an empty target flank alone (no row reaches column ql)
    Extension L = zero, R = zero;
    if (la) L = a.side_ext[0][p];
    if (ra) R = a.side_ext[1][p];
    L.score_qend = !la && f.y != 0 ? EXTEND_NO_QEND : L.score_qend;
    L.t_end_qend = !la && f.y != 0 ? -1 : L.t_end_qend;
    R.score_qend = !ra && f.w != 0 ? EXTEND_NO_QEND : R.score_qend;
    R.t_end_qend = !ra && f.w != 0 ? -1 : R.t_end_qend;

    // ---- the record: a side contributes the H of the cell its walk starts from
    const int li = L.cigar_from ? L.t_end_qend : L.t_end, lj = L.cigar_from ? f.y : L.q_end, lh = L.cigar_from ? L.score_qend : L.score;
    const int ri = R.cigar_from ? R.t_end_qend : R.t_end, rj = R.cigar_from ? f.w : R.q_end, rh = R.cigar_from ? R.score_qend : R.score;
    const int tl = a.t_len[p], ql = a.q_len[p];
    const ChainAlignment r{lh + anchor_score + gsum + rh, f.x - li, tl - f.z + ri, f.y - lj, ql - f.w + rj, anchor_score, L.dropped | R.dropped << 1, L.cigar_from | R.cigar_from << 1};

    int size = 0;
    if (!a.score_only) {
        const uint32_t *const lrow = a.side_cigar[0] + p * (a.istride / 4), *const rrow = a.side_cigar[1] + p * (a.istride / 4);
        const int nl = la ? a.side_clen[0][p] / 4 : 0, nr = ra ? a.side_clen[1][p] / 4 : 0;
        char *const out = a.cigar + p * (int64_t)a.cigar_stride;
        const int64_t bytes = chain_cigar<false>(a, lane, a0, a1, lrow, nl, rrow, nr, out);
        if (bytes > (a.binary_cigar ? a.cigar_stride & ~3 : a.cigar_stride)) {
            fail(ST_CIGAR_OVERFLOW);
            return;
        }
        chain_cigar<true>(a, lane, a0, a1, lrow, nl, rrow, nr, out);
        size = (int)bytes;
    }
    if (a.gap_score_out) {
        for (int64_t i = a0 + lane; i + 1 < a1; i += 64) {
            const int st = a.anchor_t[i], sq = a.anchor_q[i], sl = a.anchor_len[i];
            const int gt = a.anchor_t[i + 1] - st - sl, gq = a.anchor_q[i + 1] - sq - sl;
            a.gap_score_out[i] = gt > 0 && gq > 0 ? a.gscore[i] : run_score(gt + gq, o, e);
        }
    }
    finish(0, r, L, R, size);
}

} // namespace

hipError_t launch_chain_split(const ChainArgs &a, hipStream_t stream)
{
    if (a.n < 1) return hipSuccess;
    if (a.n > SEED_MAX_CHUNK) return hipErrorInvalidValue;
    if (!a.rev_t || !a.rev_q || !a.flank || !a.pstat || !a.owner || !a.anchor_start) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_chain_split_kernel, dim3((unsigned)a.n), dim3(64), 0, stream, a);
    return hipGetLastError();
}

// gaps 0 .. total_anchors - 1 on a.slots waves, wave w in workspace slot w
hipError_t launch_gap_fill(const ChainArgs &a, hipStream_t stream)
{
    if (a.n < 1 || a.total_anchors < 1) return hipSuccess;
    if (!a.ws || a.slots < 1 || a.slot_bytes < 256 || !a.owner || !a.pstat || !a.gscore || !a.gstatus || !a.gclen || (!a.score_only && (!a.grow || a.gstride < 4)))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_gap_fill_kernel, dim3((unsigned)a.slots), dim3(64), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_chain_join(const ChainArgs &a, hipStream_t stream)
{
    if (a.n < 1) return hipSuccess;
    if (a.n > SEED_MAX_CHUNK) return hipErrorInvalidValue;
    if (!a.aln || !a.flank || !a.pstat || !a.owner || (!a.score_only && (!a.cigar || !a.cigar_len || !a.side_cigar[0] || !a.side_cigar[1] || a.istride < 4 || !a.grow)))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_chain_join_kernel, dim3((unsigned)a.n), dim3(64), 0, stream, a);
    return hipGetLastError();
}

} // namespace mgl_sw_dev
