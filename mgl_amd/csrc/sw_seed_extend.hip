// sw_seed_extend.hip -- the two kernels that mgl_sw_extend_seed_batch_device puts around the extension kernels (the
// function is tests/seed_extend_textbook.py's): sw_seed_split_kernel in front of them, sw_seed_join_kernel behind.  One wave per pair
// in both, pair blockIdx.x: with a loop over pairs the join kept more scalars alive across it than there are registers for.
// sw_seed_extend.h describes the staging they share with the host side.
//
// The split validates the seed, writes the four flank descriptors and copies the two left flanks reversed into the staging rows, 64
// bytes per wave and step: lane l of step s stores byte 64 s + l of the copy, which is byte len - 1 - 64 s - l of the flank, so both
// the loads and the stores of a step are 64 consecutive bytes.  The right flanks stay where they are.
//
// The join adds the seed's score up (64 columns a step, one wave reduction), combines the two side records, and writes the joined
// CIGAR: the left side's binary row back to front, the seed, the right side's front to back.  Only the seed's two neighbours can merge
// with it -- each side's FIRST element, the one at its anchor --, so the joined elements are a function of their index and the wave
// formats 64 of them a step, a prefix sum of their widths placing each lane's text (as Elems::write of sw_band_wave.h does for one
// side; that header is included for the operations, the statuses and digits()).
#include "sw_band_wave.h"
#include "sw_seed_extend.h"

namespace mgl_sw_dev {

namespace {

__global__ __launch_bounds__(64) void sw_seed_split_kernel(const SeedArgs a)
{
    const int lane = threadIdx.x;
    const int64_t p = blockIdx.x;
    const int tl = a.t_len[p], ql = a.q_len[p], st = a.seed_t[p], sq = a.seed_q[p], sl = a.seed_len[p];
    const bool ok = tl >= 1 && ql >= 1 && tl <= a.max_tl && ql <= a.max_ql && sl >= 1 && st >= 0 && sq >= 0 && (int64_t)st + sl <= tl &&
                    (int64_t)sq + sl <= ql;
    const int lt = ok ? st : -1, lq = ok ? sq : -1, rt = ok ? tl - st - sl : -1, rq = ok ? ql - sq - sl : -1;
    const bool left = lt >= 1 && lq >= 1, right = rt >= 1 && rq >= 1;
    const int64_t ts = a.t_start[p], qs = a.q_start[p];
    if (lane == 0) {
        a.flank[p] = make_int4(lt, lq, rt, rq);
        a.off[0][p] = p * a.tstride;
        a.off[1][p] = p * a.qstride;
        a.off[2][p] = right ? ts + st + sl : 0;
        a.off[3][p] = right ? qs + sq + sl : 0;
        a.len[0][p] = left ? lt : 0;
        a.len[1][p] = left ? lq : 0;
        a.len[2][p] = right ? rt : 0;
        a.len[3][p] = right ? rq : 0;
    }
    // a flank beyond BANDED_MAX_LEN is longer than a staging row: it is not copied, and the extension kernel, whose range guard
    // refuses it, never reads the row
    if (!left || lt > BANDED_MAX_LEN || lq > BANDED_MAX_LEN) return;
    const uint8_t *const tsrc = a.targets + ts, *const qsrc = a.queries + qs;
    uint8_t *const tdst = a.rev_t + p * a.tstride, *const qdst = a.rev_q + p * a.qstride;
    for (int k = lane; k < lt; k += 64) tdst[k] = tsrc[lt - 1 - k];
    for (int k = lane; k < lq; k += 64) qdst[k] = qsrc[lq - 1 - k];
}

__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

__global__ __launch_bounds__(64) void sw_seed_join_kernel(const SeedArgs a)
{
    const int lane = threadIdx.x;
    const Extension zero{0, 0, 0, 0, 0, 0, 0, 0};
    const int64_t p = blockIdx.x;
    const int4 f = a.flank[p];
    auto finish = [&](const int status, const SeedAlignment &r, const Extension &l, const Extension &rr, const int cigar_len) {
        if (lane != 0) return;
        a.aln[p] = r;
        if (a.left_out) a.left_out[p] = l;
        if (a.right_out) a.right_out[p] = rr;
        if (a.status) a.status[p] = status;
        if (a.cigar_len) a.cigar_len[p] = cigar_len;
    };
    auto fail = [&](const int status) { finish(status, SeedAlignment{0, 0, 0, 0, 0, 0, 0, 0}, zero, zero, 0); };
    if (f.x < 0) {
        fail(ST_BAD_ARG);
        return;
    }
    const int st = a.seed_t[p], sq = a.seed_q[p], sl = a.seed_len[p];
    const bool la = f.x >= 1 && f.y >= 1, ra = f.z >= 1 && f.w >= 1;
    const int ls = la ? a.side_status[0][p] : 0, rs = ra ? a.side_status[1][p] : 0;
    // the seed's own guard: its score and the merged element stay in range as a side's do
    const int64_t s = a.match > -a.mismatch ? a.match : -(int64_t)a.mismatch;
    if (ls == ST_UNSUPPORTED || rs == ST_UNSUPPORTED || f.x + sl + f.z > BANDED_MAX_LEN || f.y + sl + f.w > BANDED_MAX_LEN || s * sl > BANDED_MAX_SCORE) {
        fail(ST_UNSUPPORTED);
        return;
    }
    if (ls || rs) { // a side's row is too small: so is the caller's (sw_seed_extend.h)
        fail(ls ? ls : rs);
        return;
    }
    // a side that never reached the extension kernel: the query flank is empty (nothing left to extend: the empty extension ends
    // on column ql = 0), or the target flank alone (no row reaches column ql)
    Extension L = zero, R = zero;
    if (la) L = a.side_ext[0][p];
    if (ra) R = a.side_ext[1][p];
    L.score_qend = !la && f.y != 0 ? EXTEND_NO_QEND : L.score_qend;
    L.t_end_qend = !la && f.y != 0 ? -1 : L.t_end_qend;
    R.score_qend = !ra && f.w != 0 ? EXTEND_NO_QEND : R.score_qend;
    R.t_end_qend = !ra && f.w != 0 ? -1 : R.t_end_qend;

    // ---- the seed's score
    const uint8_t *const tseed = a.targets + a.t_start[p] + st, *const qseed = a.queries + a.q_start[p] + sq;
    int same = 0;
    for (int k = lane; k < sl; k += 64) same += tseed[k] == qseed[k];
    same = wave_sum(same);
    const int seed_score = same * a.match + (sl - same) * a.mismatch;

    // ---- the records: a side contributes the H of the cell its walk starts from
    const int li = L.cigar_from ? L.t_end_qend : L.t_end, lj = L.cigar_from ? f.y : L.q_end, lh = L.cigar_from ? L.score_qend : L.score;
    const int ri = R.cigar_from ? R.t_end_qend : R.t_end, rj = R.cigar_from ? f.w : R.q_end, rh = R.cigar_from ? R.score_qend : R.score;
    const SeedAlignment r{lh + seed_score + rh, st - li, st + sl + ri, sq - lj, sq + sl + rj, seed_score, L.dropped | R.dropped << 1, L.cigar_from | R.cigar_from << 1};
    if (a.score_only) {
        finish(0, r, L, R, 0);
        return;
    }

    // ---- the joined elements, by index: the left row back to front without its first element where that is an M, the seed with
    // what merged into it, the right row front to back likewise
    const uint32_t *const lrow = a.side_cigar[0] + p * (a.istride / 4), *const rrow = a.side_cigar[1] + p * (a.istride / 4);
    const int nl = la ? a.side_clen[0][p] / 4 : 0, nr = ra ? a.side_clen[1][p] / 4 : 0;
    const uint32_t l0 = nl ? lrow[0] : OP_I, r0 = nr ? rrow[0] : OP_I;
    const bool lm = (l0 & 15u) == OP_M, rm = (r0 & 15u) == OP_M;
    const uint32_t seed_el = (uint32_t)(sl + (lm ? (int)(l0 >> 4) : 0) + (rm ? (int)(r0 >> 4) : 0)) << 4 | OP_M;
    const int nlk = nl - (lm ? 1 : 0), nrk = nr - (rm ? 1 : 0), ne = nlk + 1 + nrk;
    auto element = [&](const int m) { return m < nlk ? lrow[nl - 1 - m] : m == nlk ? seed_el : rrow[m - nlk - 1 + (rm ? 1 : 0)]; };
    int size = 4 * ne;
    if (!a.binary_cigar) {
        int w = 0;
        for (int m = lane; m < ne; m += 64) w += digits((int)(element(m) >> 4)) + 1;
        size = wave_sum(w);
    }
    const int cap = a.binary_cigar ? a.cigar_stride & ~3 : a.cigar_stride;
    if (size > cap) {
        fail(ST_CIGAR_OVERFLOW);
        return;
    }
    char *const out = a.cigar + p * (int64_t)a.cigar_stride;
    const bool words = (reinterpret_cast<uintptr_t>(out) & 3) == 0;
    for (int base = 0, at = 0; base < ne; base += 64) {
        const int m = base + lane;
        const uint32_t v = m < ne ? element(m) : 0;
        const int len = (int)(v >> 4);
        const int w = m < ne ? (a.binary_cigar ? 4 : digits(len) + 1) : 0;
        int incl = w;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        int pos = at + incl;
        if (m < ne) {
            if (a.binary_cigar && words) {
                *reinterpret_cast<uint32_t *>(out + pos - 4) = v;
            } else if (a.binary_cigar) { // a row that does not start on a multiple of four: byte by byte, little endian
                out[pos - 4] = (char)(v & 0xff);
                out[pos - 3] = (char)((v >> 8) & 0xff);
                out[pos - 2] = (char)((v >> 16) & 0xff);
                out[pos - 1] = (char)(v >> 24);
            } else {
                const unsigned op = v & 15u;
                out[--pos] = op == OP_M ? 'M' : op == OP_I ? 'I' : 'D';
                for (int x = len; x > 0; x /= 10) out[--pos] = (char)('0' + x % 10);
            }
        }
        at += __shfl(incl, 63);
    }
    finish(0, r, L, R, size);
}

} // namespace

hipError_t launch_seed_split(const SeedArgs &a, hipStream_t stream)
{
    if (a.n < 1) return hipSuccess;
    if (a.n > SEED_MAX_CHUNK) return hipErrorInvalidValue;
    if (!a.rev_t || !a.rev_q || !a.flank) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_seed_split_kernel, dim3((unsigned)a.n), dim3(64), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_seed_join(const SeedArgs &a, hipStream_t stream)
{
    if (a.n < 1) return hipSuccess;
    if (a.n > SEED_MAX_CHUNK) return hipErrorInvalidValue;
    if (!a.aln || !a.flank || (!a.score_only && (!a.cigar || !a.cigar_len || !a.side_cigar[0] || !a.side_cigar[1] || a.istride < 4))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_seed_join_kernel, dim3((unsigned)a.n), dim3(64), 0, stream, a);
    return hipGetLastError();
}

} // namespace mgl_sw_dev
