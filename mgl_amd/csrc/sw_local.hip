// sw_local.hip -- kernel B of mgl_sw_local_batch_device_matrix: local (zero-floor) Smith-Waterman of any pair in int32, with the score,
// both ends, the begin and the CIGAR (the function is tests/local_textbook.py's, which the tests compare with).
//
// One wave per pair.  The 64 lanes hold 64 consecutive target rows (a strip) and sweep the query's columns on an anti-diagonal: at step
// s lane l is at column j = s - l + 1, so H and E of the cell above come from lane l - 1's previous step (one lane shift) and the
// diagonal from the step before that.  Lane 0 takes the row above the strip from a carry row in the pair's workspace slot, which lane 63
// writes for the next strip.  Every cell leaves one decision byte (bits 0-1: where H came from, 0 = the zero floor / 1 = diagonal /
// 2 = F / 3 = E, in that priority; bit 2: F extends; bit 3: E extends), stored by anti-diagonal step so that a step's 64 bytes are
// one line: [strip][step][lane].  The end is the smallest (i, j) holding the maximum (each lane keeps its first, a butterfly
// reduction picks the smallest row), and lane 0 walks the bytes twice: once to size the CIGAR, once to write it back to front.
//
// Batches are cut into chunks of workspace slots by the host (sw_local.cpp); a pair whose cells do not fit a slot gets
// MGL_SW_ERR_UNSUPPORTED.  MGL_SW_FLAG_SCORE_ONLY keeps no decisions and walks nothing (kernel A's batches that are outside its guard).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sw_local.h"

namespace mgl_sw_dev {

namespace {

constexpr int ST_BAD_ARG = 1, ST_CIGAR_OVERFLOW = 2, ST_UNSUPPORTED = 5; // mgl_sw_status

__device__ __forceinline__ int digits(int v)
{
    int d = 1;
    while (v >= 10) {
        v /= 10;
        ++d;
    }
    return d;
}

// lane 0: the walk from (i, j) in state H; emit(op, run) is called once per run, last run first (ops 0 = M, 1 = I, 2 = D).  Returns
// the cell it stopped in.
template <class Emit>
__device__ __forceinline__ void local_walk(const unsigned char *dir, const int ql, int &i, int &j, Emit emit)
{
    const int64_t strip_bytes = (int64_t)(ql + 63) * 64;
    auto at = [&](const int ii, const int jj) {
        const int r = ii - 1;
        return dir[(int64_t)(r >> 6) * strip_bytes + (int64_t)(jj - 1 + (r & 63)) * 64 + (r & 63)];
    };
    int state = 0, op = -1, run = 0;
    auto put = [&](const int o) {
        if (o == op) {
            ++run;
            return;
        }
        if (run) emit(op, run);
        op = o;
        run = 1;
    };
    for (;;) {
        if (state == 0) {
            if (i == 0 || j == 0) break;
            const unsigned d = at(i, j);
            const unsigned src = d & 3u;
            if (src == 0) break;
            if (src == 1) {
                put(0);
                --i;
                --j;
            } else {
                state = src == 2 ? 1 : 2;
            }
        } else if (state == 1) {
            const unsigned d = at(i, j);
            put(1);
            --j;
            state = (d & 4u) ? 1 : 0;
        } else {
            const unsigned d = at(i, j);
            put(2);
            --i;
            state = (d & 8u) ? 2 : 0;
        }
    }
    if (run) emit(op, run);
}

__global__ __launch_bounds__(64) void sw_local_pair_kernel(const LocalArgs a)
{
    __shared__ unsigned char code_s[256];
    __shared__ signed char mat_s[MATRIX_DIM * MATRIX_DIM];
    const int lane = threadIdx.x;
    reinterpret_cast<unsigned *>(code_s)[lane] = reinterpret_cast<const unsigned *>(a.code)[lane];
#pragma unroll
    for (int x = 0; x < MATRIX_DIM * MATRIX_DIM / 256; ++x)
        reinterpret_cast<unsigned *>(mat_s)[x * 64 + lane] = reinterpret_cast<const unsigned *>(a.matrix)[x * 64 + lane];
    __syncthreads();

    const int64_t p = a.first + blockIdx.x;
    const int tl = a.t.len[p], ql = a.q.len[p];
    const int64_t ts = a.t.off[p], qs = a.q.off[p];
    LocalHit hit{0, 0, 0, 0, 0};
    auto finish = [&](const int status, const int cigar_len) {
        if (lane != 0) return;
        a.hit[p] = hit;
        if (a.status) a.status[p] = status;
        if (a.cigar_len) a.cigar_len[p] = cigar_len;
    };
    if (tl < 0 || ql < 0 || tl > a.max_tl || ql > a.max_ql) return finish(ST_BAD_ARG, 0);
    if (tl == 0 || ql == 0) return finish(0, 0); // a hole
    if (local_pair_bytes(tl, ql, a.score_only) > a.slot_bytes || (int64_t)(a.smax > 0 ? a.smax : 0) * (tl < ql ? tl : ql) >= (1 << 29))
        return finish(ST_UNSUPPORTED, 0);

    const int o = a.gopen, e = a.gext;
    int2 *const carry = reinterpret_cast<int2 *>(a.ws + (int64_t)blockIdx.x * a.slot_bytes);
    unsigned char *const dir = reinterpret_cast<unsigned char *>(carry) + (int64_t)(ql + 1) * 8;
    for (int j = lane; j <= ql; j += 64) carry[j] = make_int2(0, NEG_INF);
    __threadfence_block();

    int best = 0, bi = 0, bj = 0;
    const int strips = (tl + 63) / 64, steps = ql + 63;
    const unsigned char *const tq = a.q.data + qs;
    for (int s = 0; s < strips; ++s) {
        const int i = s * 64 + lane + 1;
        const bool rowv = i <= tl;
        const signed char *const mrow = mat_s + (rowv ? code_s[a.t.data[ts + i - 1]] : 0) * MATRIX_DIM;
        unsigned char *const dstrip = dir + (int64_t)s * steps * 64 + lane;
        int hleft = 0, f = NEG_INF, prev_up = 0, out_h = 0, out_e = NEG_INF;
        for (int step = 0; step < steps; ++step) {
            const int j = step - lane + 1;
            int up_h = __shfl_up(out_h, 1), up_e = __shfl_up(out_e, 1);
            if (lane == 0 && j <= ql) {
                const int2 c = carry[j];
                up_h = c.x;
                up_e = c.y;
            }
            if (j >= 1 && j <= ql) {
                const int sc = mrow[code_s[tq[j - 1]]];
                const int diag = prev_up + sc;
                const int ev = max(up_h - o, up_e - e);
                const int fv = max(hleft - o, f - e);
                const int h = max(max(0, diag), max(ev, fv));
                if (!a.score_only && rowv) {
                    const unsigned src = h == 0 ? 0u : h == diag ? 1u : h == fv ? 2u : 3u;
                    const unsigned fx = (f - e >= hleft - o) ? 4u : 0u, ex = (up_e - e >= up_h - o) ? 8u : 0u;
                    dstrip[(int64_t)step * 64] = (unsigned char)(src | fx | ex);
                }
                if (rowv && h > best) {
                    best = h;
                    bi = i;
                    bj = j;
                }
                hleft = h;
                f = fv;
                out_h = h;
                out_e = ev;
                if (lane == 63 && s + 1 < strips) carry[j] = make_int2(h, ev);
            } else if (j < 1) {
                out_h = 0;
                out_e = NEG_INF;
            }
            prev_up = up_h;
        }
        __threadfence_block(); // lane 63's carry row before lane 0 of the next strip reads it
        __builtin_amdgcn_wave_barrier();
    }
    // the smallest (i, j) that holds the maximum: score descending, then row, then column
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const int ob = __shfl_xor(best, m), oi = __shfl_xor(bi, m), oj = __shfl_xor(bj, m);
        const bool take = ob > best || (ob == best && (oi < bi || (oi == bi && oj < bj)));
        best = take ? ob : best;
        bi = take ? oi : bi;
        bj = take ? oj : bj;
    }
    if (best <= 0) return finish(0, 0);
    hit.score = best;
    if (a.score_only) return finish(0, 0);
    if (lane != 0) return;
    __threadfence_block();
    // pass 1: the CIGAR's size; pass 2: write it back to front
    int i0 = bi, j0 = bj, size = 0;
    local_walk(dir, ql, i0, j0, [&](int, int run) { size += a.binary_cigar ? 4 : digits(run) + 1; });
    hit.t_begin = i0;
    hit.t_end = bi;
    hit.q_begin = j0;
    hit.q_end = bj;
    if (size > a.cigar_stride) return finish(ST_CIGAR_OVERFLOW, size);
    char *const out = a.cigar + p * (int64_t)a.cigar_stride;
    int pos = size, i1 = bi, j1 = bj;
    local_walk(dir, ql, i1, j1, [&](int op, int run) {
        if (a.binary_cigar) {
            pos -= 4;
            const uint32_t w = (uint32_t)run << 4 | (uint32_t)op;
            out[pos] = (char)(w & 0xff);
            out[pos + 1] = (char)((w >> 8) & 0xff);
            out[pos + 2] = (char)((w >> 16) & 0xff);
            out[pos + 3] = (char)(w >> 24);
        } else {
            out[--pos] = "MID"[op];
            for (int v = run; v > 0; v /= 10) out[--pos] = (char)('0' + v % 10);
        }
    });
    finish(0, size);
}

} // namespace

// pairs [a.first, a.first + a.count): one wave each, pair first + k in workspace slot k
hipError_t launch_local_pairs(const LocalArgs &a, hipStream_t stream)
{
    if (a.count < 1) return hipSuccess;
    if (!a.matrix || !a.code || !a.hit || !a.ws || a.slot_bytes < 256 || (!a.score_only && (!a.cigar || !a.cigar_len)) || a.count > 0x7fffffff)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_local_pair_kernel, dim3((unsigned)a.count), dim3(64), 0, stream, a);
    return hipGetLastError();
}

} // namespace mgl_sw_dev
