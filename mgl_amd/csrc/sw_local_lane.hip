// sw_local_lane.hip -- kernel A of mgl_sw_local_batch_device_matrix: the local (zero-floor) Smith-Waterman SCORE of tiles of 128 pairs
// that share their target (MGL_SW_FLAG_SHARED_TARGET + MGL_SW_FLAG_SCORE_ONLY): the score pass of a database search.  The mapping is
// sw_dp16_lane_matrix.hip's -- two pairs per lane in packed 16-bit halves, a strip of 32 target rows in registers, the query's columns
// swept one by one, the scores of a column one row of a strip profile the wave builds in LDS, a persistent grid that draws its tiles
// largest first off a self-resetting counter -- with the local recurrence:
//
//     E = max(H_up - o, E_up - e),  F = max(H_left - o, F_left - e),  H = max(0, H_diag + S, E, F),  score = max H.
//
// Every value is kept as an UNSIGNED 16-bit half floored at zero.  That changes nothing: H >= 0 anyway, and an E or F below zero never
// makes an H or, through e >= 0, a larger E or F than the floored value does.  The floor then costs nothing where a clamped subtract
// is needed anyway: the profile holds S + K (K = max(0, -min S), a byte) and the diagonal is v_pk_sub_u16 clamp (H_diag + S + K, K) =
// max(0, H_diag + S); the opens and extensions are clamped subtracts too.  No (i + j) e offset frame as in the GATK kernels: it cannot
// absorb the floor.  A step (one row of a column, two pairs) is 11 VALU instructions: the score's v_perm, the diagonal's add and
// clamped subtract, two maxima for H, one clamped subtract for the open, two each for E and F, one maximum into the running maximum.
//
// The running maximum is one register per lane (both pairs), with no masks: rows beyond the target's end (a strip the target ends
// inside) take a zero profile byte, columns beyond a pair's own query length take the GHOST code whose profile row is zero.  A cell
// whose score is -K <= 0 never exceeds the largest real cell (nor does anything it feeds, all of it lies below or right of the real
// matrix), so those cells cannot change the maximum.  So the wave sweeps to the tile's longest query, and a query shorter than that --
// or a hole, a pair of length 0 -- just rides along.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "sw_lane_cell.h"
#include "sw_local.h"

namespace mgl_sw_dev {

namespace {

constexpr int LA_R = LOCAL_LANE_R;
constexpr int LA_LDS_CODE = 0;
constexpr int LA_LDS_M = 256;
constexpr int LA_LDS_SP = LA_LDS_M + MATRIX_DIM * MATRIX_DIM;        // (MATRIX_DIM + 1) codes x LA_R rows
constexpr int LA_LDS_T = LA_LDS_SP + (MATRIX_DIM + 1) * LA_R;        // the target as codes (0xff beyond its end)
static_assert(LA_LDS_T % 16 == 0, "LDS carve alignment");

__device__ __forceinline__ unsigned pk_usub_sat(unsigned a, unsigned b)
{
    return __builtin_bit_cast(unsigned, __builtin_elementwise_sub_sat(as_us2(a), as_us2(b)));
}
__device__ __forceinline__ unsigned pk_umax(unsigned a, unsigned b)
{
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(as_us2(a), as_us2(b)));
}

// R rows of one column for both packed pairs.  h[r]: H of row r, column j - 1 on entry, column j on exit; f[r]: F of row r for column j
// on entry, for column j + 1 on exit; hdo: H of the row above the strip, column j - 1; e: E of the strip's first row (in), of the row
// below the strip (out); hlast: H of the strip's last row (out); mx: the running maximum.
template <int R>
__device__ __forceinline__ void local_column(unsigned (&h)[R], unsigned (&f)[R], const uint4 (&sa)[R / 16], const uint4 (&sb)[R / 16], const unsigned hdo,
                                             unsigned &e, unsigned &hlast, unsigned &mx, const unsigned kb, const unsigned go, const unsigned ge,
                                             const unsigned (&sel)[4])
{
    auto word = [&](const uint4 (&s)[R / 16], const int r) {
        const uint4 &v = s[r >> 4];
        const int k = (r >> 2) & 3;
        return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w;
    };
    auto score = [&](const int r) { return __builtin_amdgcn_perm(word(sb, r), word(sa, r), sel[r & 3]); };
    unsigned dg = pk_add(hdo, score(0));
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const unsigned diag = pk_usub_sat(dg, kb);
        if (r + 1 < R) dg = pk_add(h[r], score(r + 1)); // (before row r overwrites h[r]: the diagonal of row r + 1)
        const unsigned hn = pk_umax(pk_umax(diag, e), f[r]);
        const unsigned open = pk_usub_sat(hn, go);
        e = pk_umax(open, pk_usub_sat(e, ge));
        f[r] = pk_umax(open, pk_usub_sat(f[r], ge));
        mx = pk_umax(mx, hn);
        h[r] = hn;
        asm volatile("" : "+v"(f[r]), "+v"(h[r]));
    }
    hlast = h[R - 1];
}

__device__ __forceinline__ void local_strip(const int qmax, uint2 *bnd, const unsigned *qst, const unsigned char *sp, const unsigned kb, const unsigned go,
                                            const unsigned ge, const unsigned (&sel)[4], const bool last, unsigned &mx)
{
    constexpr int R = LA_R;
    unsigned h[R], f[R];
#pragma unroll
    for (int r = 0; r < R; ++r) h[r] = f[r] = 0u; // H[i][0] = 0; F[i][1] = max(0 - o, -inf), floored
    unsigned hdo = 0u;                              // H[i0][0]
    uint2 *bp = bnd + 64;                           // column j
    auto scores_of = [&](const unsigned codes_a, const unsigned codes_b, const int k, uint4 (&sa)[R / 16], uint4 (&sb)[R / 16]) {
        const uint4 *pa = reinterpret_cast<const uint4 *>(sp + ((codes_a >> (8 * k)) & 0xffu) * R);
        const uint4 *pb = reinterpret_cast<const uint4 *>(sp + ((codes_b >> (8 * k)) & 0xffu) * R);
#pragma unroll
        for (int x = 0; x < R / 16; ++x) {
            sa[x] = pa[x];
            sb[x] = pb[x];
        }
    };
    auto one_column = [&](const uint2 top, const uint4 (&sa)[R / 16], const uint4 (&sb)[R / 16]) {
        unsigned e = top.y, hlast;
        local_column<R>(h, f, sa, sb, hdo, e, hlast, mx, kb, go, ge, sel);
        hdo = top.x;
        if (!last) bp[0] = make_uint2(hlast, e);
        bp += 64;
    };
    // columns 1 .. qmax, four at a time (one dword of codes per query); the codes beyond qmax are the ghost's
    for (int j = 1; j <= qmax; j += 4) {
        const uint2 top0 = bp[0], top1 = bp[64], top2 = bp[128], top3 = bp[192];
        const unsigned qa = qst[0], qb = qst[64];
        qst += 128;
        uint4 sa0[R / 16], sb0[R / 16], sa1[R / 16], sb1[R / 16];
        scores_of(qa, qb, 0, sa0, sb0);
        one_column(top0, sa0, sb0);
        if (j + 1 > qmax) break;
        scores_of(qa, qb, 1, sa1, sb1);
        one_column(top1, sa1, sb1);
        if (j + 2 > qmax) break;
        scores_of(qa, qb, 2, sa0, sb0);
        one_column(top2, sa0, sb0);
        if (j + 3 > qmax) break;
        scores_of(qa, qb, 3, sa1, sb1);
        one_column(top3, sa1, sb1);
    }
}

__global__ __launch_bounds__(64, 3) void sw_local_lane_kernel(const LocalArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int R = LA_R;
    const int lane = threadIdx.x;
    const int64_t tiles = (a.count + 127) >> 7, slots = gridDim.x, slot = blockIdx.x;
    unsigned long long *const ctr = reinterpret_cast<unsigned long long *>(a.tile_ctr); // {draws, waves out}: ONE object

    reinterpret_cast<unsigned *>(smem + LA_LDS_CODE)[lane] = reinterpret_cast<const unsigned *>(a.code)[lane];
#pragma unroll
    for (int x = 0; x < MATRIX_DIM * MATRIX_DIM / 256; ++x)
        reinterpret_cast<unsigned *>(smem + LA_LDS_M)[x * 64 + lane] = reinterpret_cast<const unsigned *>(a.matrix)[x * 64 + lane];
    if (lane < LA_R / 4) reinterpret_cast<unsigned *>(smem + LA_LDS_SP + LOCAL_GHOST_CODE * LA_R)[lane] = 0u; // the ghost's row
    const unsigned char *const code_of = smem + LA_LDS_CODE;
    const signed char *const mat = reinterpret_cast<const signed char *>(smem + LA_LDS_M);
    unsigned char *const sp = smem + LA_LDS_SP;
    unsigned char *const tcode = smem + LA_LDS_T;

    const int K = local_lane_bias(a.smin);
    const unsigned kb = pack2(K, K), go = pack2(a.gopen, a.gopen), ge = pack2(a.gext, a.gext);
    unsigned sel[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        sel[u] = 0x0c040c00u + 0x00010001u * (unsigned)u;
        asm volatile("" : "+s"(sel[u]));
    }
    unsigned char *const region = a.ws + (int64_t)slot * local_lane_region_bytes(a.max_ql);
    uint2 *const bnd = reinterpret_cast<uint2 *>(region) + lane;
    unsigned *const qst = reinterpret_cast<unsigned *>(region + local_lane_bnd_bytes(a.max_ql)) + lane;

    for (int64_t draw = slot; draw < tiles;) {
        const int64_t tile = a.tile_order[draw];
        const int64_t p0 = a.first + tile * 128;
        const int cnt = (int)min((int64_t)128, a.count - tile * 128);
        const bool validA = 2 * lane < cnt, validB = 2 * lane + 1 < cnt;
        const int64_t pA = p0 + (validA ? 2 * lane : 0), pB = p0 + (validB ? 2 * lane + 1 : 0);
        // ---- the promise: one target (start and length); query lengths may differ
        const int tl = __builtin_amdgcn_readfirstlane(a.t.len[p0]);
        const int64_t t0 = a.t.off[p0];
        const unsigned t0lo = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long long)t0), t0hi = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)t0 >> 32));
        const int64_t tstart = (int64_t)((unsigned long long)t0lo | (unsigned long long)t0hi << 32);
        const int qlA = validA ? a.q.len[pA] : 0, qlB = validB ? a.q.len[pB] : 0;
        const bool mine = (!validA || (a.t.off[pA] == tstart && a.t.len[pA] == tl)) && (!validB || (a.t.off[pB] == tstart && a.t.len[pB] == tl)) &&
                          qlA >= 0 && qlB >= 0 && qlA <= a.max_ql && qlB <= a.max_ql;
        if (__builtin_amdgcn_ballot_w64(!mine) != 0ull || tl < 0 || tl > a.max_tl) {
            if (a.status) {
                if (validA) a.status[pA] = 1; // MGL_SW_ERR_BAD_ARG
                if (validB) a.status[pB] = 1;
            }
        } else {
            int qmax = max(qlA, qlB);
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) qmax = max(qmax, __shfl_xor(qmax, m));
            qmax = __builtin_amdgcn_readfirstlane(qmax);
            unsigned mx = 0u;
            if (tl > 0 && qmax > 0) {
                const int strips = lane_strips(tl, R);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // (the previous tile's readers of tcode / sp are through)
                __builtin_amdgcn_wave_barrier();
                for (int x = lane; x < strips * R; x += 64) tcode[x] = x < tl ? code_of[a.t.data[tstart + x]] : (unsigned char)0xff;
                {
                    const unsigned char *const qa = a.q.data + (validA ? a.q.off[pA] : 0), *const qb = a.q.data + (validB ? a.q.off[pB] : 0);
                    for (int cb = 0; cb < (qmax + 3) >> 2; ++cb) {
                        unsigned wa = 0, wb = 0;
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const int col = 4 * cb + k;
                            wa |= (unsigned)(col < qlA ? code_of[qa[col]] : LOCAL_GHOST_CODE) << (8 * k);
                            wb |= (unsigned)(col < qlB ? code_of[qb[col]] : LOCAL_GHOST_CODE) << (8 * k);
                        }
                        qst[(size_t)(2 * cb) * 64] = wa;
                        qst[(size_t)(2 * cb + 1) * 64] = wb;
                    }
                    for (int j = 0; j <= qmax; ++j) bnd[(size_t)j * 64] = make_uint2(0u, 0u); // H[0][j] = 0, E[1][j] = max(-o, -inf), floored
                }
                for (int k = 0; k < strips; ++k) {
                    // ---- the strip profile: lane l writes the 16 rows (l & 1) * 16 .. + 15 of code l >> 1; rows beyond the target are 0
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    {
                        const int code = lane >> 1, r0 = (lane & 1) * 16;
                        unsigned w[4];
#pragma unroll
                        for (int x = 0; x < 4; ++x) {
                            unsigned v = 0;
#pragma unroll
                            for (int y = 0; y < 4; ++y) {
                                const int tc = tcode[k * R + r0 + 4 * x + y];
                                const unsigned b = tc == 0xff ? 0u : (unsigned)((int)mat[tc * MATRIX_DIM + code] + K) & 0xffu;
                                v |= b << (8 * y);
                            }
                            w[x] = v;
                        }
                        *reinterpret_cast<uint4 *>(sp + code * R + r0) = make_uint4(w[0], w[1], w[2], w[3]);
                    }
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    local_strip(qmax, bnd, qst, sp, kb, go, ge, sel, k == strips - 1, mx);
                }
            }
            if (validA) {
                a.hit[pA] = LocalHit{(int)(mx & 0xffffu), 0, 0, 0, 0};
                if (a.status) a.status[pA] = 0;
            }
            if (validB) {
                a.hit[pB] = LocalHit{(int)(mx >> 16), 0, 0, 0, 0};
                if (a.status) a.status[pB] = 0;
            }
        }
        if (tiles <= slots) break;
        unsigned next = 0;
        if (lane == 0) {
            next = (unsigned)__hip_atomic_fetch_add(ctr, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (next >= (unsigned)tiles && a.grid_fault) __hip_atomic_store(a.grid_fault, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        draw = slots + (int64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)next);
    }
    if (tiles > slots && lane == 0) { // the last wave out zeroes the counter (sw_dp16_lane_ck.hip)
        const unsigned out = (unsigned)(__hip_atomic_fetch_add(ctr, 1ull << 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 32);
        if (out == (unsigned)slots - 1u)
            __hip_atomic_store(ctr, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else if (out >= (unsigned)slots && a.grid_fault)
            __hip_atomic_store(a.grid_fault, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

} // namespace

// a.lane_slots regions of local_lane_region_bytes(a.max_ql) at a.ws; the tiles drawn in the order a.tile_order; a.tile_ctr (zero) where
// the tiles outnumber the slots
hipError_t launch_local_lane(const LocalArgs &a, hipStream_t stream)
{
    const int64_t tiles = (a.count + 127) / 128;
    if (tiles < 1) return hipSuccess;
    if (a.lane_slots < 1 || !a.matrix || !a.code || !a.hit || !a.ws || !a.tile_order || (tiles > a.lane_slots && !a.tile_ctr) ||
        !local_lane_ok(a.smin, a.smax, a.gopen, a.gext, a.max_tl, a.max_ql))
        return hipErrorInvalidValue;
    const int lds = local_lane_lds_bytes(a.max_tl);
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_local_lane_kernel, dim3((unsigned)std::min<int64_t>(tiles, a.lane_slots)), dim3(64), lds, stream, a);
    return hipGetLastError();
}

} // namespace mgl_sw_dev
