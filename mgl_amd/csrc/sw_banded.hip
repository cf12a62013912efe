// sw_banded.hip -- sw_banded_kernel, the kernel of mgl_sw_align_batch_device_banded: the GATK function (DESIGN.md section 2's
// recurrence, priorities, tie rules, end-cell scans and walk) over the cells of a diagonal band only (the
// function is tests/banded_textbook.py's, which the tests compare with).
//
// One wave per pair, int32.  The mapping of the band onto the wave, the sweep of a strip of 64 rows, the four decision bits per cell,
// the wave-wide walk and the CIGAR output are sw_band_wave.h's, shared with sw_extend.hip and described there.  What is here: the
// per-pair guards, row 0, the scans of the last column's and the last row's in-band cells for the end cell, and what each overhang
// strategy does before and after the walk.
#include "sw_band_wave.h"

namespace mgl_sw_dev {

namespace {

__global__ __launch_bounds__(64) void sw_banded_kernel(const BandedArgs a)
{
    const int lane = threadIdx.x;
    const int o = a.gopen, e = a.gext;
    const bool indel = (a.strategy & (OS_INDEL | OS_LEAD_ID)) != 0;
    unsigned char *const slot = a.ws + (int64_t)blockIdx.x * a.slot_bytes;

    for (int64_t p = blockIdx.x; p < a.n; p += a.slots) {
        const int tl = a.t.len[p], ql = a.q.len[p];
        Score sc{0, 0, 0, 0, 0, 0};
        auto finish = [&](const int status, const int offset, const int cigar_len) {
            if (lane != 0) return;
            a.offset[p] = offset;
            if (a.score) a.score[p] = sc;
            if (a.status) a.status[p] = status;
            if (a.cigar_len) a.cigar_len[p] = cigar_len;
        };
        if (tl < 1 || ql < 1 || tl > a.max_tl || ql > a.max_ql) {
            finish(ST_BAD_ARG, 0, 0);
            continue;
        }
        if (!banded_range_ok(tl, ql, a.match, a.mismatch, o, e) || banded_pair_bytes(tl, ql, a.band, a.score_only != 0) > a.slot_bytes) {
            finish(ST_UNSUPPORTED, 0, 0);
            continue;
        }
        const int lo = banded_lo(tl, ql, a.band), hi = banded_hi(tl, ql, a.band);
        int2 *const carry = reinterpret_cast<int2 *>(slot);
        uint32_t *const elems = reinterpret_cast<uint32_t *>(slot + banded_carry_bytes(ql));
        uint32_t *const dir = reinterpret_cast<uint32_t *>(slot + banded_carry_bytes(ql) + banded_elem_bytes(tl, ql));
        const int64_t strip_words = (int64_t)banded_strip_steps(tl, ql, a.band) * 8;
        const int64_t ts = a.t.off[p];
        const unsigned char *const tq = a.q.data + a.q.off[p];

        // row 0: the border's H and the E that enters row 1, minus infinity beyond the band
        for (int j = lane; j <= ql; j += 64) {
            const int b = border(j, o, e, indel);
            carry[j] = j <= hi ? make_int2(b, b - o) : make_int2(NEG, NEG);
        }
        __threadfence_block();
        __builtin_amdgcn_wave_barrier();

        int mq = NEG, mqt = -1; // the lane's last-column best: later rows win ties
        const int strips = (tl + 63) / 64;
        for (int k = 0; k < strips; ++k) {
            Swept sw;
            const Strip st = strip_setup(k, lane, tl, ql, lo, hi, o, e, indel, a.t.data + ts, tq, carry, dir + (int64_t)k * strip_words);
            sweep_strip<false>(st, lane, a.match, a.mismatch, o, e, !a.score_only, sw);
            if (st.s_last != NEVER && sw.h_last >= mq) {
                mq = sw.h_last;
                mqt = 64 * k + lane + 1;
            }
            __threadfence_block(); // the carry row before the next strip (or the last-row scan) reads it
            __builtin_amdgcn_wave_barrier();
        }
        // ---- the last column: the largest H, the later row among equals
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const int oq = __shfl_xor(mq, m), ot = __shfl_xor(mqt, m);
            const bool take = oq > mq || (oq == mq && ot > mqt);
            mq = take ? oq : mq;
            mqt = take ? ot : mqt;
        }
        // ---- the last row's in-band cells in column order: a larger H takes over, an equal one only when strictly nearer the
        // diagonal -- so the winner is the first of the nearest among the largest
        int rb = NEG, rj = 0x7fffffff;
        for (int j = max(1, tl + lo) + lane; j <= ql; j += 64) {
            const int h = carry[j].x;
            const int d = abs(tl - j), bd = abs(tl - rj);
            if (h > rb || (h == rb && d < bd)) { // (a lane's columns ascend: among equals at equal distance the first stays)
                rb = h;
                rj = j;
            }
        }
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const int ob = __shfl_xor(rb, m), oj = __shfl_xor(rj, m);
            const int d = abs(tl - rj), od = abs(tl - oj);
            const bool take = ob > rb || (ob == rb && (od < d || (od == d && oj < rj)));
            rb = take ? ob : rb;
            rj = take ? oj : rj;
        }
        sc.mqe = mq;
        sc.mqe_t = mqt;
        sc.max = mq;
        sc.max_t = mqt;
        sc.max_q = ql;
        sc.seg_length = 0;
        if (rb > mq || (rb == mq && abs(tl - rj) < abs(mqt - ql))) {
            sc.max = rb;
            sc.max_t = tl;
            sc.max_q = rj;
            sc.seg_length = ql - rj;
        }
        if (a.score_only) {
            finish(0, 0, 0);
            continue;
        }

        // ---- the walk, the whole wave on one path
        const Dirs dv{dir, lo, hi, strip_words};
        int I, J, seg = 0;
        if (a.strategy == OS_INDEL) {
            I = tl;
            J = ql;
        } else if (a.strategy != OS_LEAD_ID) {
            I = sc.max_t;
            J = sc.max_q;
            seg = sc.seg_length;
        } else {
            I = sc.mqe_t;
            J = ql;
        }
        Elems el{elems, lane, a.binary_cigar, 0, 0};
        if (seg > 0 && a.strategy == OS_SOFTCLIP) {
            el.push(OP_S, seg);
            seg = 0;
        }
        const Walked w = walk(dv, lane, I, J, seg, el);
        I = w.I;
        J = w.J;
        seg = w.seg;
        const unsigned state = w.state;
        int off;
        if (a.strategy == OS_SOFTCLIP) {
            el.push(state, seg);
            if (J > 0) el.push(OP_S, J);
            off = I;
        } else if (a.strategy == OS_IGNORE) {
            el.push(state, seg + J);
            off = I - J;
        } else {
            el.push(state, seg);
            if (I > 0) el.push(OP_D, I);
            else if (J > 0) el.push(OP_I, J);
            off = 0;
        }
        const int cap = a.binary_cigar ? a.cigar_stride & ~3 : a.cigar_stride;
        if (el.size > cap) {
            finish(ST_CIGAR_OVERFLOW, 0, el.size);
            continue;
        }
        el.write<true>(a.cigar + p * (int64_t)a.cigar_stride);
        finish(0, off, el.size);
        __threadfence_block(); // (the next pair reuses the slot)
        __builtin_amdgcn_wave_barrier();
    }
}

} // namespace

// pairs 0 .. n - 1 on a.slots waves, wave w in workspace slot w
hipError_t launch_banded(const BandedArgs &a, hipStream_t stream)
{
    if (a.n < 1) return hipSuccess;
    if (!a.offset || !a.ws || a.slots < 1 || a.slot_bytes < 256 || (!a.score_only && (!a.cigar || !a.cigar_len)) || (a.score_only && !a.score)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_banded_kernel, dim3((unsigned)a.slots), dim3(64), 0, stream, a);
    return hipGetLastError();
}

} // namespace mgl_sw_dev
