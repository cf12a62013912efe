// sw_cigar_wave.h -- what one wave does with one alignment's CIGAR slot, once, for the kernels that stand behind an alignment entry
// (sw_describe.hip, sw_pileup.hip): the check of the record and the slot before any base is read, and the parse of the slot into the
// wave's part of LDS, a chunk of elements at a time.  Device code only; everything is inlined into the kernel that includes it.
//
// The check: the CIGAR slot is read 64 bytes (text) or 64 words (binary) a step, a lane each.  In text the operation bytes are found
// by a ballot, and an operation's lane forms its number from the digits between the previous operation and itself -- the step's bytes
// lie in LDS for that -- or, where there is no operation in front of it in the step, behind the digits carried over from the steps
// before.  The lanes add up what their elements spend in 64 bits.  A slot passes with every element M / I / D with 1 <= len < 2^31, no
// byte left over, and both sums equal to the spans.
// The parse: the slot again, now into LDS, DESCRIBE_CHUNK elements at a time (a step never yields more than 64, so a chunk is closed
// while 64 still fit): len, op and the element's offsets in the two spans, from a wave prefix scan.
#ifndef MGL_SW_CIGAR_WAVE_H
#define MGL_SW_CIGAR_WAVE_H

#include "sw_describe.h"

namespace mgl_sw_dev {
namespace cigar_wave {

constexpr int OP_M = 0, OP_I = 1, OP_D = 2, OP_EQ = 7, OP_X = 8, OP_NONE = -1;
constexpr uint64_t NUM_SAT = (uint64_t)1 << 40; // a number beyond 32 bits stays beyond them
constexpr int DIG_SAT = 1 << 20;

struct WaveLds {
    int32_t len[DESCRIBE_CHUNK], toff[DESCRIBE_CHUNK], qoff[DESCRIBE_CHUNK];
    uint8_t op[DESCRIBE_CHUNK];
    uint8_t txt[64];
};

__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int top_bit(const uint64_t m) { return 63 - __clzll((long long)m); } // m != 0

struct Parser {
    const char *slot;
    int bytes, pos;
    bool binary, words;
    uint64_t cval; // text: the digits behind the last operation so far
    int cdig;
    bool bad;
    int64_t acc_t, acc_q; // the check: this lane's elements
    int base_t, base_q;   // the parse: the spans spent in front of the next element
};

// one step of the slot: up to 64 elements.  STORE: into the chunk at `count`; else into the lanes' sums.  -> the elements it found
template <bool STORE>
__device__ __forceinline__ int parse_step(Parser &P, WaveLds &L, const int lane, const int count)
{
    const uint64_t lt = ((uint64_t)1 << lane) - 1;
    bool isop = false, bad = false;
    int len = 0, op = OP_M;
    if (P.binary) {
        const int cnt = min(64, (P.bytes - P.pos) / 4);
        isop = lane < cnt;
        uint32_t v = 0;
        if (isop) {
            const char *const at = P.slot + P.pos + 4 * lane;
            if (P.words) v = *reinterpret_cast<const uint32_t *>(at);
            else v = (uint32_t)(uint8_t)at[0] | (uint32_t)(uint8_t)at[1] << 8 | (uint32_t)(uint8_t)at[2] << 16 | (uint32_t)(uint8_t)at[3] << 24;
        }
        len = (int)(v >> 4);
        op = (int)(v & 15u);
        bad = isop && (op > OP_D || len < 1);
        P.pos += 4 * cnt;
    } else {
        const int cnt = min(64, P.bytes - P.pos);
        const bool in = lane < cnt;
        const uint8_t b = in ? (uint8_t)P.slot[P.pos + lane] : (uint8_t)0;
        L.txt[lane] = b;
        wave_sync();
        isop = in && (b == 'M' || b == 'I' || b == 'D');
        const bool isdig = in && b >= '0' && b <= '9';
        bad = in && !isop && !isdig;
        const uint64_t opmask = __ballot(isop);
        const uint64_t below = opmask & lt;
        const int j = below ? top_bit(below) : -1;
        if (isop) {
            uint64_t val = j < 0 ? P.cval : 0;
            const int nd = (j < 0 ? P.cdig : 0) + lane - j - 1;
            for (int k = j + 1; k < lane; ++k) val = min(val * 10 + (uint64_t)(uint8_t)(L.txt[k] - '0'), NUM_SAT);
            bad |= nd == 0 || val == 0 || val > (uint64_t)0x7fffffff;
            len = (int)min(val, (uint64_t)0x7fffffff);
            op = b == 'M' ? OP_M : b == 'I' ? OP_I : OP_D;
        }
        // what is left behind the step's last operation
        const int h = opmask ? top_bit(opmask) : -1;
        if (h >= 0) {
            P.cval = 0;
            P.cdig = 0;
        }
        for (int k = h + 1; k < cnt; ++k) P.cval = min(P.cval * 10 + (uint64_t)(uint8_t)(L.txt[k] - '0'), NUM_SAT);
        P.cdig = min(P.cdig + cnt - 1 - h, DIG_SAT);
        wave_sync(); // txt is written again by the next step
        P.pos += cnt;
    }
    if (__ballot(bad)) {
        P.bad = true;
        return 0;
    }
    const int dt = isop && op != OP_I ? len : 0, dq = isop && op != OP_D ? len : 0;
    const uint64_t mask = __ballot(isop);
    if (!STORE) {
        P.acc_t += dt;
        P.acc_q += dq;
    } else { // (the slot has passed the check: both sums are below 2^31, so the halves do not carry into each other)
        const unsigned long long mine = (unsigned long long)(unsigned)dt | (unsigned long long)(unsigned)dq << 32;
        unsigned long long incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        if (isop) {
            const int at = count + __popcll(mask & lt);
            const unsigned long long excl = incl - mine;
            L.len[at] = len;
            L.op[at] = (uint8_t)op;
            L.toff[at] = P.base_t + (int)(unsigned)(excl & 0xffffffffull);
            L.qoff[at] = P.base_q + (int)(unsigned)(excl >> 32);
        }
        const unsigned long long tot = __shfl(incl, 63);
        P.base_t += (int)(unsigned)(tot & 0xffffffffull);
        P.base_q += (int)(unsigned)(tot >> 32);
    }
    return __popcll(mask);
}

__device__ __forceinline__ int64_t wave_sum64(long long v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

// The check of alignment p's record r and slot, nothing of the sequences read: -> whether it passes, with P set up on the slot (its
// position behind the last byte; see rewind)
__device__ __forceinline__ bool check_alignment(Parser &P, WaveLds &L, const int lane, const mgl_sw_chain_alignment &r, const int tl, const int ql,
                                                const int cl, const char *const slot, const int cigar_stride, const int binary)
{
    bool ok = 0 <= r.t_beg && r.t_beg <= r.t_end && r.t_end <= tl && 0 <= r.q_beg && r.q_beg <= r.q_end && r.q_end <= ql;
    ok = ok && cl >= 0 && cl <= cigar_stride && (!binary || (cl & 3) == 0);
    P.slot = slot;
    P.bytes = ok ? cl : 0;
    P.binary = binary != 0;
    P.words = (reinterpret_cast<uintptr_t>(P.slot) & 3) == 0;
    if (ok) {
        while (P.pos < P.bytes && !P.bad) parse_step<false>(P, L, lane, 0);
        const int64_t st = wave_sum64(P.acc_t), sq = wave_sum64(P.acc_q);
        ok = !P.bad && (P.binary || P.cdig == 0) && st == (int64_t)r.t_end - r.t_beg && sq == (int64_t)r.q_end - r.q_beg;
    }
    return ok;
}

// back to the slot's first byte, for the parse
__device__ __forceinline__ void rewind(Parser &P)
{
    P.pos = 0;
    P.cval = 0;
    P.cdig = 0;
}

} // namespace cigar_wave
} // namespace mgl_sw_dev

#endif
