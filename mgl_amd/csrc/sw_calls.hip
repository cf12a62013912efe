// sw_calls.hip -- sw_insertions_kernel, sw_genotype_count_kernel and sw_genotype_write_kernel (the definition is
// tests/calls_textbook.py's).
//
// sw_insertions_kernel: sw_pileup_kernel's frame -- one wave per alignment, persistent over the batch, the status and select words
// first, the check of sw_cigar_wave.h whole before the first add, the slot parsed into LDS a chunk at a time -- and another walk: M
// and D elements are skipped.  The chunk is taken 64 elements a step, a lane each: the lane of an I element looks its position, the
// one in front of the target cursor, up among the active sites by a binary search that never leaves the S records whatever they
// hold.  The wave then takes the matched elements in turn by ballot: lane j < L reads inserted base j and adds 1 to its column's
// channel word, lane 0 adds 1 to the length word (word 0 alone where L > max_ins).  max_ins is at most 64, so an element is one step.
// Every add is a relaxed, agent-scope atomic whose result is not used, as sw_pileup.hip's add_word.  No scratch; the LDS is WaveLds.
//
// The genotype entry: a thread per site slot.  sw_genotype_count_kernel counts the slot's events (0 to 3; a slot behind the active
// sites has none) and sums them over its block of CALLS_SITE_BLOCK slots; rocPRIM's device-wide exclusive scan turns the blocks'
// counts into the blocks' first places; sw_genotype_write_kernel evaluates the slots of the blocks that have events in front of the
// capacity again and writes their records in site order, and inside a site SNV, deletion, insertion.
#include "sw_calls.h"

#include <rocprim/device/device_scan.hpp>

#include "sw_cigar_wave.h"

namespace mgl_sw_dev {

namespace {

using namespace cigar_wave;

// A / a 0, C / c 1, G / g 2, T / t 3, every other byte 4 (sw_pileup.hip's rule)
__device__ __forceinline__ int channel_of(const uint8_t b)
{
    const uint8_t u = b & 0xdf;
    return u == 'A' ? 0 : u == 'C' ? 1 : u == 'G' ? 2 : u == 'T' ? 3 : 4;
}

__device__ __forceinline__ void add_word(uint32_t *const at, const uint32_t v)
{
    (void)__hip_atomic_fetch_add(at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int64_t active_sites(const int64_t *const n_sites, const int64_t site_capacity)
{
    return min(max(n_sites[0], (int64_t)0), site_capacity);
}

// -> the site among sites[0 .. S) whose pos is `want`, -1 where there is none.  Every read lies inside the S records
__device__ __forceinline__ int64_t find_site(const mgl_sw_site *const sites, const int64_t S, const int64_t want)
{
    int64_t lo = 0, hi = S;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)sites[mid].pos < want) lo = mid + 1;
        else hi = mid;
    }
    return lo < S && (int64_t)sites[lo].pos == want ? lo : -1;
}

__global__ __launch_bounds__(64 * DESCRIBE_WAVES) void sw_insertions_kernel(const InsertionsArgs a)
{
    __shared__ WaveLds lds[DESCRIBE_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    WaveLds &L = lds[wave];
    const int64_t waves = (int64_t)gridDim.x * DESCRIBE_WAVES;
    const int64_t S = active_sites(a.n_sites, a.site_capacity);
    const int64_t W = 6 * (int64_t)a.max_ins + 1;
    for (int64_t p = (int64_t)blockIdx.x * DESCRIBE_WAVES + wave; p < a.n; p += waves) {
        auto finish = [&](const int status) {
            if (lane == 0 && a.status) a.status[p] = status;
        };
        const int sin = a.status_in ? a.status_in[p] : 0;
        if (sin != 0) { // nothing of the alignment is read
            finish(sin);
            continue;
        }
        if (a.select && a.select[p] == 0) {
            finish(MGL_SW_OK);
            continue;
        }
        const mgl_sw_chain_alignment r = a.aln[p];
        Parser P{};
        if (!check_alignment(P, L, lane, r, a.t_len[p], a.q_len[p], a.cigar_len[p], a.cigar + p * (int64_t)a.cigar_stride, a.cigar_stride, a.binary)) {
            finish(MGL_SW_ERR_BAD_ARG);
            continue;
        }
        // ---- the walk: the first target column stands at rel0, counted from the region's first position, as a site's pos is
        const int64_t rel0 = a.t_start[p] + r.t_beg - a.region_beg;
        const uint8_t *const Q = a.queries + a.q_start[p] + r.q_beg;
        rewind(P);
        while (P.pos < P.bytes) {
            int count = 0;
            while (P.pos < P.bytes && count + 64 <= DESCRIBE_CHUNK) count += parse_step<true>(P, L, lane, count);
            wave_sync();
            for (int e0 = 0; e0 < count; e0 += 64) {
                const int e = e0 + lane;
                int64_t row = -1;
                if (e < count && L.op[e] == OP_I) row = find_site(a.sites, S, rel0 + L.toff[e] - 1); // behind the position in front of the cursor
                uint64_t matched = __ballot(row >= 0);
                while (matched) {
                    const int src = __ffsll((unsigned long long)matched) - 1;
                    matched &= matched - 1;
                    const int len = L.len[e0 + src];
                    uint32_t *const words = a.ins + __shfl(row, src) * W;
                    if (len > a.max_ins) {
                        if (lane == 0) add_word(words, 1u);
                    } else {
                        if (lane < len) add_word(words + a.max_ins + 1 + 5 * lane + channel_of(Q[L.qoff[e0 + src] + lane]), 1u);
                        if (lane == 0) add_word(words + len, 1u);
                    }
                }
            }
            wave_sync(); // the chunk is written again
        }
        finish(MGL_SW_OK);
    }
}

// ---- the genotype entry

struct Event {
    int kind, len, ref, alt, flags;
    int64_t depth, r, a;
};

// a site's events in their order: slot 0 the SNV, 1 the deletion, 2 the insertion (fixed places: no indexed register array)
struct Events {
    bool has[3];
    Event e[3];
    __device__ __forceinline__ int n() const { return (int)has[0] + (int)has[1] + (int)has[2]; }
};

// the events of site slot s, all arithmetic in 64 bits.  A slot behind the active sites, and a site whose pos lies outside the
// table, has none
__device__ __forceinline__ Events events_at(const GenotypeArgs &g, const int64_t S, const int64_t s)
{
    Events out{};
    if (s >= S) return out;
    const mgl_sw_site site = g.sites[s];
    const int64_t pos = site.pos;
    if (pos < 0 || pos >= g.region_len) return out;
    int64_t c[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) c[k] = (int64_t)g.counts[k * g.region_len + pos];
    const int64_t depth = c[0] + c[1] + c[2] + c[3] + c[4] + c[5];
    const int ref = channel_of(g.ref[pos]);
    int64_t cref = c[0];
#pragma unroll
    for (int k = 1; k < 5; ++k) cref = ref == k ? c[k] : cref;
    if ((site.flags & 2) && ref <= 3 && site.alt >= 0 && site.alt <= 3) {
        int64_t calt = c[0];
#pragma unroll
        for (int k = 1; k < 4; ++k) calt = site.alt == k ? c[k] : calt;
        out.has[0] = true;
        out.e[0] = Event{1, 1, ref, site.alt, 0, depth, cref, calt};
    }
    auto deleted = [&](const int64_t k, const int64_t at) { // site k is a deletion site at position `at`
        if (k < 0 || k >= S) return false;
        const mgl_sw_site o = g.sites[k];
        return (o.flags & 4) != 0 && (int64_t)o.pos == at;
    };
    if ((site.flags & 4) && !deleted(s - 1, pos - 1)) { // a run's first position
        int len = 1;
        while (len < g.max_del && deleted(s + len, pos + len)) ++len;
        out.has[1] = true;
        out.e[1] = Event{2, len, ref, -1, deleted(s + len, pos + len) ? 1 : 0, depth, cref, c[5]};
    }
    if ((site.flags & 8) && g.ins) {
        const uint32_t *const words = g.ins + s * (6 * (int64_t)g.max_ins + 1);
        uint32_t best = 0;
        int len = 0;
        for (int l = 1; l <= g.max_ins; ++l) {
            const uint32_t w = words[l];
            if (w > best) { // (the smallest length wins a tie)
                best = w;
                len = l;
            }
        }
        out.has[2] = len != 0;
        out.e[2] = Event{3, len, ref, -1, 0, depth, max(depth - c[6], (int64_t)0), (int64_t)best};
    }
    return out;
}

// -> this thread's first place among the block's events and (in every thread) their number
__device__ __forceinline__ int block_places(const int mine, int &total)
{
    __shared__ int wave_events[CALLS_SITE_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    if (lane == 63) wave_events[wave] = incl;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < CALLS_SITE_BLOCK / 64; ++w) {
        before += w < wave ? wave_events[w] : 0;
        total += wave_events[w];
    }
    return before + incl - mine;
}

__global__ __launch_bounds__(CALLS_SITE_BLOCK) void sw_genotype_count_kernel(const GenotypeArgs g)
{
    const int64_t S = active_sites(g.n_sites, g.site_capacity);
    const int64_t s = (int64_t)blockIdx.x * CALLS_SITE_BLOCK + threadIdx.x;
    int total;
    block_places(events_at(g, S, s).n(), total);
    if (threadIdx.x == 0) {
        g.block_count[blockIdx.x] = total;
        if (blockIdx.x == 0) g.block_count[g.blocks] = 0; // the scan's last place is the number of all events
    }
}

__device__ __forceinline__ int32_t clip31(const int64_t v) { return (int32_t)min(v, (int64_t)0x7fffffff); }

__global__ __launch_bounds__(CALLS_SITE_BLOCK) void sw_genotype_write_kernel(const GenotypeArgs g)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) g.n_calls[0] = g.block_start[g.blocks];
    const int64_t first = g.block_start[blockIdx.x];
    if (g.block_count[blockIdx.x] == 0 || first >= g.call_capacity) return; // (the same in every thread)
    const int64_t S = active_sites(g.n_sites, g.site_capacity);
    const int64_t s = (int64_t)blockIdx.x * CALLS_SITE_BLOCK + threadIdx.x;
    const Events ev = events_at(g, S, s);
    int total;
    int64_t at = first + block_places(ev.n(), total);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (!ev.has[k] || at >= g.call_capacity) continue; // (the places ascend: behind the capacity nothing more is written)
        const Event &e = ev.e[k];
        const int64_t l0 = e.r * g.cost_match + e.a * g.cost_error, l1 = (e.r + e.a) * g.cost_het, l2 = e.a * g.cost_match + e.r * g.cost_error;
        const int64_t m = min(l0, min(l1, l2));
        const int32_t pl0 = clip31((l0 - m + 128) >> 8), pl1 = clip31((l1 - m + 128) >> 8), pl2 = clip31((l2 - m + 128) >> 8);
        mgl_sw_call o;
        o.pos = g.sites[s].pos;
        o.kind = e.kind;
        o.len = e.len;
        o.ref = e.ref;
        o.alt = e.alt;
        o.depth = clip31(e.depth);
        o.ref_count = clip31(e.r);
        o.alt_count = clip31(e.a);
        o.gt = l0 == m ? 0 : l1 == m ? 1 : 2;
        o.gq = min(99, o.gt == 0 ? min(pl1, pl2) : o.gt == 1 ? min(pl0, pl2) : min(pl0, pl1));
        o.qual = pl0;
        o.pl0 = pl0;
        o.pl1 = pl1;
        o.pl2 = pl2;
        o.flags = e.flags;
        o.reserved = 0;
        g.calls[at] = o;
        if (g.ins_seq) { // the call's row: an insertion's bases and zeros behind them; zeros for the other kinds
            uint8_t *const row = g.ins_seq + at * g.max_ins;
            const uint32_t *const cols = g.ins ? g.ins + s * (6 * (int64_t)g.max_ins + 1) + g.max_ins + 1 : nullptr;
            for (int j = 0; j < g.max_ins; ++j) {
                uint8_t b = 0;
                if (e.kind == 3 && j < e.len) {
                    uint32_t best = cols[5 * j];
                    int ch = 0;
                    for (int k2 = 1; k2 < 5; ++k2) {
                        if (cols[5 * j + k2] > best) { // (the lowest channel wins a tie)
                            best = cols[5 * j + k2];
                            ch = k2;
                        }
                    }
                    b = (uint8_t)(0x4e54474341ull >> (8 * ch)); // "ACGTN", a byte a channel
                }
                row[j] = b;
            }
        }
        ++at;
    }
}

bool genotype_args_good(const GenotypeArgs &g)
{
    return g.counts && g.ref && g.sites && g.n_sites && g.n_calls && g.region_len >= 1 && g.region_len <= 0x7fffffff && g.site_capacity >= 1 &&
           g.site_capacity <= ((int64_t)1 << 30) && g.blocks == (g.site_capacity + CALLS_SITE_BLOCK - 1) / CALLS_SITE_BLOCK && g.block_count &&
           g.block_start && g.max_ins >= 1 && g.max_ins <= CALLS_MAX_INS && g.max_del >= 1 && g.max_del <= CALLS_MAX_DEL && g.call_capacity >= 0 &&
           g.call_capacity <= CALLS_MAX_CALLS && (g.calls || g.call_capacity == 0) && (g.ins_seq || !g.ins || g.call_capacity == 0);
}

} // namespace

hipError_t launch_insertions(const InsertionsArgs &a, hipStream_t stream)
{
    if (a.n < 1) return hipSuccess;
    if (a.n > DESCRIBE_MAX_CHUNK || a.groups < 1 || a.cigar_stride < 0) return hipErrorInvalidValue;
    if (!a.queries || !a.t_start || !a.q_start || !a.t_len || !a.q_len || !a.aln || !a.cigar || !a.cigar_len) return hipErrorInvalidValue;
    if (!a.sites || !a.n_sites || !a.ins || a.region_beg < 0 || a.site_capacity < 1 || a.site_capacity > ((int64_t)1 << 30)) return hipErrorInvalidValue;
    if (a.max_ins < 1 || a.max_ins > CALLS_MAX_INS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_insertions_kernel, dim3((unsigned)a.groups), dim3(64 * DESCRIBE_WAVES), 0, stream, a);
    return hipGetLastError();
}

hipError_t genotype_scan_bytes(const int64_t entries, size_t *bytes)
{
    if (entries < 1 || !bytes) return hipErrorInvalidValue;
    *bytes = 0;
    return rocprim::exclusive_scan(nullptr, *bytes, (const int64_t *)nullptr, (int64_t *)nullptr, (int64_t)0, (size_t)entries, rocprim::plus<int64_t>(), 0);
}

hipError_t launch_genotype_count(const GenotypeArgs &g, hipStream_t stream)
{
    if (!genotype_args_good(g)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_genotype_count_kernel, dim3((unsigned)g.blocks), dim3(CALLS_SITE_BLOCK), 0, stream, g);
    return hipGetLastError();
}

hipError_t launch_genotype_scan(const GenotypeArgs &g, hipStream_t stream)
{
    if (!genotype_args_good(g) || !g.scan_tmp) return hipErrorInvalidValue;
    size_t bytes = g.scan_bytes;
    return rocprim::exclusive_scan(g.scan_tmp, bytes, g.block_count, g.block_start, (int64_t)0, (size_t)(g.blocks + 1), rocprim::plus<int64_t>(), stream);
}

hipError_t launch_genotype_write(const GenotypeArgs &g, hipStream_t stream)
{
    if (!genotype_args_good(g)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sw_genotype_write_kernel, dim3((unsigned)g.blocks), dim3(CALLS_SITE_BLOCK), 0, stream, g);
    return hipGetLastError();
}

} // namespace mgl_sw_dev
