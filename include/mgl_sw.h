/*
 * mgl_sw.h -- C ABI of libmgl_sw_hip.so, the MI355X (gfx950) implementation of
 * mgl's Smith-Waterman affine-gap alignment core.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ or framework
 * types.  Every entry point names the reference interface it stands in for
 * (paths relative to /root/reference/src/main/native/mgl_sw/).  Results are
 * bit-exact with the reference CPU path (score, CIGAR, offset, traceback).
 *
 * Error convention (the reference has none -- it never checks anything,
 * SURVEY.md 8b): every function returns an mgl_sw_status; 0 is success.
 * There is NO CPU fallback inside this library: without a usable HIP device
 * every compute entry point returns MGL_SW_ERR_DEVICE.
 *
 * Threading: like the reference's alignNative (stateless, re-entrant,
 * ..._MicrosoftSmithWaterman.cpp:44-71) every function may be called from any
 * thread.  An mgl_sw_ctx serialises the calls made on it; use one ctx per
 * host thread (or per GPU) for concurrency.  mgl_sw_align() goes through the
 * coalescing front-end (mgl_sw_set_coalescing, on by default); with that
 * switched off it uses a thread-local ctx.
 */
#ifndef MGL_SW_H
#define MGL_SW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 102 (round 5): mgl_sw_plan has its round-4 fields workspace_fixed_bytes / resident_waves UNDER A NEW NUMBER (round 4 grew the struct and
 * kept 101), mgl_sw_explain_sized and mgl_sw_ctx_check are new.  A caller built against another number must not pass its mgl_sw_plan to
 * mgl_sw_explain (the library writes sizeof(mgl_sw_plan) of ITS header): compare mgl_sw_version() with MGL_SW_VERSION at load time -- the
 * Python mirror does (mgl_amd/_lib.py) -- or call mgl_sw_explain_sized, which never writes beyond the size it is given. */
/* 103: mgl_sw_plan.diag_fold. */
/* 104: mgl_sw_local_batch_device_matrix and mgl_sw_local_hit. */
#define MGL_SW_VERSION 104

/* overhang strategies: sw_common.h:22-25 (= MicrosoftSmithWaterman.java:39-56) */
#define MGL_SW_OS_SOFTCLIP 0x01
#define MGL_SW_OS_INDEL 0x02
#define MGL_SW_OS_LEAD_ID 0x04
#define MGL_SW_OS_IGNORE 0x08

#define MGL_SW_NEG_INF (-0x40000000) /* sw_common.h:33 */

typedef enum mgl_sw_status {
    MGL_SW_OK = 0,
    MGL_SW_ERR_BAD_ARG = 1,        /* null pointer, length < 1, unknown strategy */
    MGL_SW_ERR_CIGAR_OVERFLOW = 2, /* a CIGAR did not fit; *cigar_len holds the size needed */
    MGL_SW_ERR_NOMEM = 3,          /* host or device allocation failed */
    MGL_SW_ERR_DEVICE = 4,         /* no HIP device / HIP runtime error (see mgl_sw_last_error) */
    MGL_SW_ERR_UNSUPPORTED = 5     /* geometry outside what the kernels cover (see mgl_sw_max_query_len), or scores that
                                      would leave the 32-bit range (parameters x lengths >= 2^30) */
} mgl_sw_status;

/* ScoreMax, sw_common.h:36-40: best score of the last column (mqe, row mqe_t,
 * ties -> larger row), best of last column U last row (max, max_t, max_q) and
 * seg_length = ql - max_q when a last-row cell won. */
typedef struct mgl_sw_score {
    int32_t mqe, mqe_t;
    int32_t max, max_t, max_q;
    int32_t seg_length;
} mgl_sw_score;

/* What one kernel pass cost, for bench.py's roofline (HIP events recorded on
 * the stream the kernels ran on, summed over the chunks of the last call). */
typedef struct mgl_sw_timing {
    float dp_ms;        /* sw_dp_kernel (matrix fill + traceback bits)     */
    float tb_ms;        /* sw_traceback_kernel (path walk + CIGAR text)    */
    int32_t dp_launches, tb_launches;
    int64_t cells;      /* sum tl*ql of the last call                      */
    int64_t tb_bytes;   /* traceback bytes written to HBM by the last call */
    int32_t packed16;   /* 1 when the packed-int16 fill kernel (sw_dp16_kernel) ran */
    int32_t clock_mhz;  /* profiling level 2: shader clock seen inside the fill kernel (s_memtime / s_memrealtime) */
    int32_t fill_kernel; /* which fill kernel the last chunk ran: MGL_SW_KERNEL_* */
    int32_t reserved;
} mgl_sw_timing;
#define MGL_SW_KERNEL_DP32 0      /* sw_dp_kernel: int32, 16 rows x four pairs per wave          */
#define MGL_SW_KERNEL_DP16 1      /* sw_dp16_kernel: packed int16, two pairs per lane, systolic  */
#define MGL_SW_KERNEL_DP32_64 2   /* sw_dp64_kernel: int32, 64 rows, one pair per wave           */
#define MGL_SW_KERNEL_COOP 3      /* sw_dp_coop_kernel: one pair per workgroup (long reads)      */
#define MGL_SW_KERNEL_LANE16 4    /* sw_dp16_lane_kernel: packed int16, two pairs per LANE       */
#define MGL_SW_KERNEL_COOP16 5    /* sw_dp_coop16_kernel: long reads, packed int16, 128 rows/wave */
#define MGL_SW_KERNEL_STRIP16 6   /* sw_dp16_strip_kernel: long reads, one 32-row strip per lane-half */
#define MGL_SW_KERNEL_LANE16_CK 7 /* sw_dp16_lane_ck_kernel: the lane kernel, checkpoints instead of stored flags */
#define MGL_SW_KERNEL_SMALL 8     /* sw_small_kernel: small batches, one wave per pair, scores kept in LDS, fill + walk in one launch */
#define MGL_SW_KERNEL_LANE16_MATRIX 9 /* sw_dp16_lane_matrix_kernel: substitution matrix, two pairs per lane, tiles that share their target */
#define MGL_SW_KERNEL_LOCAL_LANE 10 /* sw_local_lane_kernel: local score pass, two pairs per lane, tiles that share their target */
#define MGL_SW_KERNEL_LOCAL 11 /* sw_local_pair_kernel: local alignment, one wave per pair, int32, ends + begin + CIGAR */
#define MGL_SW_KERNEL_BANDED 12 /* sw_banded_kernel: the GATK function over a diagonal band, one wave per pair, int32 */
#define MGL_SW_KERNEL_EXTEND (MGL_SW_KERNEL_BANDED + 1) /* 13, sw_extend_kernel: anchored extension with Z-drop over a centred band, one wave per pair, int32 */
#define MGL_SW_KERNEL_EXTEND_ADAPTIVE (MGL_SW_KERNEL_BANDED + 2) /* 14, sw_extend_adaptive_kernel: the same with the band re-centred every 64 rows (MGL_SW_FLAG_EXTEND_ADAPTIVE_BAND) */

/* What the library WOULD do with a batch: the planner's decisions, without running anything (mgl_sw_explain). */
typedef struct mgl_sw_plan {
    int32_t fill_kernel;        /* MGL_SW_KERNEL_*: the kernel of a uniform batch, or of the bulk of a sorted mixed one */
    int32_t precision_bits;     /* 16 (packed int16 behind the range guard) or 32 */
    int32_t rows;               /* target rows per stripe / strip of that kernel */
    int32_t waves_per_block;
    int32_t waves_per_pair;     /* long-read kernels: waves that share one pair; else 0 */
    int32_t traceback;          /* 0 = four flags per cell stored in HBM, 1 = none stored (checkpoints; the walk recomputes), 2 = score only */
    int32_t fused_walk;         /* 1 = every lane walks its own paths inside the fill kernel, 0 = traceback kernel on an auxiliary stream */
    int32_t sorted_by_library;  /* mixed geometries: 0 = not sorted (int32 kernel), 1 = counting sort on the device, 2 = on the host */
    int32_t fill_streams;       /* 1, or 2 when consecutive chunks alternate between two streams (host entries, lane kernel) */
    int32_t workspace_halves;   /* 1, or 2 when chunk k's walk overlaps chunk k+1's fill */
    int64_t chunk_pairs;        /* pairs per launch */
    int64_t chunks;             /* launches of the fill kernel for this batch */
    int64_t workspace_bytes_per_pair;
    int64_t workspace_bytes;    /* of the context's workspace that this batch would use (per-pair bytes of a chunk + the fixed part, per half) */
    int64_t workspace_fixed_bytes; /* of those, the part that does not grow with the batch: the regions of sw_dp16_lane_ck_kernel's persistent grid, one per wave slot */
    int64_t resident_waves;     /* wave slots of that grid (0: the kernel is launched one wave or workgroup per unit of work) */
    int32_t diag_fold;          /* the checkpointed lane kernel and the long-read strip kernel without stored flags: K of their folded diagonal
                                   (one multiply-add forms H + match / mismatch + 2 gext in their base-code form), 0 = none for these parameters */
} mgl_sw_plan;

typedef struct mgl_sw_ctx mgl_sw_ctx; /* opaque: one GPU, its workspace and stream */

int mgl_sw_version(void);
const char *mgl_sw_strerror(int status);
/* number of HIP devices visible (0 when there is none or no runtime) */
int mgl_sw_device_count(void);
/* longest query accepted (2^24; the matrix must also stay below 2^34 cells) */
int mgl_sw_max_query_len(void);
/* longest query whose stripe carry fits LDS with one wave per pair; longer ones run one pair per workgroup
 * (sw_dp_coop.hip), the waves handing the carry on through small LDS rings */
int mgl_sw_max_lds_query_len(void);

int mgl_sw_ctx_create(int device, mgl_sw_ctx **out);
void mgl_sw_ctx_destroy(mgl_sw_ctx *ctx);
/* text of the last HIP / argument error seen on this ctx ("" if none) */
const char *mgl_sw_last_error(const mgl_sw_ctx *ctx);
/* cap on the device traceback workspace (bytes); default: a quarter of the device's memory (72 GB on an
 * MI355X), at least 4 GiB; memory is only reserved as batches need it.  Batches are processed in chunks that fit. */
int mgl_sw_ctx_set_workspace(mgl_sw_ctx *ctx, int64_t bytes);
/* fill-kernel arithmetic: 0 (default) = per batch, the packed-int16 kernel when every pair has
 * the same tl and ql and the score range fits 16 bits, else int32; long reads: the 16-bit one-pair-per-workgroup
 * kernel, which checks its own score window and redoes a pair in 32 bits if it must, when the scoring parameters make
 * that worthwhile; 32 = always int32; 16 = like 0, but the long-read kernel is tried whenever its constants fit at
 * all (tests of the fall-back).  Results are bit-identical either way. */
int mgl_sw_ctx_set_precision(mgl_sw_ctx *ctx, int bits);
/* where the int32 fill kernel keeps its stripe carry: 0 (default) = LDS whenever the query fits, 1 = always the
 * HBM scratch used for long queries (for tests; results are identical) */
int mgl_sw_ctx_set_carry_memory(mgl_sw_ctx *ctx, int mode);
/* target rows per stripe (= lanes per pair) of the int32 fill kernel: 0 (default) = 16 (four pairs per wave) for
 * queries below 1024 bases, 64 (one pair per wave) from there on; 16 / 64 force one (tests; identical results) */
int mgl_sw_ctx_set_stripe_rows(mgl_sw_ctx *ctx, int rows);
/* long reads: one pair per workgroup, its waves pipelined over the pair's 64-row stripes (sw_dp_coop.hip).
 * 0 (default) = taken when the query is too long for the one-wave-per-pair LDS carve (see
 * mgl_sw_max_lds_query_len); 1 = never; 2..16 = always, with that many waves per pair (tests; identical
 * results) */
int mgl_sw_ctx_set_cooperative(mgl_sw_ctx *ctx, int mode);
/* queries of 1 024 bases and more (targets of any length: beyond 16 384 rows in several passes): one pair per workgroup, every lane-half a strip of 17 .. 32
 * target rows kept in registers (sw_dp16_strip.hip), per-strip 16-bit baselines.  0 (default) = taken for such batches when the
 * scoring parameters fit its static 16-bit window and enough of its strip slots would be busy; 1 = never; 2 = whenever
 * eligible, whatever the lengths (tests; identical results) */
int mgl_sw_ctx_set_strip_kernel(mgl_sw_ctx *ctx, int mode);
/* uniform batches whose scores fit 16 bits: which packed kernel runs.  0 (default) = by launch size: from 262 144 pairs on
 * the two-pairs-per-LANE kernel (sw_dp16_lane.hip: 128 pairs per wave, nothing shared between lanes), below that the
 * two-pairs-per-lane-of-a-16-lane-group kernel (sw_dp16.hip: eight pairs per wave); 1 = never the lane kernel;
 * 2 = the lane kernel whenever the batch is eligible (tests; results are identical) */
int mgl_sw_ctx_set_lane_kernel(mgl_sw_ctx *ctx, int mode);
/* the lane kernel stores no traceback by default (sw_dp16_lane_ck.hip): its fill keeps the carry row leaving every 16 target rows and
 * the lanes' state every 32 query columns, and the path walk recomputes the 16 x 32 blocks it crosses (same flags, same results, about
 * a fifth of the matrix twice instead of eight flag instructions for every cell).  0 (default) = that form whenever the lane kernel
 * runs with 32-row strips and writes CIGARs, and for the geometries of a batch of mixed lengths that fill whole waves of 128 pairs
 * (chunks sorted by geometry, from two rounds of the chip on); 1 = never (the flags of every cell are stored: needed before
 * mgl_sw_ctx_expand_slot); 2 = same as 0 (tests) */
int mgl_sw_ctx_set_lane_checkpoint(mgl_sw_ctx *ctx, int mode);
/* small batches are latency bound: up to MGL_SW_SMALL_BATCH_PAIRS pairs (MGL_SW_SMALL_BATCH_PAIRS_MIXED without a promise of one geometry:
 * measured crossovers, scripts/small_batch_probe.py) whose targets have at most 512 rows and whose matrix of kept
 * scores fits a workgroup's LDS (256 x 150, 400 x 190, ...) run one wave per pair in ONE launch that fills, walks and writes the text
 * (sw_small.hip; nothing of the workspace is touched).  0 (default) = those batches, on a context none of whose other kernel
 * choices has been forced; 1 = never; 2 = every batch whose bounds allow it, whatever its size and the other settings (the
 * coalescing front-end of mgl_sw_align) */
int mgl_sw_ctx_set_small_kernel(mgl_sw_ctx *ctx, int mode);
#define MGL_SW_SMALL_BATCH_PAIRS 5120
#define MGL_SW_SMALL_BATCH_PAIRS_MIXED 8192
/* 1 = HIP events around every kernel launch of a call, on the streams the kernels run on, read back by
 * mgl_sw_ctx_get_timing (the call itself stays asynchronous); 2 = additionally stamp the shader clock
 * inside the fill kernel (diagnostic; a few extra instructions per workgroup); 3 = as 1, summed over every call until
 * mgl_sw_ctx_get_timing reads and clears it (dp_ms / dp_launches = the mean launch duration over a timed loop); 0 = off */
int mgl_sw_ctx_set_profiling(mgl_sw_ctx *ctx, int enable);
/* The plan for a batch of n pairs up to max_tl x max_ql with these parameters, as the entry named by `entry` would run it on this
 * context (its workspace limit and forced modes included) -- nothing is launched, allocated or copied.  flags: MGL_SW_FLAG_*;
 * packed2: the sequences are 2-bit packed; entry: 0 = device-resident (mgl_sw_align_batch_device*), 1 = host buffers
 * (mgl_sw_align_batch / _status / _2bit).  ctx may be NULL: a default context on a 256-CU device (what the CPU tests pin), with
 * workspace_limit bytes of workspace (0: the default, or the context's own limit when ctx is given).  Planned with a CIGAR stride of
 * 64 bytes (the only decision the stride enters is whether a small batch's text fits the one-wave-per-pair kernel's LDS: a call with
 * a much larger stride may leave that kernel where this plan names it).  Returns the status the call itself would return from its
 * planning (MGL_SW_ERR_UNSUPPORTED, ...). */
int mgl_sw_explain(mgl_sw_ctx *ctx, int64_t workspace_limit, int64_t n, int max_tl, int max_ql, int match, int mismatch, int gopen,
                   int gext, int strategy, int flags, int packed2, int entry, mgl_sw_plan *out);
/* ... the same for a caller whose mgl_sw_plan may be older or newer than the library's: at most out_size bytes of *out are written (the
 * struct only ever grows at its end), and what the library does not know of a larger struct is zeroed. */
int mgl_sw_explain_sized(mgl_sw_ctx *ctx, int64_t workspace_limit, int64_t n, int max_tl, int max_ql, int match, int mismatch, int gopen,
                         int gext, int strategy, int flags, int packed2, int entry, mgl_sw_plan *out, size_t out_size);
int mgl_sw_ctx_get_timing(mgl_sw_ctx *ctx, mgl_sw_timing *out); /* waits for the last call's kernels */
/* What a kernel found out about itself AFTER the call that enqueued it returned (the device entries do not wait for their kernels):
 * today, a persistent grid of sw_dp16_lane_ck_kernel that drew a tile number no launch of its size can draw -- its counter did not
 * stand at zero, tiles may be undone.  Synchronise the stream, then ask: MGL_SW_OK, or MGL_SW_ERR_DEVICE (sticky: every later call on
 * the context reports it too; destroy the context).  The host entries ask by themselves before they return.  Waits for nothing. */
int mgl_sw_ctx_check(mgl_sw_ctx *ctx);

/* Sign normalisation of the JNI boundary
 * (..._MicrosoftSmithWaterman.cpp:51-55): match > 0, mismatch < 0, open > 0,
 * ext > 0 whatever signs the caller used.  All align entry points apply it. */
void mgl_sw_normalize_params(int *match, int *mismatch, int *gopen, int *gext);

/*
 * One pair.  Replaces align_avx (sw_avx.h:6) / align_scalar (sw_scalar.h:9)
 * and the body of alignNative (..._MicrosoftSmithWaterman.cpp:44-71):
 * cigar receives *cigar_len ASCII bytes, no terminator (like cigar.copy(),
 * .cpp:65); *offset is the alignment offset they return; *ez (optional) the
 * ScoreMax the reference keeps local (sw_avx.cpp:9).
 */
int mgl_sw_align(const char *t, int tl, const char *q, int ql, int match, int mismatch, int gopen,
                 int gext, int strategy, char *cigar, int cigar_cap, int *cigar_len, int *offset,
                 mgl_sw_score *ez);

/*
 * Coalescing of concurrent one-pair calls (the way GATK drives alignNative: many threads, one pair each,
 * MicrosoftSmithWaterman.java:66-86).  Every mgl_sw_align call (hence the JNI export) is parked and merged
 * with the calls of other threads that use the same parameters and strategy into one device batch, flushed
 * when as many calls are waiting as the previous batch held (a lone caller never waits), when max_batch are,
 * or when the oldest has waited max_wait_us.  Results are exactly those of the direct call.  ON by default
 * (max_batch 4096, max_wait_us 50; environment: MGL_SW_COALESCE_US, -1 = off, and MGL_SW_COALESCE_BATCH);
 * max_batch = 0 switches it off: every call is then its own device round trip on the calling thread's context.
 */
int mgl_sw_set_coalescing(int max_batch, int max_wait_us);
/* device batches flushed / pairs served by the coalescer so far */
int mgl_sw_coalescing_stats(int64_t *batches, int64_t *pairs);
/*
 * ... and in front of the coalescer, for pairs of the size GATK sends (targets up to 512 bases, queries up to 2 048, the matrix of
 * scores within a workgroup's LDS: 256 x 150, 400 x 190, ...): every calling thread leases a MAILBOX -- its request half in device
 * memory the host stores into over the large BAR where the platform has one (MGL_SW_SERVICE_BAR=0: never), else in pinned host
 * memory; its reply half in pinned host memory -- and one resident wave that serves it (sw_service.hip).  A call writes its pair into the mailbox and spins until the wave hands the
 * result back: no kernel launch, no stream synchronisation and no other thread on the request path (this replaces the
 * launch-per-call of ..._MicrosoftSmithWaterman.cpp:44-71's callers).  A wave ends by itself when its mailbox has been quiet for
 * idle_us (default 1 000; environment MGL_SW_SERVICE_IDLE_US) or after MGL_SW_SERVICE_LIFE_MS (default 20) -- a resident
 * kernel holds up device-wide synchronisation for that long at most -- and the next call launches it again.  `slots` mailboxes at
 * most (default 64, environment MGL_SW_SERVICE_SLOTS, at most 128, and never more than half the device's CUs: a mailbox's wave holds
 * its carve of LDS -- 64 KB, the full 160 KB only once a pair has needed it -- for as long as the grid lives); threads beyond that,
 * pairs that do not fit, and any call whose wave does not answer within 20 s (the service is switched off from then on) take the
 * coalescer.  slots = 0 switches the service off; idle_us = 0 keeps the current value.  Follows mgl_sw_set_coalescing: with
 * coalescing off every call is a direct call.
 */
int mgl_sw_set_service(int slots, int idle_us);
/* calls served through mailboxes / launches of the service kernel so far */
int mgl_sw_service_stats(int64_t *calls, int64_t *launches);

/*
 * Batch, host buffers.  Pair k is targets[t_off[k] .. t_off[k+1]) against
 * queries[q_off[k] .. q_off[k+1]) (raw bytes, compared for equality exactly
 * as sw.cpp:55).  One parameter set and strategy per batch.  cigar_out is
 * n * cigar_stride bytes; each pair's slot is zero padded (the contract of
 * the Java side's zero-filled direct buffer, MicrosoftSmithWaterman.java:71-85).
 * score_out and cigar_len_out may be NULL.
 */
int mgl_sw_align_batch(mgl_sw_ctx *ctx, int64_t n, const uint8_t *targets, const int64_t *t_off,
                       const uint8_t *queries, const int64_t *q_off, int match, int mismatch,
                       int gopen, int gext, int strategy, int32_t *offset_out,
                       mgl_sw_score *score_out, char *cigar_out, int cigar_stride,
                       int32_t *cigar_len_out);

/*
 * The same with a per-pair status array (int32[n], mgl_sw_status values): with status_out non-NULL a CIGAR that
 * does not fit its slot -- or a device-side failure of one pair -- is reported there and does not fail the call
 * (*cigar_len_out still receives the size needed).  status_out == NULL is exactly mgl_sw_align_batch.
 */
int mgl_sw_align_batch_status(mgl_sw_ctx *ctx, int64_t n, const uint8_t *targets, const int64_t *t_off,
                              const uint8_t *queries, const int64_t *q_off, int match, int mismatch,
                              int gopen, int gext, int strategy, int32_t *offset_out,
                              mgl_sw_score *score_out, char *cigar_out, int cigar_stride,
                              int32_t *cigar_len_out, int32_t *status_out);

/*
 * Several GPUs from ONE process ("single process, one host thread per device").  Pairs are independent
 * -- alignNative holds no state, ..._MicrosoftSmithWaterman.cpp:44-71 -- so mgl_sw_align_batch_multi cuts the host
 * batch into contiguous shards, one per device of the set, balanced by the DP cells (sum tl * ql) they hold, and runs
 * every shard through mgl_sw_align_batch_status on that device's own context from its own host thread.  Results are
 * written straight into the caller's arrays (shards are disjoint slices); no inter-GPU traffic.  Arguments and error
 * behaviour are those of mgl_sw_align_batch_status.  `devices` = n_devices HIP ordinals (NULL: 0 .. n_devices-1; an
 * ordinal may be listed more than once -- each entry gets its own context and host thread).
 */
typedef struct mgl_sw_multi mgl_sw_multi;
int mgl_sw_multi_create(int n_devices, const int *devices, mgl_sw_multi **out);
void mgl_sw_multi_destroy(mgl_sw_multi *m);
int mgl_sw_multi_device_count(const mgl_sw_multi *m);
/* the context of entry `index` (to tune it with the mgl_sw_ctx_set_* calls); owned by the set */
mgl_sw_ctx *mgl_sw_multi_ctx(mgl_sw_multi *m, int index);
int mgl_sw_multi_set_workspace(mgl_sw_multi *m, int64_t bytes_per_device);
const char *mgl_sw_multi_last_error(const mgl_sw_multi *m);
int mgl_sw_align_batch_multi(mgl_sw_multi *m, int64_t n, const uint8_t *targets, const int64_t *t_off,
                             const uint8_t *queries, const int64_t *q_off, int match, int mismatch,
                             int gopen, int gext, int strategy, int32_t *offset_out,
                             mgl_sw_score *score_out, char *cigar_out, int cigar_stride,
                             int32_t *cigar_len_out, int32_t *status_out);
/* first pair of every shard of the last mgl_sw_align_batch_multi call: first_out[0 .. n_devices] */
int mgl_sw_multi_last_shards(mgl_sw_multi *m, int64_t *first_out);
/* The sharding rule by itself (host only, no device needed): contiguous parts of pairs 0 .. n-1 with equal shares of
 * sum tl * ql, every boundary a multiple of `align` pairs; first_out[0 .. parts], first_out[parts] == n. */
int mgl_sw_shard_by_cells(int64_t n, const int64_t *t_off, const int64_t *q_off, int parts, int64_t align,
                          int64_t *first_out);

/*
 * Batch, device-resident: every pointer is a device pointer on ctx's GPU and
 * the work is enqueued on `stream` (a hipStream_t; NULL = the null stream)
 * without synchronising -- unless profiling is enabled.  max_tl / max_ql are
 * upper bounds of the pair lengths (they size the workspace).  status_out
 * (optional, int32[n]) receives a per-pair mgl_sw_status (0 or
 * MGL_SW_ERR_CIGAR_OVERFLOW).  flags: MGL_SW_FLAG_UNIFORM_GEOMETRY promises that every
 * pair has exactly tl == max_tl and ql == max_ql (enables the packed-int16 fill kernels; the
 * host-buffer entry detects this by itself).  Without a promise a batch of 1024 pairs or more whose
 * (max_tl, max_ql) grid has at most 2^20 cells is sorted by geometry on the device, chunk by chunk
 * (counting sort, sw_regroup_*_kernel): blocks of eight pairs of one geometry go through the packed
 * kernel, the few left over through the int32 kernel, every result lands at its pair's own index.  The
 * host reads one word per chunk back to size those launches, so such a call waits for the sorts (not for
 * the alignments) before it returns; MGL_SW_AUTO_GROUP=0 in the environment keeps the int32 kernel.
 */
#define MGL_SW_FLAG_UNIFORM_GEOMETRY 0x1
/* MGL_SW_FLAG_BINARY_CIGAR: the CIGAR slot receives BAM-style little-endian uint32 elements
 * (length << 4 | op, op M=0 I=1 D=2 S=4) instead of the text of sw.cpp:251-252; cigar_len is then in bytes
 * (4 per element) and cigar_stride should be a multiple of 4.  Same elements, same order. */
#define MGL_SW_FLAG_BINARY_CIGAR 0x2
/* MGL_SW_FLAG_GROUPED_GEOMETRY: a promise that every aligned block of eight consecutive pairs (pairs 8k .. 8k+7;
 * the last block may be shorter) has one (tl, ql) -- e.g. a batch of variable-length reads sorted by length and
 * padded per length to a multiple of eight.  Such a batch is eligible for the packed-int16 kernel like a uniform
 * one (each wave of that kernel works on one block).  Results are undefined if the promise is broken. */
#define MGL_SW_FLAG_GROUPED_GEOMETRY 0x4
/* MGL_SW_FLAG_SCORE_ONLY: the caller only wants d_score_out (all six ScoreMax fields, bit-identical to the full
 * call).  A hint: batches that run on the packed-int16 kernel then skip the traceback flags and the path walk
 * (offsets are written as 0, cigar_len as 0, the CIGAR slots are left untouched); every other batch runs the full
 * path.  Not a reference feature (align_* always builds the CIGAR): a pre-filter mode for database searches. */
#define MGL_SW_FLAG_SCORE_ONLY 0x8
/* MGL_SW_FLAG_SHARED_TARGET (mgl_sw_align_batch_device_matrix only; ignored elsewhere): a promise that every aligned block of 128
 * consecutive pairs (pairs 128k .. 128k+127; the last block may be shorter) shares ONE target -- the same d_t_off and d_t_len -- and
 * one query length: a database search laid out database sequence by database sequence.  Such a batch runs on a kernel that gives every
 * lane two pairs and looks the scores of a column up as one row of a per-strip profile (sw_dp16_lane_matrix.hip); gap penalties and
 * matrix must satisfy 0 <= S + gopen + gext <= 255 for every entry and the score range 16 bits, else the flag is read as
 * MGL_SW_FLAG_GROUPED_GEOMETRY.  A block that breaks the promise is NOT computed: its pairs get MGL_SW_ERR_BAD_ARG in d_status_out.
 * With d_status_out == NULL nothing could report such a block, so the flag is ignored and does not imply the grouped promise either:
 * without other flags the batch runs as one of mixed geometries on the int32 kernel, every pair computed whatever the layout.
 * The call looks at every block's lengths before it launches (8 bytes per block back to the host: it waits for `stream` once) and sizes its
 * workspace by the largest blocks; the blocks may come in any order.
 * Combines with MGL_SW_FLAG_SCORE_ONLY (needs d_score_out) and MGL_SW_FLAG_BINARY_CIGAR. */
#define MGL_SW_FLAG_SHARED_TARGET 0x10
/* MGL_SW_FLAG_EXTEND_TO_QUERY_END (mgl_sw_extend_batch_device only; ignored elsewhere): the CIGAR describes the path to
 * (t_end_qend, ql), the best cell of the query's last column, wherever there is one; see there. */
#define MGL_SW_FLAG_EXTEND_TO_QUERY_END 0x20
/* MGL_SW_FLAG_EXTEND_ADAPTIVE_BAND (mgl_sw_extend_batch_device only; ignored elsewhere): the band follows the alignment -- it is
 * re-centred every MGL_SW_EXTEND_RECENTRE_ROWS target rows on the diagonal of the row maximum; see there.  The number of rows is part
 * of the function's definition (the outputs depend on it), not an implementation detail. */
#define MGL_SW_FLAG_EXTEND_ADAPTIVE_BAND 0x40
#define MGL_SW_EXTEND_RECENTRE_ROWS 64
int mgl_sw_align_batch_device(mgl_sw_ctx *ctx, void *stream, int64_t n, const uint8_t *d_targets,
                              const int64_t *d_t_off, const uint8_t *d_queries,
                              const int64_t *d_q_off, int max_tl, int max_ql, int match,
                              int mismatch, int gopen, int gext, int strategy,
                              int32_t *d_offset_out, mgl_sw_score *d_score_out, char *d_cigar_out,
                              int cigar_stride, int32_t *d_cigar_len_out, int32_t *d_status_out,
                              int flags);

/*
 * Batch, device-resident, 2-bit packed bases -- the wire format for ACGT data instead of the
 * ASCII-in-ByteBuffer of MicrosoftSmithWaterman.java:73-75.  d_target_bases / d_query_bases hold four bases per
 * byte, base k of an array in bits 2*(k%4) of byte k/4 (A=0 C=1 G=2 T=3 by convention; the kernels only test
 * equality, exactly like sw.cpp:55 does on bytes).  Pair p is the d_t_len[p] bases starting at BASE index
 * d_t_start[p] against the d_q_len[p] bases starting at d_q_start[p] -- target windows may overlap, e.g. windows
 * into one packed genome.  With MGL_SW_FLAG_UNIFORM_GEOMETRY the length arrays may be NULL (every pair max_tl x
 * max_ql).  Everything else as mgl_sw_align_batch_device; results equal those of the ASCII entries on the
 * unpacked sequences.
 */
int mgl_sw_align_batch_device_2bit(mgl_sw_ctx *ctx, void *stream, int64_t n, const uint8_t *d_target_bases,
                                   const int64_t *d_t_start, const int32_t *d_t_len,
                                   const uint8_t *d_query_bases, const int64_t *d_q_start,
                                   const int32_t *d_q_len, int max_tl, int max_ql, int match, int mismatch,
                                   int gopen, int gext, int strategy, int32_t *d_offset_out,
                                   mgl_sw_score *d_score_out, char *d_cigar_out, int cigar_stride,
                                   int32_t *d_cigar_len_out, int32_t *d_status_out, int flags);

/*
 * The same wire format from HOST memory (replaces the ASCII-in-ByteBuffer contract of MicrosoftSmithWaterman.java:73-75 for callers
 * that hold packed bases): target_base_count / query_base_count are the numbers of bases the two packed arrays hold.  The packed
 * arrays travel chunk by chunk beside the kernels when the pairs' start positions ascend (reads packed back to back), or whole
 * before the first chunk (windows into one genome, in any order); results leave as in mgl_sw_align_batch_status (status_out may
 * be NULL: then a CIGAR that does not fit fails the call).  Everything else as mgl_sw_align_batch_device_2bit.
 */
int mgl_sw_align_batch_2bit(mgl_sw_ctx *ctx, int64_t n, const uint8_t *target_bases, int64_t target_base_count,
                            const int64_t *t_start, const int32_t *t_len, const uint8_t *query_bases,
                            int64_t query_base_count, const int64_t *q_start, const int32_t *q_len, int max_tl, int max_ql,
                            int match, int mismatch, int gopen, int gext, int strategy, int32_t *offset_out,
                            mgl_sw_score *score_out, char *cigar_out, int cigar_stride, int32_t *cigar_len_out,
                            int32_t *status_out, int flags);

/*
 * Page-lock arrays the caller passes to the host-buffer entries (mgl_sw_align_batch, _status, _2bit) again and again --
 * hipHostRegister: the direct ByteBuffers of a JVM are a natural fit.  Copies from registered input arrays are asynchronous DMA
 * (the entry no longer blocks inside pageable copies), and when EVERY output array of a call lies in registered memory the
 * results are copied straight into it instead of through the context's own pinned ring.  Registration costs milliseconds per
 * gigabyte: do it once, not per call.  Unregister before freeing the memory (waits for the context's copies to finish).
 */
int mgl_sw_register_host_buffer(mgl_sw_ctx *ctx, void *ptr, size_t bytes);
int mgl_sw_unregister_host_buffer(mgl_sw_ctx *ctx, void *ptr);

/*
 * ASCII bases addressed by (start, length) per pair instead of consecutive offsets: pair k =
 * d_targets[d_t_start[k] .. + d_t_len[k]) against d_queries[d_q_start[k] .. + d_q_len[k]).  Sequences may be shared
 * or reordered without moving bytes (e.g. to satisfy MGL_SW_FLAG_GROUPED_GEOMETRY by sorting index arrays).
 * Everything else as mgl_sw_align_batch_device; outputs are indexed by k.
 */
int mgl_sw_align_batch_device_indexed(mgl_sw_ctx *ctx, void *stream, int64_t n, const uint8_t *d_targets,
                                      const int64_t *d_t_start, const int32_t *d_t_len, const uint8_t *d_queries,
                                      const int64_t *d_q_start, const int32_t *d_q_len, int max_tl, int max_ql,
                                      int match, int mismatch, int gopen, int gext, int strategy,
                                      int32_t *d_offset_out, mgl_sw_score *d_score_out, char *d_cigar_out,
                                      int cigar_stride, int32_t *d_cigar_len_out, int32_t *d_status_out, int flags);

/*
 * Substitution-matrix scoring ("protein" mode).  NOT in the reference, which scores
 * by byte equality only (sw.cpp:55): the same recurrence, overhang strategies and traceback with
 *     diag = H[i-1][j-1] + matrix[code[t[i-1]] * 32 + code[q[j-1]]]
 * code: 256 bytes -> 0..31, matrix: 32 x 32 int8 (both HOST pointers, copied per call); gopen / gext as in the
 * other entries.  d_t_len / d_q_len (optional, int32 per pair): with them d_t_off[k] / d_q_off[k] are per-pair START
 * positions, so one database sequence can serve many pairs; NULL = pair k is [off[k], off[k+1]).  Uniform / grouped batches (flags) whose score range fits 16 bits
 * take the packed kernel, all others the int32 kernel; queries up to about 3 300 residues (MGL_SW_ERR_UNSUPPORTED
 * beyond), targets any length.  No parity claim exists for this mode: it is validated against the CPU restatement's own extension and
 * an independent textbook DP (tests/test_gpu_matrix.py).
 */
int mgl_sw_align_batch_device_matrix(mgl_sw_ctx *ctx, void *stream, int64_t n, const uint8_t *d_targets,
                                     const int64_t *d_t_off, const int32_t *d_t_len, const uint8_t *d_queries,
                                     const int64_t *d_q_off, const int32_t *d_q_len, int max_tl, int max_ql,
                                     const int8_t *matrix, const uint8_t *code, int gopen,
                                     int gext, int strategy, int32_t *d_offset_out, mgl_sw_score *d_score_out,
                                     char *d_cigar_out, int cigar_stride, int32_t *d_cigar_len_out,
                                     int32_t *d_status_out, int flags);

/*
 * LOCAL Smith-Waterman with a substitution matrix (NOT a reference function, and NOT the GATK function of the entries above): the score
 * of a protein or DNA database search, as SSEARCH, SWIPE or BWA's ksw compute it.  For i = 1..tl, j = 1..ql, s = matrix[code[t[i-1]]]
 * [code[q[j-1]]] (row = target code, as mgl_sw_align_batch_device_matrix):
 *     E[i][j] = max(H[i-1][j] - o, E[i-1][j] - e)    (consumes target: 'D')
 *     F[i][j] = max(H[i][j-1] - o, F[i][j-1] - e)    (consumes query: 'I')
 *     H[i][j] = max(0, H[i-1][j-1] + s, E[i][j], F[i][j]),   H[0][*] = H[*][0] = 0, E[0][*] = F[*][0] = -inf
 * a gap of length k costs o + (k-1) e (gopen / gext normalised as in the other entries, each at most 2^24).  score = the largest H
 * (0 if there is no cell); (t_end, q_end) = the smallest (i, j) holding it, i first: half-open ends.  The path is walked back from
 * there: H == 0 stops, then the diagonal ('M'), then F, then E (DESIGN.md 2's priorities); in F / E extension wins ties.  The cell it
 * stops in is (t_begin, q_begin): the alignment is t[t_begin:t_end] against q[q_begin:q_end], its CIGAR has M / I / D only, no clips.
 * score == 0: all four coordinates 0, an empty CIGAR.  Checked against the textbook DP in tests/ (tests/local_textbook.py).
 *
 * Pair k: the d_t_len[k] bytes at d_targets + d_t_start[k] against the d_q_len[k] bytes at d_queries + d_q_start[k] (ASCII, device
 * memory; lengths at most max_tl / max_ql, else MGL_SW_ERR_BAD_ARG for that pair).  UNLIKE the GATK entries a length of 0 is valid: such a
 * pair is a hole, its hit is all zeros, its status 0, nothing is computed for it.  matrix (32 x 32 int8) and code (256 bytes -> 0..31)
 * are HOST pointers, copied per call.  The work is enqueued on `stream`; the call does not synchronise, except that
 * MGL_SW_FLAG_SHARED_TARGET on kernel A reads every tile's geometry back once (8 bytes per tile) to order the tiles.
 * mgl_sw_ctx_get_timing's fill_kernel names the kernel that ran: MGL_SW_KERNEL_LOCAL_LANE (kernel A) or MGL_SW_KERNEL_LOCAL (kernel B).
 * flags:
 *   MGL_SW_FLAG_SCORE_ONLY: only d_hit_out[k].score is defined (the other four fields are written as 0); d_cigar_out and
 *     d_cigar_len_out may be NULL.
 *   MGL_SW_FLAG_SHARED_TARGET: a promise that every aligned block of 128 pairs has ONE target (same start, same length); query lengths
 *     may differ inside a block.  With MGL_SW_FLAG_SCORE_ONLY, a status array and a batch inside the packed kernel's range guard
 *     (sw_local.h local_lane_ok(): 16-bit scores, S - min(S) a byte, the target in LDS) the scores come from a kernel that gives every
 *     lane two pairs (sw_local_lane.hip); a block that breaks the promise then gets MGL_SW_ERR_BAD_ARG in d_status_out and nothing else
 *     written.  Everything else runs the general kernel (one wave per pair, int32, sw_local.hip), whatever the layout.
 *   MGL_SW_FLAG_BINARY_CIGAR: BAM-style uint32 elements (len << 4 | op, M=0 I=1 D=2), cigar_len in bytes.
 * d_status_out (optional, int32 per pair): 0, MGL_SW_ERR_CIGAR_OVERFLOW (d_cigar_len_out then holds the size needed; the hit is
 * complete), MGL_SW_ERR_UNSUPPORTED (a pair too large for the workspace, or scores beyond 2^29), MGL_SW_ERR_BAD_ARG (see above).
 * A pair that the general kernel gives MGL_SW_ERR_UNSUPPORTED or MGL_SW_ERR_BAD_ARG gets a hit of all zeros and a cigar_len of 0, and
 * no byte of its CIGAR row is written; nor is any byte of a row at or beyond that pair's cigar_len, whatever its status.
 * The call fails only on bad arguments (n < 0, a null matrix / code / sequence / hit array, a code >= 32, without
 * MGL_SW_FLAG_SCORE_ONLY a null CIGAR array or a stride below 2 -- 4 for binary) and device errors: MGL_SW_ERR_DEVICE without a GPU.
 */
typedef struct mgl_sw_local_hit {
    int32_t score, t_begin, t_end, q_begin, q_end;
} mgl_sw_local_hit;
int mgl_sw_local_batch_device_matrix(mgl_sw_ctx *ctx, void *stream, int64_t n, const uint8_t *d_targets, const int64_t *d_t_start,
                                     const int32_t *d_t_len, const uint8_t *d_queries, const int64_t *d_q_start, const int32_t *d_q_len,
                                     int max_tl, int max_ql, const int8_t *matrix, const uint8_t *code, int gopen, int gext,
                                     mgl_sw_local_hit *d_hit_out, char *d_cigar_out, int cigar_stride, int32_t *d_cigar_len_out,
                                     int32_t *d_status_out, int flags);

/*
 * BANDED alignment (NOT a reference function: the reference has no band; opt-in, for long reads whose path stays near the main
 * diagonal).  The function of mgl_sw_align_batch_device_indexed -- same inputs, parameters, overhang strategies and outputs -- computed
 * over the cells of a diagonal band only.  For a pair of lengths tl, ql and the call's `band` >= 0 let
 *     lo = min(0, ql - tl) - band,   hi = max(0, ql - tl) + band;
 * a cell (i, j), 0 <= i <= tl, 0 <= j <= ql, border row and column included, is in the band iff lo <= j - i <= hi (so (0, 0) and
 * (tl, ql) always are).  Only in-band interior cells are computed; any value read from an out-of-band cell (H, E entering from above,
 * F entering from the left) is minus infinity: it loses every comparison strictly, stays minus infinity under - gext, and is replaced
 * by the open at the first in-band cell (run length 1).  The last-column scan (mqe, mqe_t) and the last-row scan (max, max_t, max_q,
 * seg_length) visit in-band cells only, in the full-matrix order with its tie rules; the walk starts where the full-matrix walk
 * starts and cannot leave the band.  Defined by tests/banded_textbook.py.  Two relations tie it to the full-matrix function:
 *   (R1) band >= max(tl, ql) covers the matrix: every output equals mgl_sw_align_batch_device_indexed's;
 *   (R2) if every cell the full-matrix walk visits is in the band, offset and CIGAR equal the full-matrix result (the six score
 *        fields need not: mqe may come from a cell whose own path leaves the band).
 * Everything is enqueued on `stream`; the call does not synchronise.  flags: MGL_SW_FLAG_BINARY_CIGAR; MGL_SW_FLAG_SCORE_ONLY
 * (d_score_out only -- it must not be NULL --, no decisions kept, d_cigar_out / d_cigar_len_out may be NULL); others are ignored.
 * The call fails before any device work with MGL_SW_ERR_BAD_ARG on n < 0, a null sequence / start / length / offset array, band < 0,
 * an unknown strategy, max_tl < 1 or max_ql < 1, and -- without MGL_SW_FLAG_SCORE_ONLY -- a null CIGAR array or a stride below 2 (4 for
 * binary); with MGL_SW_ERR_DEVICE without a GPU.
 * d_status_out (optional, int32 per pair): 0; MGL_SW_ERR_BAD_ARG for a length below 1 or above max_tl / max_ql;
 * MGL_SW_ERR_CIGAR_OVERFLOW (d_cigar_len_out holds the size needed, the scores are complete); MGL_SW_ERR_UNSUPPORTED for a pair
 * outside the kernel's range guard or too large for one workspace slot.  The range guard (sw_banded.h banded_range_ok(), on the
 * normalised parameters): lengths at most 2^28, gopen and gext at most 2^24, and
 *     max(match, |mismatch|) * min(tl, ql) + 2 gopen + gext * max(tl, ql) <= 2^29.
 * A slot (banded_pair_bytes()) holds 8 (ql + 1) bytes, 4 (tl + ql + 4) bytes and -- four bits per swept cell --
 * 32 ceil(tl / 64) (min(ql, hi - lo + 64) + 63) bytes; the grid has up to eight waves per CU, one slot each, as far as the context's
 * workspace limit allows, and works a larger batch off inside the one launch.  The lengths are device data, so every slot is sized for
 * the LARGEST pair that max_tl, max_ql and the band admit (a pair's band widens with |ql - tl|: the worst has ql near
 * (tl + 2 band + 64) / 2), not for the pairs of the batch: max_tl = max_ql = 10 000 at band 512 reserves 27 MiB a slot -- 58 GB of the
 * (grow-only) workspace for 2 048 waves -- where a 10 000 x 10 000 pair uses 5.7 MiB.  Under a smaller workspace limit the grid has
 * fewer waves, nothing else changes.  Pass tight max_tl / max_ql.  A pair with a non-zero status gets offset 0, a
 * cigar_len of 0 (except overflow), scores of 0 (except overflow) and no byte of its CIGAR row written; nor is any byte of a row at or
 * beyond that pair's cigar_len, whatever its status.  mgl_sw_ctx_get_timing's fill_kernel: MGL_SW_KERNEL_BANDED.
 */
int mgl_sw_align_batch_device_banded(mgl_sw_ctx *ctx, void *stream, int64_t n, const uint8_t *d_targets, const int64_t *d_t_start,
                                     const int32_t *d_t_len, const uint8_t *d_queries, const int64_t *d_q_start, const int32_t *d_q_len,
                                     int max_tl, int max_ql, int match, int mismatch, int gopen, int gext, int strategy, int band,
                                     int32_t *d_offset_out, mgl_sw_score *d_score_out, char *d_cigar_out, int cigar_stride,
                                     int32_t *d_cigar_len_out, int32_t *d_status_out, int flags);

/*
 * ANCHORED EXTENSION with Z-drop (NOT a reference function; opt-in, for the extend step of a seed - chain - extend read mapper).  The
 * start is fixed at (0, 0), the end is free, and work stops once the score has fallen too far below the best seen (the Z-drop rule of
 * ksw2 / minimap2 / BWA-MEM).  Defined by tests/extend_textbook.py.  Per pair: a target of tl >= 1 and a query of ql >= 1 bytes
 * compared by equality, the parameters normalised as everywhere (a gap of k costs o + (k - 1) e); per call: band >= 0 and zdrop
 * (< 0: the rule is off).
 *   Band: a cell (i, j), border included, is in the band iff -band <= j - i <= band, whatever tl and ql are; (tl, ql) may lie outside.
 *   Borders: H(0, 0) = 0, H(0, j) = -(o + (j - 1) e), H(i, 0) = -(o + (i - 1) e) for in-band border cells.
 *   Interior: the recurrence, priorities, run lengths and minus infinity of the banded entry above -- the diagonal wins ties, then the
 *   horizontal gap; a gap opens only where strictly better than extending; a read from an out-of-band cell is minus infinity.
 *   Rows: rowmax(i) is the largest H over row i's in-band cells (the border column while i <= band, the border row for i = 0), rj(i)
 *   the smallest column holding it; best(i) the largest H over rows 0 .. i, at the smallest row, then the smallest column (best(0) is
 *   0 at (0, 0)).  A row without a cell in the band (i > ql + band) has rowmax = minus infinity.
 *   Z-drop: row i >= 1 drops iff zdrop >= 0 and
 *       best(i - 1).H - rowmax(i) > zdrop + e * |(i - best(i - 1).i) - (rj(i) - best(i - 1).j)|.
 *   rows_done = (first dropping row) - 1, or tl; rows beyond rows_done do not exist for any output.
 * mgl_sw_extension: score, t_end, q_end = best(rows_done) and its cell (score >= 0; (0, 0) is the empty extension); score_qend,
 * t_end_qend = the largest H(i, ql) over in-band rows 1 <= i <= rows_done, the later row among equals, or -0x40000000, -1 without
 * such a cell; rows_done; dropped (0 / 1); cigar_from: 0 = the CIGAR's walk started at (t_end, q_end), 1 = at (t_end_qend, ql) --
 * with MGL_SW_FLAG_EXTEND_TO_QUERY_END wherever t_end_qend >= 1.  The CIGAR is the banded walk from that cell back to (0, 0): global
 * on the prefix pair, M / I / D only, no soft clips, a walk that reaches row 0 or column 0 finishes with one I or D run; it spends
 * exactly the start cell's target and query bases and is empty (cigar_len 0) for (0, 0).
 * flags: MGL_SW_FLAG_EXTEND_TO_QUERY_END, MGL_SW_FLAG_BINARY_CIGAR, MGL_SW_FLAG_SCORE_ONLY (d_ext_out only -- cigar_from as the full call
 * gives it --, no decisions kept, d_cigar_out / d_cigar_len_out may be NULL); others are ignored.  The call fails before any device work
 * with MGL_SW_ERR_BAD_ARG on n < 0, a null sequence / start / length array, a null d_ext_out, band < 0, max_tl < 1 or max_ql < 1, and --
 * without MGL_SW_FLAG_SCORE_ONLY -- a null CIGAR array or a stride below 2 (4 for binary); with MGL_SW_ERR_DEVICE without a GPU.
 * d_status_out (optional): the banded entry's statuses -- MGL_SW_ERR_BAD_ARG for a length below 1 or above max_tl / max_ql,
 * MGL_SW_ERR_UNSUPPORTED outside the banded range guard or too large for one workspace slot, MGL_SW_ERR_CIGAR_OVERFLOW.  A pair with a
 * non-zero status gets an all-zero record, a cigar_len of 0 and no byte of its CIGAR row written; nor is any byte of a row at or beyond
 * that pair's cigar_len.  A slot holds 8 (ql + 1) bytes, 4 (tl + ql + 4) bytes and 32 ceil(tl / 64) (min(ql, 2 band + 64) + 63) bytes
 * (each part rounded as in sw_extend.h); the band does not widen with |ql - tl|, so the formula is monotone and every slot is sized at
 * (max_tl, max_ql): 6 MiB for 10 000 x 10 000 at band 512.  Grid, persistence and workspace limit as for the banded entry.
 * Everything is enqueued on `stream`; the call does not synchronise.  mgl_sw_ctx_get_timing's fill_kernel: MGL_SW_KERNEL_EXTEND.
 *
 * MGL_SW_FLAG_EXTEND_ADAPTIVE_BAND: THE BAND FOLLOWS THE ALIGNMENT.  Defined by tests/extend_adaptive_textbook.py; everything above holds
 * except the band.  Rows are grouped in blocks of R = MGL_SW_EXTEND_RECENTRE_ROWS = 64: row i >= 1 is in block b = (i - 1) / R, row 0
 * counts with block 0.  Block b has a centre d_b, d_0 = 0, and a cell (i, j), border included, is in the band iff
 * d_b - band <= j - i <= d_b + band for the block b of its own row.  For b >= 1, d_b = rj(R b) - R b, the diagonal of the smallest
 * column holding the largest in-band H of row R b (the border column included where it is in that row's band); d_b = d_(b-1) where row
 * R b has no in-band cell.  A cell has one band, its row's, and an out-of-band cell is minus infinity for every reader: row R b + 1
 * reads H and E of row R b only where row R b had them under d_(b-1).  |d_b - d_(b-1)| <= band follows.  The border column is in the
 * band of row i whenever i + d_b - band <= 0; a row has a cell iff i + d_b - band <= ql, and a row without one drops when the rule is
 * on and is empty when it is off, as above.  rowmax, rj, best, the drop rule, every field of the record and the CIGAR are as above,
 * over this band.  So `band` need only cover the largest indel between two re-centrings, not the drift summed over the extension.
 * A pair with tl <= 64 and any pair at band >= tl + ql give exactly the result without the flag.  The band is used as given up to
 * max_tl + max_ql.  Combines with the three flags above.  A slot holds 4 ceil(tl / 64) bytes more (rounded to 256; not with
 * MGL_SW_FLAG_SCORE_ONLY), still sized at (max_tl, max_ql).  fill_kernel: MGL_SW_KERNEL_EXTEND_ADAPTIVE.
 */
typedef struct mgl_sw_extension {
    int32_t score, t_end, q_end, score_qend, t_end_qend, rows_done, dropped, cigar_from;
} mgl_sw_extension;
int mgl_sw_extend_batch_device(mgl_sw_ctx *ctx, void *stream, int64_t n, const uint8_t *d_targets, const int64_t *d_t_start,
                               const int32_t *d_t_len, const uint8_t *d_queries, const int64_t *d_q_start, const int32_t *d_q_len, int max_tl,
                               int max_ql, int match, int mismatch, int gopen, int gext, int band, int zdrop, mgl_sw_extension *d_ext_out,
                               char *d_cigar_out, int cigar_stride, int32_t *d_cigar_len_out, int32_t *d_status_out, int flags);

/*
 * TWO-SIDED SEED EXTENSION (NOT a reference function; opt-in): a seed in the middle of a read extended to the left and to the right
 * with mgl_sw_extend_batch_device's function and joined into one alignment, all on the device.  Defined by
 * tests/seed_extend_textbook.py.  Per pair: a target window T of tl >= 1 and a query Q of ql >= 1 bytes as above, and a seed
 * (d_seed_t, d_seed_q, d_seed_len: int32 per pair) st, sq, sl that lays T[st .. st + sl) against Q[sq .. sq + sl): sl >= 1, 0 <= st,
 * st + sl <= tl, 0 <= sq, sq + sl <= ql.  Per call: the parameters, band, zdrop and the flags of mgl_sw_extend_batch_device, which hold
 * for each side unchanged (the band clamp is that entry's, for the flag in force).
 *   Seed: one `sl M` element; seed_score = the sum of match / mismatch over its sl columns (a seed need not be exact).
 *   Right side: the extension of Q[sq + sl ..) along T[st + sl ..) as defined above (with MGL_SW_FLAG_EXTEND_ADAPTIVE_BAND: as defined
 *   there).  Left side: the same function on the REVERSED flanks, reverse(T[0 .. st)) and reverse(Q[0 .. sq)); its CIGAR elements are
 *   taken in reverse order.  What is said there about long deletions and the band holds for each side on its own.
 *   A side with an empty flank never reaches the extension: with an empty query flank (the target flank empty or not) its record is
 *   all zero -- the empty extension, which ends on column ql = 0 --; with the target flank alone empty it is all zero except
 *   score_qend = -0x40000000, t_end_qend = -1 (no row reaches column ql).  Both have an empty CIGAR.
 *   A side contributes the H of the cell its CIGAR starts from: score_qend at (t_end_qend, flank ql) where its cigar_from is 1,
 *   otherwise score at (t_end, q_end).
 * mgl_sw_seed_alignment: score = left contribution + seed_score + right contribution; t_beg, t_end, q_beg, q_end, half open, in the
 * window's and the query's coordinates: t_beg = st - the left start cell's row, t_end = st + sl + the right start cell's row, the query
 * likewise with the columns; seed_score; dropped and cigar_from: the sides' values, bit 0 left, bit 1 right.
 * d_left_out, d_right_out (optional, each may be NULL): the two sides' mgl_sw_extension in FLANK coordinates (the left one on the
 * reversed flanks), as mgl_sw_extend_batch_device gives them, or the records above for an empty flank.
 * The CIGAR: the left side's elements last to first, `sl M`, the right side's first to last, adjacent equal operations merged (only
 * the seed's neighbours can be); M / I / D, no clips -- q_beg / q_end say what a soft clip would.  It spends exactly t_end - t_beg
 * target and q_end - q_beg query bases.
 * flags: MGL_SW_FLAG_EXTEND_TO_QUERY_END, MGL_SW_FLAG_EXTEND_ADAPTIVE_BAND, MGL_SW_FLAG_BINARY_CIGAR, MGL_SW_FLAG_SCORE_ONLY (records only;
 * d_cigar_out / d_cigar_len_out may be NULL); others are ignored.  The call fails before any device work with MGL_SW_ERR_BAD_ARG on
 * n < 0, a null sequence / start / length / seed array, a null d_aln_out, band < 0, max_tl < 1 or max_ql < 1, and -- without
 * MGL_SW_FLAG_SCORE_ONLY -- a null CIGAR array or a stride below 2 (4 for binary); with MGL_SW_ERR_DEVICE without a GPU.
 * d_status_out (optional): MGL_SW_ERR_BAD_ARG for a length below 1 or above max_tl / max_ql or a seed that breaks the inequalities
 * above; MGL_SW_ERR_UNSUPPORTED where a non-empty side is outside the banded range guard or too large for one workspace slot, or the
 * pair has a length above 2^28 or max(match, |mismatch|) * sl > 2^29; MGL_SW_ERR_CIGAR_OVERFLOW where the JOINED CIGAR does not fit
 * cigar_stride, and only then (a side's internal row holds as many elements as a joined CIGAR of cigar_stride bytes can have, or as
 * max_tl + max_ql admits: sw_seed_extend.h).  A pair with a non-zero status gets an all-zero record, all-zero side records, a
 * cigar_len of 0 and no byte of its CIGAR row written; nor is any byte of a row at or beyond that pair's cigar_len.
 * Device work, all on `stream`, no synchronisation: sw_seed_split_kernel (seed checks, flank descriptors, the reversed copies of the
 * left flanks; the right flanks are read in place), the extension kernel once over the left and once over the right flanks, and
 * sw_seed_join_kernel (seed score, record, joined CIGAR).  The staging -- per pair about max_tl + max_ql bytes of reversed flanks, 150
 * bytes of descriptors and records and two internal CIGAR rows of at most 2 cigar_stride bytes -- and the extension slots come out of
 * one borrowing of the context's workspace and count against its limit: a batch whose staging is more than half the limit is worked
 * off in chunks of as many pairs as half the limit holds (one pair a chunk where half the limit does not hold one: its staging then
 * takes more than half), and a limit that does not hold one pair's staging beside a slot fails with MGL_SW_ERR_NOMEM.  Slots, grid and
 * persistence as for mgl_sw_extend_batch_device.  mgl_sw_ctx_get_timing's fill_kernel: MGL_SW_KERNEL_EXTEND, or
 * MGL_SW_KERNEL_EXTEND_ADAPTIVE with the flag -- the fill that ran; dp_launches counts two per chunk.
 */
typedef struct mgl_sw_seed_alignment {
    int32_t score, t_beg, t_end, q_beg, q_end, seed_score, dropped, cigar_from;
} mgl_sw_seed_alignment;
int mgl_sw_extend_seed_batch_device(mgl_sw_ctx *ctx, void *stream, int64_t n, const uint8_t *d_targets, const int64_t *d_t_start,
                                    const int32_t *d_t_len, const uint8_t *d_queries, const int64_t *d_q_start, const int32_t *d_q_len,
                                    const int32_t *d_seed_t, const int32_t *d_seed_q, const int32_t *d_seed_len, int max_tl, int max_ql, int match,
                                    int mismatch, int gopen, int gext, int band, int zdrop, mgl_sw_seed_alignment *d_aln_out,
                                    mgl_sw_extension *d_left_out, mgl_sw_extension *d_right_out, char *d_cigar_out, int cigar_stride,
                                    int32_t *d_cigar_len_out, int32_t *d_status_out, int flags);

/*
 * CHAIN ALIGNMENT (NOT a reference function; opt-in): what a long-read mapper hands an aligner is a chain, several colinear anchors
 * per read.  The left side of the first anchor and the right side of the last one are extended as mgl_sw_extend_seed_batch_device
 * extends a seed's, every gap between two consecutive anchors is filled GLOBALLY over a diagonal band, and all of it is joined into
 * one alignment on the device.  Defined by tests/chain_textbook.py.  Per pair p: a target window T of tl >= 1 and a query Q of
 * ql >= 1 bytes as above, and K >= 1 anchors: d_anchor_start (int64, n + 1 entries, ascending, CSR into the anchor arrays: pair p has
 * anchors d_anchor_start[p] .. d_anchor_start[p + 1] - 1, all inside [0, total_anchors)), d_anchor_t, d_anchor_q, d_anchor_len
 * (int32 per anchor): anchor k lays T[st_k .. st_k + sl_k) against Q[sq_k .. sq_k + sl_k), sl_k >= 1, 0 <= st_0, 0 <= sq_0,
 * st_k + sl_k <= st_(k+1) and sq_k + sl_k <= sq_(k+1), and the last anchor ends inside the window and the query.  Per call: the
 * parameters, band, zdrop and the flags of mgl_sw_extend_seed_batch_device.
 *   Anchors: one `sl_k M` element each; anchor_score = the sum of match / mismatch over all anchors' columns (they need not be exact).
 *   Left and right side: exactly those of mgl_sw_extend_seed_batch_device, the left side of anchor 0 on the reversed flanks and the
 *   right side of anchor K - 1 -- the records of an empty flank, cigar_from and what a side contributes included.
 *   Gap k, between anchors k and k + 1: T[st_k + sl_k .. st_(k+1)) against Q[sq_k + sl_k .. sq_(k+1)), gt and gq bases.
 *   gt = gq = 0: no element, score 0.  gt = 0 < gq: `gq I`, score -(gopen + (gq - 1) gext).  gq = 0 < gt: `gt D`, likewise.
 *   Otherwise the global fill: mgl_sw_align_batch_device_banded's function under MGL_SW_OS_INDEL on the gap -- its band rule
 *   (lo = min(0, gq - gt) - band, hi = max(0, gq - gt) + band: both corners are in the band), gap-penalty borders on both axes, its
 *   recurrence, priorities, run lengths and minus infinity, its walk from (gt, gq) back to (0, 0) -- and the gap's score is
 *   H(gt, gq), which that entry does not return.  Always the plain band rule, also with MGL_SW_FLAG_EXTEND_ADAPTIVE_BAND, which
 *   holds for the two sides only.  LIMIT: there is no Z-drop inside a gap; a gap is aligned end to end whatever it costs.
 * mgl_sw_chain_alignment: score = left contribution + anchor_score + the gaps' scores + right contribution; t_beg, t_end, q_beg,
 * q_end half open, as in mgl_sw_seed_alignment with st_0 in front and the last anchor's end behind; anchor_score; dropped and
 * cigar_from: the sides' values, bit 0 left, bit 1 right.  For K = 1 the record is bit for bit mgl_sw_seed_alignment.
 * d_left_out, d_right_out (optional): the sides' records, as there.  d_gap_score_out (optional): one int32 per anchor index, the
 * score of the gap behind that anchor; 0 for a pair's last anchor, for the anchors of a pair with a non-zero status and for anchors
 * that belong to no pair.
 * The CIGAR: the left side's elements last to first, anchor 0, gap 0, anchor 1, ..., anchor K - 1, the right side's elements,
 * adjacent equal operations merged (only an M next to an anchor can be; two anchors merge across an empty gap); M / I / D.  It spends
 * exactly t_end - t_beg target and q_end - q_beg query bases.
 * max_gap_tl, max_gap_ql (>= 0): the caller's bounds on gt and gq of the gaps that have bases on both sides; they size the fill's
 * slots and the gaps' internal rows as max_tl and max_ql size a side's.
 * flags: as mgl_sw_extend_seed_batch_device.  The call fails before any device work with MGL_SW_ERR_BAD_ARG on n < 0 or above 2^30,
 * total_anchors < 0 or above 2^30, a null sequence / start / length / anchor array, a null d_aln_out, band < 0, max_tl < 1 or
 * max_ql < 1, max_gap_tl < 0 or max_gap_ql < 0, and -- without MGL_SW_FLAG_SCORE_ONLY -- a null CIGAR array or a stride below 2
 * (4 for binary); with MGL_SW_ERR_DEVICE without a GPU.
 * d_status_out (optional), in this order: MGL_SW_ERR_BAD_ARG for a length below 1 or above max_tl / max_ql, for K < 1 or a range of
 * d_anchor_start that descends or leaves [0, total_anchors), for an anchor that breaks an inequality above, and for a pair whose
 * range shares an anchor with that of a pair of lower index (which keeps the anchor);
 * MGL_SW_ERR_UNSUPPORTED where a non-empty side is refused as by mgl_sw_extend_seed_batch_device, where a gap with bases on both
 * sides is longer than max_gap_tl / max_gap_ql, outside the banded range guard or too large for one workspace slot, where a length
 * is above 2^28, and where the pair fails the sum guard
 *   max(match, |mismatch|) min(tl, ql) + 2 gopen (K + 1) + gext (tl + ql) <= 2^30
 * -- the sum of the banded range guard's bounds over the pair's K + 1 filled segments and K anchors, so that every partial sum of
 * segment scores stays in an int32; MGL_SW_ERR_CIGAR_OVERFLOW where the JOINED CIGAR does not fit cigar_stride, and only then (the
 * internal row of a side or a gap holds as many elements as a joined CIGAR of cigar_stride bytes can have: sw_chain.h).  A pair with
 * a non-zero status gets an all-zero record, all-zero side records, a cigar_len of 0 and no byte of its CIGAR row written; nor is
 * any byte of a row at or beyond that pair's cigar_len.
 * Device work, all on `stream`, no synchronisation: sw_chain_split_kernel (the checks, the flank descriptors and the reversed left
 * flanks, one gap descriptor per anchor), the extension kernel once over the left and once over the right flanks,
 * sw_gap_fill_kernel (one wave per gap, persistent on slots) and sw_chain_join_kernel (anchor scores, record, d_gap_score_out, joined
 * CIGAR).  The staging -- per pair what mgl_sw_extend_seed_batch_device stages, per anchor 16 bytes and an internal CIGAR row of at
 * most 2 cigar_stride and at most 4 (max_gap_tl + max_gap_ql) bytes -- and the slots come out of one borrowing of the context's
 * workspace and count against its limit.  The extension slots are sized at (max_tl, max_ql), the fill's as
 * mgl_sw_align_batch_device_banded sizes them at (max_gap_tl, max_gap_ql, band); the two kinds follow one another on the stream and
 * share one region behind the staging.  The anchor counts are device data, so the batch is staged whole: a limit that does not hold
 * its staging beside a slot fails with MGL_SW_ERR_NOMEM, and the caller splits the batch.  mgl_sw_ctx_get_timing's fill_kernel:
 * MGL_SW_KERNEL_EXTEND, or MGL_SW_KERNEL_EXTEND_ADAPTIVE with the flag -- the extension that ran; dp_launches counts three.
 */
typedef struct mgl_sw_chain_alignment {
    int32_t score, t_beg, t_end, q_beg, q_end, anchor_score, dropped, cigar_from;
} mgl_sw_chain_alignment;
int mgl_sw_align_chain_batch_device(mgl_sw_ctx *ctx, void *stream, int64_t n, const uint8_t *d_targets, const int64_t *d_t_start,
                                    const int32_t *d_t_len, const uint8_t *d_queries, const int64_t *d_q_start, const int32_t *d_q_len,
                                    const int64_t *d_anchor_start, const int32_t *d_anchor_t, const int32_t *d_anchor_q, const int32_t *d_anchor_len,
                                    int64_t total_anchors, int max_tl, int max_ql, int max_gap_tl, int max_gap_ql, int match, int mismatch, int gopen,
                                    int gext, int band, int zdrop, mgl_sw_chain_alignment *d_aln_out, mgl_sw_extension *d_left_out,
                                    mgl_sw_extension *d_right_out, int32_t *d_gap_score_out, char *d_cigar_out, int cigar_stride,
                                    int32_t *d_cigar_len_out, int32_t *d_status_out, int flags);

/*
 * ANCHOR CHAINING (NOT a reference function; opt-in): the chain stage in front of mgl_sw_align_chain_batch_device.  A read's seed hits
 * -- candidates, many of them on a wrong diagonal or from repeats -- go in; the best colinear chain comes out, on the device, in the
 * layout that entry reads.  Integers only; defined by tests/chain_dp_textbook.py.  Per read p: tl = d_t_len[p] and ql = d_q_len[p]
 * (no sequence byte is read) and N_p >= 0 candidates: d_cand_start (int64, n + 1 entries, CSR into d_cand_t, d_cand_q, d_cand_len,
 * int32 arrays of total_cand entries); candidate i lays T[t_i .. t_i + l_i) against Q[q_i .. q_i + l_i), the chain entry's convention.
 * Per call: max_pred in 1 .. 64, max_dist_t, max_dist_q, bw >= 0, pen_gap, pen_skip >= 0 in 1/256 units.
 * The DP is defined on INDEX order alone: the entry neither sorts nor checks an order.  Callers sort a read's candidates by target
 * position, so that the window of max_pred predecessors means something.  j may precede i iff
 *   i - max_pred <= j < i,  dt = t_i - (t_j + l_j) >= 0,  dq = q_i - (q_j + l_j) >= 0,  dt <= max_dist_t,  dq <= max_dist_q,
 *   dd = |dt - dq| <= bw
 * (no overlap: exactly the inequalities the chain entry demands of two consecutive anchors), and
 *   f(i) = max( l_i, max_j f(j) + l_i - pen(j, i) ),  pen = ((pen_gap dd + pen_skip min(dt, dq)) >> 8) + (ilog2(dd + 1) >> 1),
 * ilog2 = floor log2: minimap2's chaining score with its float terms made integer.  Ties go to the largest j, "no predecessor"
 * counting as j = -1; pred(i) is that j, relative to the read's first candidate.  The chain ends in the i with the largest f(i), ties
 * to the smallest i, follows pred to -1 and is emitted in ascending order, K_p anchors; its score is f(end).  f >= 1, and f is at most
 * the sum of the chain's l, which is at most ql because every step has dq >= 0: f is an int32 for every ql.  N_p = 0: K_p = 0, score
 * 0, status 0 (mgl_sw_align_chain_batch_device then refuses that pair for K < 1).
 * Outputs, all device memory: d_chain_start_out (int64, n + 1 entries, ascending: the prefix sum of K_p, made on the device);
 * d_chain_t_out, d_chain_q_out, d_chain_len_out (int32, capacity total_cand): read p's anchors from d_chain_start_out[p] on, nothing
 * written at or beyond d_chain_start_out[n]; d_chain_score_out (int32, n); d_f_out, d_pred_out (optional, int32 per candidate): f and
 * pred of every candidate of a read with status 0, for callers who trace other chains themselves.  With total_anchors = total_cand,
 * max_gap_tl = max_dist_t and max_gap_ql = max_dist_q these arrays are valid arguments of mgl_sw_align_chain_batch_device as they are.
 * The call fails before any device work with MGL_SW_ERR_BAD_ARG on a null required array, n or total_cand outside [0, 2^30],
 * max_pred outside 1 .. 64, a negative distance, bw or penalty, max_cand < 0, and
 * pen_gap bw + pen_skip min(max_dist_t, max_dist_q) >= 2^31 (the int32 guard of pen); with MGL_SW_ERR_DEVICE without a GPU.
 * d_status_out (optional), per read, in this order: MGL_SW_ERR_BAD_ARG for a range of d_cand_start that descends or leaves
 * [0, total_cand), tl or ql below 1, a candidate with l < 1, t < 0, q < 0, t + l > tl or q + l > ql; MGL_SW_ERR_UNSUPPORTED for
 * N_p > max_cand, the caller's bound, which sizes what the kernel keeps per read (one byte per candidate: in LDS up to 32768, in a
 * workspace slot per wave beyond).  A refused read gets K_p = 0, score 0 and nothing else written.  Ranges that overlap (possible only
 * around a descending one) are the caller's error: the reads that share candidates get unspecified chains, nothing is written out of
 * bounds.
 * Device work, all on `stream`, no synchronisation: sw_chain_dp_kernel (one wave per read, persistent: the checks, the DP, the
 * trace-back), sw_chain_dp_scan_kernel (d_chain_start_out) and sw_chain_dp_pack_kernel (the chains into their CSR place).  The
 * workspace -- 4 bytes per read, 4 per candidate, and the slots -- comes out of one borrowing of the context's and counts against
 * its limit: MGL_SW_ERR_NOMEM where the limit does not hold it beside one slot.  This stage has no MGL_SW_KERNEL_* id:
 * mgl_sw_ctx_get_timing's fill_kernel stays what it was (the other fields are reset as by every device entry).
 * LIMITS: max_pred <= 64; overlapping hits on one diagonal are not chained to each other (minimap2 trims them); one chain per read
 * (d_f_out / d_pred_out are the way to others); no max_skip heuristic; candidates are not sorted here.
 */
int mgl_sw_chain_anchors_batch_device(mgl_sw_ctx *ctx, void *stream, int64_t n, const int32_t *d_t_len, const int32_t *d_q_len,
                                      const int64_t *d_cand_start, const int32_t *d_cand_t, const int32_t *d_cand_q, const int32_t *d_cand_len,
                                      int64_t total_cand, int max_cand, int max_pred, int max_dist_t, int max_dist_q, int bw, int pen_gap, int pen_skip,
                                      int64_t *d_chain_start_out, int32_t *d_chain_t_out, int32_t *d_chain_q_out, int32_t *d_chain_len_out,
                                      int32_t *d_chain_score_out, int32_t *d_f_out, int32_t *d_pred_out, int32_t *d_status_out);

/*
 * ANCHOR CHAINING IN GROUPS (NOT a reference function; opt-in): mgl_sw_chain_anchors_batch_device with one more required array,
 * d_cand_group (int32 per candidate; mgl_sw_index_contig_of_batch_device writes it).  Defined by tests/contig_textbook.py
 * (chain_dp_grouped).  j may precede i only if, beside that entry's inequalities, group[j] == group[i] and group[i] >= 0 -- the rule
 * minimap2 applies with rid.  A candidate of group -1 is a chain of its own with f = l.  Group values are not checked.  The outputs,
 * the statuses and their order, the workspace, the scan and the pack are that entry's; a null d_cand_group is MGL_SW_ERR_BAD_ARG
 * before any device work.  Device work: sw_chain_dp_kernel<true> in place of <false>.  DESIGN.md section 9m.
 */
int mgl_sw_chain_anchors_grouped_batch_device(mgl_sw_ctx *ctx, void *stream, int64_t n, const int32_t *d_t_len, const int32_t *d_q_len,
                                              const int64_t *d_cand_start, const int32_t *d_cand_t, const int32_t *d_cand_q, const int32_t *d_cand_len,
                                              const int32_t *d_cand_group, int64_t total_cand, int max_cand, int max_pred, int max_dist_t, int max_dist_q,
                                              int bw, int pen_gap, int pen_skip, int64_t *d_chain_start_out, int32_t *d_chain_t_out, int32_t *d_chain_q_out,
                                              int32_t *d_chain_len_out, int32_t *d_chain_score_out, int32_t *d_f_out, int32_t *d_pred_out,
                                              int32_t *d_status_out);

/*
 * SEEDING (NOT a reference function; opt-in): the seed stage in front of mgl_sw_chain_anchors_batch_device.  Reads and their windows go
 * in; every pair's candidate anchors come out, on the device, in the CSR layout and the order that entry reads.  A read is seeded
 * against its OWN window -- no index.  Integers only; defined by tests/seed_textbook.py.  Per pair p: the window T (tl = d_t_len[p]
 * bytes from d_targets + d_t_start[p]) and the query Q (ql = d_q_len[p] bytes from d_queries + d_q_start[p]), ASCII.  Per call: k in
 * 4 .. 16, w in 1 .. 32, max_occ in 1 .. 64, merge 0 / 1, max_cand in 1 .. 8192, cand_capacity in 0 .. 2^30.
 * k-mers: A = 0, C = 1, G = 2, T = 3, upper case only; the k-mer at position i is valid iff all of its k bytes are one of these; its key
 * is the 2k-bit number with the first base in the top bits; h = fmix32(key ^ 0x9E3779B9), murmur3's 32-bit finaliser.
 * The sketch of a sequence of L bytes, nk = L - k + 1 positions (empty for nk < 1): the windows are [a, a + w) for a = 0 .. nk - w, the one
 * window [0, nk) if nk < w; a window selects its valid position with the smallest h, ties to the smallest position, nothing if none is
 * valid; the sketch is the set of selected positions.
 * Hits: with occ(x) the number of positions of Q's sketch with key x, every position t of T's sketch with key x and 1 <= occ(x) <= max_occ
 * gives one raw hit (t, q, k) per position q of Q's sketch with key x; R_p is their number.
 * Merge (merge = 1): raw hits on one diagonal t - q are joined while the next starts at or before the end of the run so far (overlapping
 * or touching); a run is the candidate (t0, q0, t_last + k - t0) -- the maximal diagonal runs of the cells the raw hits cover, each an
 * exact match.  merge = 0: the candidates are the raw hits.  A pair's N_p candidates are ascending by (t, q), strictly.
 * d_status_out (optional), per pair, the first that applies: MGL_SW_ERR_BAD_ARG for tl < 1 or ql < 1; MGL_SW_ERR_UNSUPPORTED for a query
 * sketch of more than 8192 positions or R_p > max_cand (the bound is on the RAW hits: what the kernel holds and sorts);
 * MGL_SW_ERR_NOMEM by the capacity rule: with S_p the sum of N_j over j < p (a refused pair counts 0), pairs are kept in index order while
 * S_p + N_p <= cand_capacity, and from the first pair P* that does not fit on every pair, empty ones included, is MGL_SW_ERR_NOMEM (one
 * refused above keeps that status).  A pair with a non-zero status has N_p = 0.
 * Outputs, all device memory: d_cand_start_out (int64, n + 1 entries): S_p for p <= P*, S_(P*) beyond it -- ascending, and
 * d_cand_start_out[n] <= cand_capacity; d_cand_t_out, d_cand_q_out, d_cand_len_out (int32, capacity cand_capacity): nothing is written
 * at or beyond d_cand_start_out[n].  With total_cand = cand_capacity the four arrays are valid arguments of
 * mgl_sw_chain_anchors_batch_device as they are.
 * The call fails before any device work with MGL_SW_ERR_BAD_ARG on n outside [0, 2^30], a null required array or a parameter outside its
 * range above; with MGL_SW_ERR_DEVICE without a GPU; with MGL_SW_ERR_NOMEM where the workspace limit does not hold the batch's staging
 * (4 + 12 max_cand bytes per pair: the batch is staged whole) beside one slot (64 KiB, 160 KiB where max_cand is above 2048).
 * Device work, all on `stream`, no synchronisation: sw_seed_kernel (one workgroup per pair, persistent: both sketches, the probe, the
 * merge), sw_seed_scan_kernel (d_cand_start_out and the capacity cut) and sw_seed_pack_kernel (the candidates into their CSR place), out
 * of one borrowing of the context's workspace.  This stage has no MGL_SW_KERNEL_* id: mgl_sw_ctx_get_timing's fill_kernel stays what it
 * was (the other fields are reset as by every device entry).
 * LIMITS: forward strand only (both: mgl_sw_seed_strands_batch_device below); the pair's own window (against an index of a whole
 * reference: mgl_sw_seed_index_batch_device below); k <= 16; a query's sketch and a pair's raw hits are bounded
 * at 8192; no occurrence cap on the window's side (mgl_sw_seed_index_batch_device has one); the batch is staged whole.
 */
int mgl_sw_seed_batch_device(mgl_sw_ctx *ctx, void *stream, int64_t n, const uint8_t *d_targets, const int64_t *d_t_start, const int32_t *d_t_len,
                             const uint8_t *d_queries, const int64_t *d_q_start, const int32_t *d_q_len, int k, int w, int max_occ, int merge,
                             int max_cand, int64_t cand_capacity, int64_t *d_cand_start_out, int32_t *d_cand_t_out, int32_t *d_cand_q_out,
                             int32_t *d_cand_len_out, int32_t *d_status_out);

/*
 * SEEDING BOTH STRANDS (NOT a reference function; opt-in): mgl_sw_seed_batch_device for reads of unknown orientation.  Defined by
 * tests/strand_textbook.py: the result is mgl_sw_seed_batch_device's on the batch of 2n ROWS, row 2p = (T_p, Q_p) and row 2p + 1 =
 * (T_p, rc(Q_p)), with rc(Q)[i] = comp(Q[ql - 1 - i]); comp swaps upper-case A <-> T and C <-> G and maps every other byte to itself, so
 * a k-mer that is not valid stays so at its mirrored place.  Statuses, the max_cand and 8192-sketch bounds and the capacity rule are
 * per row and in row order; a candidate's q is a coordinate of that row's ORIENTED read.  Row 2p is what mgl_sw_seed_batch_device
 * gives for pair p.  The arguments are that entry's, with n in [0, 2^29].
 * Outputs, all device memory: d_cand_start_out (int64, 2n + 1 entries); d_cand_t_out, d_cand_q_out, d_cand_len_out (int32, capacity
 * cand_capacity): nothing is written at or beyond d_cand_start_out[2n]; d_row_t_len_out, d_row_q_len_out (optional, int32, 2n entries
 * each): tl_p and ql_p per row, so that with total_cand = cand_capacity these arrays are valid arguments of
 * mgl_sw_chain_anchors_batch_device over 2n reads as they are; d_status_out (optional, 2n entries).
 * The call fails before any device work as mgl_sw_seed_batch_device does; MGL_SW_ERR_NOMEM where the workspace limit does not hold the
 * staging of the 2n rows (4 + 12 max_cand bytes per row) beside one slot (128 KiB, 320 KiB where max_cand is above 2048).
 * Device work, all on `stream`, no synchronisation: sw_seed_strands_kernel (one workgroup per pair, persistent: the read sketched in both
 * orientations from its bytes in place, the window read and sketched ONCE and probed against both, the merge per row), then
 * sw_seed_scan_kernel and sw_seed_pack_kernel over the 2n rows, out of one borrowing of the context's workspace.  No MGL_SW_KERNEL_*
 * id: mgl_sw_ctx_get_timing's fill_kernel stays what it was.
 * LIMITS: those of mgl_sw_seed_batch_device but the strand; the staging doubles.
 */
int mgl_sw_seed_strands_batch_device(mgl_sw_ctx *ctx, void *stream, int64_t n, const uint8_t *d_targets, const int64_t *d_t_start,
                                     const int32_t *d_t_len, const uint8_t *d_queries, const int64_t *d_q_start, const int32_t *d_q_len, int k, int w,
                                     int max_occ, int merge, int max_cand, int64_t cand_capacity, int64_t *d_cand_start_out, int32_t *d_cand_t_out,
                                     int32_t *d_cand_q_out, int32_t *d_cand_len_out, int32_t *d_row_t_len_out, int32_t *d_row_q_len_out,
                                     int32_t *d_status_out);

/*
 * THE STRAND OF A READ (NOT a reference function; opt-in): between mgl_sw_chain_anchors_batch_device over the 2n rows of
 * mgl_sw_seed_strands_batch_device and mgl_sw_align_chain_batch_device.  Defined by tests/strand_textbook.py (select_strand).  In: the
 * n reads (d_queries, d_q_start, d_q_len; query_bytes is the size of d_queries and of d_queries_out) and the chain stage's outputs over
 * the 2n rows: d_chain_start (int64, 2n + 1), d_chain_t, d_chain_q, d_chain_len (int32, total_chain entries, in [0, 2^30]),
 * d_chain_score (int32, 2n).  Row r has K_r = d_chain_start[r + 1] - d_chain_start[r] anchors and the score c_r = d_chain_score[r], 0
 * where K_r = 0.  strand_p = 1 iff c_(2p+1) > c_(2p): ties and two zeros give strand 0.  Pair p gets the K_p anchors of row
 * 2p + strand_p and the oriented read, Q_p or rc(Q_p).
 * Outputs, all device memory: d_strand_out (int32, n); d_queries_out (uint8, query_bytes; it must not overlap d_queries): read p
 * oriented, at the SAME offset d_q_start[p], so that d_q_start and d_q_len serve both buffers -- no byte outside a read is written;
 * d_anchor_start_out (int64, n + 1: the prefix sum of K_p, made on the device); d_anchor_t_out, d_anchor_q_out, d_anchor_len_out (int32,
 * capacity total_chain): nothing is written at or beyond d_anchor_start_out[n] -- valid arguments of mgl_sw_align_chain_batch_device
 * as they are; d_score_out (optional, int32, n: the chosen chain's score); d_status_out (optional, int32, n).
 * Per pair MGL_SW_ERR_BAD_ARG for ql < 1, a read that leaves [0, query_bytes) or a row's range of d_chain_start that descends or leaves
 * [0, total_chain]: strand 0, K_p = 0, score 0, and neither a byte nor an anchor is written for it.  Reads that overlap in d_queries,
 * or row ranges that overlap, are the caller's error: the result is unspecified, nothing is written out of bounds.
 * The call fails before any device work with MGL_SW_ERR_BAD_ARG on a null required array, n outside [0, 2^29], total_chain outside
 * [0, 2^30] or query_bytes < 0; with MGL_SW_ERR_DEVICE without a GPU.
 * Device work, all on `stream`, no synchronisation: sw_select_strand_kernel, sw_select_strand_scan_kernel, sw_select_strand_pack_kernel;
 * the workspace is 4 bytes per pair.  No MGL_SW_KERNEL_* id.
 * LIMITS: the choice is by chain score alone; one chain per read.
 */
int mgl_sw_select_strand_batch_device(mgl_sw_ctx *ctx, void *stream, int64_t n, const uint8_t *d_queries, const int64_t *d_q_start,
                                      const int32_t *d_q_len, const int64_t *d_chain_start, const int32_t *d_chain_t, const int32_t *d_chain_q,
                                      const int32_t *d_chain_len, const int32_t *d_chain_score, int64_t total_chain, int64_t query_bytes,
                                      int32_t *d_strand_out, uint8_t *d_queries_out, int64_t *d_anchor_start_out, int32_t *d_anchor_t_out,
                                      int32_t *d_anchor_q_out, int32_t *d_anchor_len_out, int32_t *d_score_out, int32_t *d_status_out);

/*
 * A MINIMIZER INDEX OF ONE REFERENCE (NOT a reference function; opt-in): what the seed stages above lack -- with it a read needs no
 * window of its own.  Defined by tests/index_textbook.py (build_index): the sketch of the reference (ref_len bytes at d_ref, device
 * memory, ASCII) by mgl_sw_seed_batch_device's definition, as M entries (key, position) ascending by (key, position).  k in 4 .. 16, w in
 * 1 .. 32, ref_len in 1 .. 2^31 - 1; positions are int32; M = 0 (a reference shorter than k, or without a valid k-mer) is a valid
 * index.  A key is the whole k-mer, so a hit is an exact match without the reference being read.
 * The handle is an opaque device object with allocations of its OWN -- not the context's workspace: it outlives calls --; several may
 * live on one context; it does not keep d_ref.  mgl_sw_index_build_device SYNCHRONISES `stream` -- it learns M before it allocates M
 * entries --, the one entry of this family that does.  *out is null on every failure.  mgl_sw_index_destroy(NULL) is harmless; an index
 * is destroyed before its device is reset, in any order with its context.
 * mgl_sw_index_get_info: ref_len, k, w, entries = M, bytes = the index's device memory (8 per entry and the bucket table).
 * mgl_sw_index_export_device: the M entries ascending into d_keys_out and d_pos_out (device memory, `capacity` entries each), enqueued
 * on `stream`, not synchronised; the internal layout is not part of the interface.
 * MGL_SW_ERR_BAD_ARG before any device work for a null pointer (a null index included), ref_len, k or w outside its range, capacity
 * below M; MGL_SW_ERR_DEVICE without a GPU; a failed allocation is MGL_SW_ERR_NOMEM or MGL_SW_ERR_DEVICE as the runtime reports it.
 * Device work of the build: sw_index_sketch_kernel twice (a count per block of 1024 positions, then the entries), sw_index_scan_kernel
 * between them, rocPRIM's radix sort over bits [0, 32 + 2k), sw_index_split_kernel, sw_index_bucket_kernel (a table over the top
 * min(2k, 24, max(10, ceil(log2 M))) bits of a key).  Scratch of the build -- 16 bytes per entry and the sort's -- is freed before it
 * returns.  No MGL_SW_KERNEL_* id.
 * LIMITS: this build knows ONE reference sequence; a reference of several contigs goes through mgl_sw_index_build_contigs_device
 * below, which keeps chains and windows inside a contig; ref_len < 2^31; k <= 16; the build synchronises.
 */
typedef struct mgl_sw_index mgl_sw_index;
typedef struct mgl_sw_index_info {
    int64_t ref_len, entries, bytes;
    int32_t k, w;
} mgl_sw_index_info;
int mgl_sw_index_build_device(mgl_sw_ctx *ctx, void *stream, const uint8_t *d_ref, int64_t ref_len, int k, int w, mgl_sw_index **out);
void mgl_sw_index_destroy(mgl_sw_index *idx);
int mgl_sw_index_get_info(const mgl_sw_index *idx, mgl_sw_index_info *out);
int mgl_sw_index_export_device(const mgl_sw_index *idx, void *stream, uint32_t *d_keys_out, int32_t *d_pos_out, int64_t capacity);

/*
 * A REFERENCE OF MANY CONTIGS (NOT a reference function; opt-in): DESIGN.md section 9m; defined by tests/contig_textbook.py.  The
 * reference stays ONE device buffer of ref_len < 2^31 bytes.  Contig c occupies [contig_start[c], contig_start[c] + contig_len[c]);
 * the contigs and the gaps between them tile the buffer: contig_start[0] = 0, contig_len[c] >= 1, contig_start[c] + contig_len[c] <
 * contig_start[c + 1] (at least ONE gap byte between two contigs), the last contig ends at ref_len, and every gap byte is one the seed
 * stage maps to no base (anything but upper-case A, C, G, T; N for instance).  One such byte is enough: no valid k-mer holds it, so no
 * k-mer crosses a boundary, and two hits on either side of it are at least k + 1 apart in t, so the merge cannot join them.
 * The index's entries stay tests/index_textbook.py's build_index(buffer, k, w): the sketch of the WHOLE buffer.  A window of w
 * positions that straddles a gap selects among the valid positions it sees on both sides -- that is part of the definition, not the
 * sketch of every contig on its own.
 * mgl_sw_index_build_contigs_device: contig_start and contig_len are HOST arrays (int64, n_contigs in 1 .. 2^20).  The rules above but
 * the gap bytes are checked on the host: MGL_SW_ERR_BAD_ARG before any device work, as for every argument of
 * mgl_sw_index_build_device.  sw_contig_gap_kernel (a workgroup per gap) reads the gap bytes: one that is a base is
 * MGL_SW_ERR_BAD_ARG too, behind a synchronisation of `stream`.  Then the build of mgl_sw_index_build_device runs as it is; the handle
 * keeps a device copy of the table (start and end, int32: 8 bytes per contig, not counted in mgl_sw_index_info.bytes).  *out is null
 * on every failure.
 * mgl_sw_index_get_contigs: *n_out = the number of contigs; with capacity >= that, the table into the host arrays start_out and
 * len_out (capacity 0 and both null: *n_out alone).  An index of mgl_sw_index_build_device reports ONE contig [0, ref_len), and the two
 * entries below treat it so.  MGL_SW_ERR_BAD_ARG for a null index or n_out, one null array, or a capacity below the number.
 * mgl_sw_index_contig_of_batch_device: per anchor i of `total` (0 .. 2^30; d_t, d_len, d_group_out int32 device arrays) group = c
 * where contig c holds [t, t + l) whole, -1 otherwise: t < 0, l < 1, inside a gap, or over a contig's end.  sw_contig_of_kernel, a
 * thread per anchor, the table searched in LDS up to 4096 contigs and in memory beyond; on `stream`, no workspace, no synchronisation.
 * MGL_SW_ERR_BAD_ARG before any device work for a null pointer or total outside its range; MGL_SW_ERR_DEVICE without a GPU.
 * No MGL_SW_KERNEL_* id.  LIMITS: contigs have no names here; ref_len < 2^31.
 */
int mgl_sw_index_build_contigs_device(mgl_sw_ctx *ctx, void *stream, const uint8_t *d_ref, int64_t ref_len, const int64_t *contig_start,
                                      const int64_t *contig_len, int64_t n_contigs, int k, int w, mgl_sw_index **out);
int mgl_sw_index_get_contigs(const mgl_sw_index *idx, int64_t capacity, int64_t *start_out, int64_t *len_out, int64_t *n_out);
int mgl_sw_index_contig_of_batch_device(mgl_sw_ctx *ctx, void *stream, const mgl_sw_index *idx, int64_t total, const int32_t *d_t,
                                        const int32_t *d_len, int32_t *d_group_out);

/*
 * SEEDING AGAINST THE INDEX (NOT a reference function; opt-in): mgl_sw_seed_strands_batch_device with the whole reference for every
 * read's window.  Defined by tests/index_textbook.py (seed_index_row, seed_index_batch).  strands = 1: n rows, row p = Q_p; strands = 2:
 * 2n rows, row 2p = Q_p and row 2p + 1 = rc(Q_p).  Per row, with occ_Q(x) the positions of the row's sketch with key x and occ_I(x) the
 * index's entries with key x: every position q of the sketch with 1 <= occ_Q(x) <= max_occ and 1 <= occ_I(x) <= max_occ_ref gives one
 * raw hit (t, q, k) per entry t; R_p is their number after both caps; merge, order, statuses (ql < 1; a sketch above 8192 positions or
 * R_p > max_cand; the capacity rule in row order) and the output layouts are mgl_sw_seed_strands_batch_device's over strands * n rows,
 * with d_row_t_len_out = ref_len for every row.  Where no key of the index occurs more than max_occ_ref times a row is what
 * mgl_sw_seed_batch_device gives for (the reference, the oriented read).  k and w are the index's.  max_occ_ref in 1 .. 8192: the cap
 * on the window's side that mgl_sw_seed_batch_device lacks.  Optional outputs: d_row_t_len_out, d_row_q_len_out, d_status_out.
 * With total_cand = cand_capacity the outputs are valid arguments of mgl_sw_chain_anchors_batch_device as they are.
 * MGL_SW_ERR_BAD_ARG before any device work for a null required pointer, strands not 1 or 2, n outside [0, 2^30 / strands], max_occ,
 * max_occ_ref, merge, max_cand or cand_capacity outside its range; MGL_SW_ERR_DEVICE without a GPU; MGL_SW_ERR_NOMEM where the
 * workspace limit does not hold the rows' staging (4 + 12 max_cand bytes per row) beside one slot (64 KiB, 160 KiB where max_cand is
 * above 2048).
 * Device work, all on `stream`, no synchronisation: sw_seed_index_kernel (one workgroup per read, persistent: a row's sketch sorted by
 * key, one lookup per distinct key through the bucket table, the merge), sw_seed_scan_kernel, sw_seed_pack_kernel.  No MGL_SW_KERNEL_*
 * id: mgl_sw_ctx_get_timing's fill_kernel stays what it was.
 * LIMITS: one chain per read follows from this stage: no secondary hits, no mapping quality; a read's raw hits over the WHOLE reference
 * are bounded by max_cand.
 */
int mgl_sw_seed_index_batch_device(mgl_sw_ctx *ctx, void *stream, const mgl_sw_index *idx, int64_t n, const uint8_t *d_queries,
                                   const int64_t *d_q_start, const int32_t *d_q_len, int strands, int max_occ, int max_occ_ref, int merge,
                                   int max_cand, int64_t cand_capacity, int64_t *d_cand_start_out, int32_t *d_cand_t_out, int32_t *d_cand_q_out,
                                   int32_t *d_cand_len_out, int32_t *d_row_t_len_out, int32_t *d_row_q_len_out, int32_t *d_status_out);

/*
 * THE WINDOW OF A CHAIN (NOT a reference function; opt-in): between the chain stage (or mgl_sw_select_strand_batch_device) over rows
 * seeded against an index and mgl_sw_align_chain_batch_device.  Defined by tests/index_textbook.py (locate_window).  Per pair with
 * K >= 1 anchors (d_anchor_start, int64, n + 1; the anchors' t in the reference's coordinates), first (t0, q0, l0) and last
 * (tK, qK, lK), ql = d_q_len[p], in 64 bits: lo = max(0, t0 - q0 - slack), hi = min(ref_len, tK + lK + (ql - qK - lK) + slack);
 * d_t_start_out[p] = lo, d_t_len_out[p] = hi - lo, and every anchor's t - lo goes to d_anchor_t_out, which may be d_anchor_t itself.
 * K = 0: t_start = 0, t_len = 0, status 0 -- the read is unmapped, and the alignment refuses it as it refuses a pair without anchors.
 * d_status_out (optional): MGL_SW_ERR_BAD_ARG for ql < 1, a range of d_anchor_start that descends or leaves [0, total_anchors], or an
 * anchor with l < 1, t < 0, q < 0, t + l > ref_len or q + l > ql; MGL_SW_ERR_UNSUPPORTED for hi - lo > max_tl.  A refused pair has
 * t_start = 0, t_len = 0 and none of its anchors written.
 * Then d_ref, d_t_start_out, d_t_len_out and the rebased anchors are valid arguments of mgl_sw_align_chain_batch_device as they are:
 * the window is never copied.
 * MGL_SW_ERR_BAD_ARG before any device work for a null required pointer, n or total_anchors outside [0, 2^30], ref_len outside
 * 1 .. 2^31 - 1, slack < 0 or max_tl < 1; MGL_SW_ERR_DEVICE without a GPU.
 * Device work on `stream`, no synchronisation, no workspace: sw_locate_window_kernel (a wave per pair).  No MGL_SW_KERNEL_* id.
 */
int mgl_sw_locate_window_batch_device(mgl_sw_ctx *ctx, void *stream, int64_t n, int64_t ref_len, const int32_t *d_q_len,
                                      const int64_t *d_anchor_start, const int32_t *d_anchor_t, const int32_t *d_anchor_q,
                                      const int32_t *d_anchor_len, int64_t total_anchors, int slack, int max_tl, int64_t *d_t_start_out,
                                      int32_t *d_t_len_out, int32_t *d_anchor_t_out, int32_t *d_status_out);

/*
 * THE WINDOW OF A CHAIN INSIDE ITS CONTIG (NOT a reference function; opt-in): mgl_sw_locate_window_batch_device with the index in
 * place of ref_len, and d_rid_out (int32, n).  Defined by tests/contig_textbook.py (locate_window_contigs).  With c the contig of the
 * pair's first anchor: an anchor in another contig or in none (mgl_sw_index_contig_of_batch_device's -1) is MGL_SW_ERR_BAD_ARG for
 * the pair; lo = max(start[c], t0 - q0 - slack), hi = min(end[c], tK + lK + (ql - qK - lK) + slack).  d_t_start_out stays in the
 * BUFFER's coordinates -- the alignment reads the reference in place --; d_rid_out[p] = c for a kept pair, -1 for an unmapped or a
 * refused one.  Every other check, output and the in-place rule are mgl_sw_locate_window_batch_device's, and so are the call-level
 * refusals (a null index or d_rid_out among them).  Device work on `stream`, no synchronisation, no workspace:
 * sw_locate_window_contigs_kernel (a wave per pair).  No MGL_SW_KERNEL_* id.
 */
int mgl_sw_locate_window_contigs_batch_device(mgl_sw_ctx *ctx, void *stream, int64_t n, const mgl_sw_index *idx, const int32_t *d_q_len,
                                              const int64_t *d_anchor_start, const int32_t *d_anchor_t, const int32_t *d_anchor_q,
                                              const int32_t *d_anchor_len, int64_t total_anchors, int slack, int max_tl, int64_t *d_t_start_out,
                                              int32_t *d_t_len_out, int32_t *d_anchor_t_out, int32_t *d_rid_out, int32_t *d_status_out);

/*
 * SECONDARY CHAINS AND MAPPING QUALITY (NOT a reference function; opt-in): behind mgl_sw_chain_anchors_batch_device, beside the strand
 * choice.  Defined by tests/rank_textbook.py; DESIGN.md section 9k.  The n reads have `strands` rows each (1 or 2: rows strands * p ..,
 * as mgl_sw_seed_index_batch_device lays them out); row r has the candidates d_cand_start[r] .. d_cand_start[r + 1] (int64, n * strands
 * + 1), d_row_q_len[r], the chain stage's d_f / d_pred for them (its optional outputs d_f_out / d_pred_out; pred relative to the row's
 * first candidate, -1: none) and, optionally, its status d_row_status[r].
 * Per row the candidates are visited by (f descending, index ascending); an unused one with f >= min_score starts a walk along pred
 * that marks what it passes and stops at -1 or at a used candidate i; the chain scores f(end) or f(end) - f(i) and is kept iff its
 * score >= min_score and its anchors K >= min_cnt.  The kept chains of a read's rows are ranked by (score descending, strand ascending,
 * end_index ascending) and cut to max_chains (1 .. 16).  In rank order a chain whose interval on the forward read overlaps an earlier
 * primary chain's by mask_level / 256 (1 .. 256; minimap2's 0.5 is 128) of the shorter of the two is that chain's secondary; otherwise
 * it is primary (parent = its own rank).  A primary chain gets mapq 0 .. 60 from its score, its best secondary's score (subsc), their
 * number (n_sub) and K, in integers; a secondary chain has mapq, n_sub and subsc 0.  No parity with minimap2 is claimed.
 * d_n_chains_out[p]: the chains of read p; d_records_out[p * max_chains ..]: their records in rank order -- records at or beyond
 * n_chains are not written.  t_beg / t_end / q_beg / q_end are the row's own oriented coordinates; end_index is the chain's last
 * candidate, from the row's first.  The first record of a read is the chain mgl_sw_select_strand_batch_device picks, where that chain
 * is kept.  Optionally d_ranked_start_out (int64, n + 1) with d_ranked_t_out / _q_out / _len_out (total_cand each; all four or none):
 * every read's kept chains one after the other in rank order, each ascending, n_anchors of each in its record.
 * d_status_out (optional), per read: MGL_SW_ERR_BAD_ARG for a row with d_row_q_len < 1, a row's range of d_cand_start that descends or
 * leaves [0, total_cand], or a pred(i) outside [-1, i) or more than 64 behind i; then MGL_SW_ERR_UNSUPPORTED for a row with more than
 * max_cand candidates.  A refused read has n_chains 0 and nothing else written.  A row whose d_row_status is not 0 contributes no
 * chains and its f / pred are never read.  A read with no kept chain is status 0 with n_chains 0.  The candidates' t, q and l are taken
 * as the chain stage accepted them and f as it wrote them.
 * MGL_SW_ERR_BAD_ARG before any device work for a null required pointer, anchor outputs that are neither all given nor all null,
 * n < 0, n * strands or total_cand above 2^30, strands outside 1, 2, max_cand outside 0 .. 8192, max_chains outside 1 .. 16,
 * min_score < 1, min_cnt < 1 or mask_level outside 1 .. 256; MGL_SW_ERR_DEVICE without a GPU; MGL_SW_ERR_NOMEM where the workspace
 * limit does not hold 4 bytes per read and, with the anchor outputs, 4 bytes per candidate.
 * Device work on `stream`, no synchronisation: sw_rank_chains_kernel (a workgroup per read) and, for the anchor outputs, a prefix sum
 * and sw_rank_pack_kernel.  No MGL_SW_KERNEL_* id: the timing record keeps its fill_kernel.
 */
typedef struct mgl_sw_ranked_chain {
    int32_t score, strand, n_anchors, t_beg, t_end, q_beg, q_end, parent, n_sub, subsc, mapq, end_index;
} mgl_sw_ranked_chain;

int mgl_sw_rank_chains_batch_device(mgl_sw_ctx *ctx, void *stream, int64_t n, int strands, const int32_t *d_row_q_len,
                                    const int64_t *d_cand_start, const int32_t *d_cand_t, const int32_t *d_cand_q, const int32_t *d_cand_len,
                                    int64_t total_cand, const int32_t *d_f, const int32_t *d_pred, const int32_t *d_row_status, int max_cand,
                                    int max_chains, int min_score, int min_cnt, int mask_level, int32_t *d_n_chains_out,
                                    mgl_sw_ranked_chain *d_records_out, int64_t *d_ranked_start_out, int32_t *d_ranked_t_out,
                                    int32_t *d_ranked_q_out, int32_t *d_ranked_len_out, int32_t *d_status_out);

/*
 * ONE ALIGNMENT JOB PER RANKED CHAIN (NOT a reference function; opt-in): behind mgl_sw_rank_chains_batch_device with its anchor outputs,
 * in front of the window, alignment and describe stages, which take the jobs as their pairs.  Defined by tests/lines_textbook.py
 * (expand_chains, oriented); DESIGN.md section 9n.  Read p is d_queries[d_q_start[p] .. + d_q_len[p]) of a buffer of query_bytes; it has
 * d_n_chains[p] records at d_records[p * max_chains ..] and their anchors, one chain behind the other in rank order, at
 * d_ranked_start[p] .. d_ranked_start[p + 1] (int64, n + 1) of d_ranked_t / _q / _len (total_anchors each), and optionally the rank
 * stage's status d_rank_status[p].
 * Every ranked chain c of a read gives one job, in rank order; with keep_secondary = 0 only the chains with parent == c do.  Jobs are
 * numbered densely over the batch in read order: d_job_start_out (int64, n + 1), *d_n_jobs_out = d_job_start_out[n] (one int64 on the
 * device).  mgl_sw_job: read, rank, strand, n_anchors, chain_score (the record's score), chain_parent, q_len, reserved (0).
 * d_job_q_len_out[j] = q_len of the job's read; d_job_q_start_out[j] = q_start of the job's read + strand * query_bytes, an offset into
 * d_oriented_out (2 * query_bytes): its first half gets Q_p at d_q_start[p] for every read with a strand-0 job, its second half rc(Q_p)
 * at query_bytes + d_q_start[p] for every read with a strand-1 job (A <-> T, C <-> G, every other byte as it is, as
 * mgl_sw_select_strand_batch_device complements); no byte of a read without such a job and no byte outside a read is written.
 * d_job_anchor_start_out (int64, job_capacity + 1) is the prefix sum of the jobs' n_anchors and d_job_anchor_t_out / _q_out / _len_out
 * (total_anchors each) hold the jobs' anchors one behind the other, copied: a CSR start array has no gaps, and the ranked arrays have
 * them wherever a chain is skipped or a read refused.  Jobs at or beyond *d_n_jobs_out and below job_capacity are written EMPTY: read
 * -1, every other field 0, q_start 0, q_len 0, no anchors; mgl_sw_locate_window_batch_device (ql < 1) and
 * mgl_sw_align_chain_batch_device (a length below 1) refuse such a pair with MGL_SW_ERR_BAD_ARG, so the stages behind this one run
 * over job_capacity pairs with no count read back.
 * d_status_out (optional), per read, in this order: d_rank_status[p] where that is not 0 (nothing else of the read is read);
 * MGL_SW_ERR_BAD_ARG for q_len < 1, a read that leaves [0, query_bytes), n_chains outside 0 .. max_chains, a record with strand
 * outside 0 / 1 or n_anchors < 1, and a d_ranked_start range that descends, leaves [0, total_anchors] or is not the sum of the read's
 * n_anchors; MGL_SW_ERR_NOMEM by the capacity rule, which is per read and greedy: in index order a read is kept iff the jobs kept so
 * far and its own stay within job_capacity (and the anchors likewise within total_anchors, which only ranges that overlap can
 * exceed); a read that is not kept changes nothing for the reads behind it.  A read with a status has no jobs.
 * MGL_SW_ERR_BAD_ARG before any device work for a null required pointer (d_rank_status and d_status_out are optional), n outside
 * [0, 2^29], max_chains outside 1 .. 16, job_capacity or total_anchors outside [0, 2^30], query_bytes < 0 or above 2^40,
 * keep_secondary outside 0 / 1, and d_oriented_out overlapping d_queries; MGL_SW_ERR_DEVICE without a GPU; MGL_SW_ERR_NOMEM where the
 * workspace limit does not hold 20 bytes per read.  n = 0 is MGL_SW_OK and writes *d_n_jobs_out = 0 and the empty jobs.
 * Device work on `stream`, no synchronisation: sw_expand_count_kernel (a thread per read), sw_expand_scan_kernel (one block),
 * sw_expand_pack_kernel (a wave per read) and sw_expand_orient_kernel (a workgroup per read and strand, 16 bytes a store between the
 * unaligned ends).  No MGL_SW_KERNEL_* id: the timing record keeps its fill_kernel.
 * LIMITS: max_chains <= 16; no hard clips: every job carries the whole read.
 */
typedef struct mgl_sw_job {
    int32_t read, rank, strand, n_anchors, chain_score, chain_parent, q_len, reserved;
} mgl_sw_job;

int mgl_sw_expand_chains_batch_device(mgl_sw_ctx *ctx, void *stream, int64_t n, const uint8_t *d_queries, const int64_t *d_q_start,
                                      const int32_t *d_q_len, int64_t query_bytes, const int32_t *d_rank_status, const int32_t *d_n_chains,
                                      const mgl_sw_ranked_chain *d_records, int max_chains, const int64_t *d_ranked_start,
                                      const int32_t *d_ranked_t, const int32_t *d_ranked_q, const int32_t *d_ranked_len, int64_t total_anchors,
                                      int keep_secondary, int64_t job_capacity, int64_t *d_n_jobs_out, int64_t *d_job_start_out,
                                      mgl_sw_job *d_jobs_out, int64_t *d_job_q_start_out, int32_t *d_job_q_len_out,
                                      int64_t *d_job_anchor_start_out, int32_t *d_job_anchor_t_out, int32_t *d_job_anchor_q_out,
                                      int32_t *d_job_anchor_len_out, uint8_t *d_oriented_out, int32_t *d_status_out);

/*
 * THE LINES OF A READ (NOT a reference function; opt-in): behind mgl_sw_align_chain_batch_device over the jobs of
 * mgl_sw_expand_chains_batch_device.  Defined by tests/lines_textbook.py (classify_alignments); DESIGN.md section 9n.  Read p has the
 * jobs d_job_start[p] .. d_job_start[p + 1] (at most 16); job j has its record d_jobs[j], its alignment d_aln[j] (of which score, q_beg
 * and q_end are read) and d_aln_status[j]; nothing of the alignment of a job with a non-zero status is read.
 * A job is live iff its status is 0, q_end > q_beg and score >= 1.  A read's live jobs ordered by (alignment score descending, rank
 * ascending, job index ascending) are its lines.  A line's interval on the forward read is [q_beg, q_end) on strand 0 and
 * [q_len - q_end, q_len - q_beg) on strand 1.  Parents are found as mgl_sw_rank_chains_batch_device finds them, on these intervals in
 * line order, with mask_level / 256 of the shorter.  flag: 0x10 on strand 1; the first line is the primary; another line that is its
 * own parent gets 0x800 (supplementary); a line with a parent gets 0x100 (secondary).  mapq (0 .. 60) of a line that is its own
 * parent comes from its alignment score, its chain score, its anchors, the number of its secondaries (n_sub), the best alignment
 * score among them (subsc) and that secondary's chain score, in 64-bit integers: minimap2's DP branch, no parity claimed.  A secondary
 * line has mapq, n_sub and subsc 0.
 * d_lines_out[j] (mgl_sw_line), per JOB index so that it lines up with the alignment's, the CIGAR's and the describe stage's rows:
 * order (the line's place among the read's lines), flag, mapq, parent (a job index; the line's own where it is its own parent),
 * n_sub, subsc, fwd_q_beg, fwd_q_end.  A job that is not live has (-1, 0, 0, -1, 0, 0, 0, 0).  Only the jobs of accepted reads get a
 * record: the empty jobs behind the last read's do not.  d_n_lines_out[p]; d_primary_job_out[p]: the job of line 0, -1 for an
 * unmapped read.
 * d_status_out (optional), per read: MGL_SW_ERR_BAD_ARG for a d_job_start range that descends, leaves [0, job_capacity] or is longer
 * than 16, and for a job in it whose `read` is not p; such a read has n_lines 0, primary_job -1 and no record written.
 * MGL_SW_ERR_BAD_ARG before any device work for a null required pointer, n outside [0, 2^29], job_capacity outside [0, 2^30], match
 * or min_score < 1 and mask_level outside 1 .. 256; MGL_SW_ERR_DEVICE without a GPU.  n = 0 is MGL_SW_OK.
 * Device work on `stream`, no synchronisation, no workspace, no LDS: sw_classify_kernel, a quarter wave per read.  No MGL_SW_KERNEL_*
 * id: the timing record keeps its fill_kernel.
 * LIMITS: 16 jobs a read; one window per chain; no supplementary-specific chaining of a clipped remainder.
 */
typedef struct mgl_sw_line {
    int32_t order, flag, mapq, parent, n_sub, subsc, fwd_q_beg, fwd_q_end;
} mgl_sw_line;

int mgl_sw_classify_alignments_batch_device(mgl_sw_ctx *ctx, void *stream, int64_t n, const int64_t *d_job_start, const mgl_sw_job *d_jobs,
                                            int64_t job_capacity, const mgl_sw_chain_alignment *d_aln, const int32_t *d_aln_status, int match,
                                            int min_score, int mask_level, mgl_sw_line *d_lines_out, int32_t *d_n_lines_out,
                                            int32_t *d_primary_job_out, int32_t *d_status_out);

/*
 * DESCRIBING ALIGNMENTS (NOT a reference function; opt-in): behind mgl_sw_align_chain_batch_device or
 * mgl_sw_extend_seed_batch_device, on the same stream, with no copy and no synchronisation in between.  What a SAM or PAF record
 * needs beyond the M / I / D CIGAR: matches, mismatches, inserted and deleted bases and runs, the MD text and the extended (= / X)
 * CIGAR.  Defined by tests/describe_textbook.py; DESIGN.md section 9l.
 * The first ten arguments and (d_cigar, cigar_stride, d_cigar_len) are what those entries took and wrote; mgl_sw_seed_alignment has the
 * layout of mgl_sw_chain_alignment, so the records of either go in.  Of a record only t_beg, t_end, q_beg, q_end are read.  The spans
 * compared are T[t_start + t_beg .. t_start + t_end) and Q[q_start + q_beg .. q_start + q_end), as BYTES: no case folding, no special
 * N -- the kernels only test equality.
 * Counts: n_match / n_mismatch over M columns; n_ins / n_del bases; n_ins_runs / n_del_runs elements.  NM = n_mismatch + n_ins + n_del,
 * a PAF line's block length = n_match + NM.
 * MD (SAM specification): a decimal run of matches, 0 where there is none; a mismatch column gives the TARGET byte and the next run; a
 * D element gives ^, its target bytes and the next run; an I element gives nothing and does not break a run; the text ends with a run
 * (the empty alignment: "0").  Extended CIGAR: every M element split into maximal = and X runs, I and D as they are, adjacent equal
 * operations merged across element borders.
 * flags: MGL_SW_FLAG_BINARY_CIGAR alone is read: the input CIGARs are the binary form those entries write (uint32 len << 4 | op,
 * d_cigar_len in bytes) and the extended CIGAR is written in the same form, = as 7 and X as 8, xcigar_len in bytes; otherwise both
 * are text.  MD is text either way.
 * d_status_in (optional): where d_status_in[p] != 0 nothing of alignment p is read, its record is all zero and d_status_out[p] =
 * d_status_in[p].  Otherwise the alignment is checked before any base is read: 0 <= t_beg <= t_end <= t_len and likewise for q;
 * 0 <= cigar_len <= cigar_stride (binary: a multiple of 4); every element M / I / D with 1 <= len; and the sums of what the elements
 * spend, taken in 64 bits, equal to the two spans.  Anything else is MGL_SW_ERR_BAD_ARG in d_status_out (optional) and an all-zero
 * record, and no access leaves the arrays whatever the slot holds.
 * d_stats_out[p].md_len and .xcigar_len are the lengths NEEDED, also where d_md_out / d_xcigar_out is NULL (a sizing pass).  A text
 * longer than its stride gives MGL_SW_ERR_CIGAR_OVERFLOW: the slot then holds the first md_stride / xcigar_stride bytes of it (whole
 * words in the binary form) and the counts are still right.  Bytes at or beyond a text's length are not written.
 * OVER-READ RULE: the sequences may be read in aligned words.  No byte is read outside the aligned 16-byte blocks that hold a byte of
 * a span, so a span may start and end anywhere in memory the caller owns up to those borders.  (The present kernel reads single bytes
 * and stays inside the spans.)
 * MGL_SW_ERR_BAD_ARG before any device work for n < 0 or above 2^30, a null sequence / start / length / record / CIGAR / d_stats_out
 * pointer, cigar_stride < 1, md_stride < 1 with d_md_out, xcigar_stride < 1 with d_xcigar_out, and with MGL_SW_FLAG_BINARY_CIGAR a
 * cigar_stride or (with d_xcigar_out) xcigar_stride that is no multiple of 4; MGL_SW_ERR_DEVICE without a GPU.  n = 0 is MGL_SW_OK.
 * Device work on `stream`, no synchronisation, no workspace: sw_describe_kernel, one wave per alignment.  No MGL_SW_KERNEL_* id: the
 * timing record keeps its fill_kernel.
 */
typedef struct mgl_sw_alignment_stats {
    int32_t n_match, n_mismatch, n_ins, n_del, n_ins_runs, n_del_runs, md_len, xcigar_len;
} mgl_sw_alignment_stats;

int mgl_sw_describe_alignments_batch_device(mgl_sw_ctx *ctx, void *stream, int64_t n, const uint8_t *d_targets, const int64_t *d_t_start,
                                            const int32_t *d_t_len, const uint8_t *d_queries, const int64_t *d_q_start, const int32_t *d_q_len,
                                            const mgl_sw_chain_alignment *d_aln, const char *d_cigar, int cigar_stride, const int32_t *d_cigar_len,
                                            const int32_t *d_status_in, mgl_sw_alignment_stats *d_stats_out, char *d_md_out, int md_stride,
                                            char *d_xcigar_out, int xcigar_stride, int32_t *d_status_out, int flags);

/*
 * PILING UP ALIGNMENTS (NOT a reference function; opt-in): behind mgl_sw_describe_alignments_batch_device and
 * mgl_sw_classify_alignments_batch_device, on the same stream, with no copy and no synchronisation in between.  What a batch of
 * alignments adds up to per position of the reference: base counts, deleted columns, insertions.  Defined by
 * tests/pileup_textbook.py; DESIGN.md section 9o.
 * The first thirteen arguments are exactly what mgl_sw_describe_alignments_batch_device takes, with its validity rules, its
 * MGL_SW_FLAG_BINARY_CIGAR (the only flag read) and its OVER-READ RULE.  (The present kernel reads no target byte at all.)
 * Alignment p is COUNTED iff d_status_in is NULL or d_status_in[p] == 0, d_select is NULL or d_select[p] != 0, and the alignment
 * passes that entry's per-alignment check.  Nothing of an alignment that is not counted is read beyond its status and select words.
 * An alignment is checked whole before its first add: a refused one adds nothing and gets MGL_SW_ERR_BAD_ARG in d_status_out
 * (optional); a status going in is passed through; a deselected alignment gets 0.
 * Positions: the absolute position of a target column is its byte offset in d_targets, d_t_start[p] + t_beg + i.  The region is
 * [region_beg, region_beg + region_len) in those offsets; columns outside it are skipped, what is inside is still counted.
 * d_counts: eight planes of region_len uint32 each, plane c at c * region_len (channel-major).  The entry ADDS into it: the caller
 * zeroes it, and several batches may accumulate into one table.  Counts wrap modulo 2^32.
 *   planes 0-4: per M column, 1 in the plane of the QUERY byte: A / a 0, C / c 1, G / g 2, T / t 3, every other byte 4;
 *   plane 5:    per column of a D element, 1;
 *   planes 6, 7: per I element of length L, 1 in plane 6 and L in plane 7 at position P - 1, P the absolute position of the next
 *               target-consuming column (the target cursor).  This covers a leading I, a trailing I and an I-only alignment.  A
 *               P - 1 outside the region, -1 included, is not counted; one in front of the alignment's own t_beg or window IS
 *               counted when it lies in the region.
 * MGL_SW_ERR_BAD_ARG before any device work for that entry's own refusals (but there is no d_stats_out and there are no texts),
 * region_beg < 0, region_len outside 1 .. 2^31 - 1 and a null d_counts; MGL_SW_ERR_DEVICE without a GPU.  n = 0 is MGL_SW_OK.
 * Device work on `stream`, no synchronisation, no workspace: sw_pileup_kernel, one wave per alignment, every add a relaxed atomic
 * without return -- integers, so the table is bit-exact whatever the order.  No MGL_SW_KERNEL_* id: the timing record keeps its
 * fill_kernel.
 */
int mgl_sw_pileup_alignments_batch_device(mgl_sw_ctx *ctx, void *stream, int64_t n, const uint8_t *d_targets, const int64_t *d_t_start,
                                          const int32_t *d_t_len, const uint8_t *d_queries, const int64_t *d_q_start, const int32_t *d_q_len,
                                          const mgl_sw_chain_alignment *d_aln, const char *d_cigar, int cigar_stride, const int32_t *d_cigar_len,
                                          const int32_t *d_status_in, const int32_t *d_select, int64_t region_beg, int64_t region_len,
                                          uint32_t *d_counts, int32_t *d_status_out, int flags);

/*
 * CANDIDATE SITES FROM A PILEUP (NOT a reference function; opt-in): what the eight planes of mgl_sw_pileup_alignments_batch_device
 * say per position.  Defined by tests/pileup_textbook.py; DESIGN.md section 9o.
 * Per position i of the region, all arithmetic in 64 bits: depth = the sum of planes 0-5; ref = the channel of
 * d_targets[region_beg + i]; call = the channel 0-5 with the largest count (5 is the deletion), the lowest channel winning a tie;
 * alt = the channel 0-4 other than ref with the largest count, the lowest winning a tie, -1 where that count is 0.
 * flags: 1 (covered) depth >= min_depth; with ok(x) := x >= min_alt and x * 256 >= min_frac * depth: 2 (SNV candidate) covered and
 * ok(alt_count); 4 (deletion) covered and ok(plane 5); 8 (insertion behind this position) covered and ok(plane 6).
 * d_call_out[i] (optional) = "ACGTN*"[call], N where the position is not covered; d_flags_out[i] (optional) = the flags.
 * A SITE is a position with flags & 14.  The sites are written in position order into d_sites_out (mgl_sw_site; pos counts from
 * region_beg; depth, call_count and alt_count clipped to 2^31 - 1), only the first site_capacity of them; d_n_sites_out[0] is the
 * total, those beyond the capacity included, so site_capacity = 0 (d_sites_out may be NULL then) is a sizing pass.
 * MGL_SW_ERR_BAD_ARG before any device work for a null d_counts, d_targets or d_n_sites_out, a null d_sites_out with
 * site_capacity > 0, region_len outside 1 .. 2^31 - 1, region_beg < 0, min_depth < 1, min_alt < 1, min_frac outside 1 .. 256 and
 * site_capacity outside 0 .. 2^30; MGL_SW_ERR_DEVICE without a GPU; MGL_SW_ERR_NOMEM where the workspace limit does not hold 16 bytes
 * per 256 positions and the scan's storage.
 * Device work on `stream`, no synchronisation, one workspace: sw_pileup_flag_kernel (a thread per position), a device-wide scan of
 * the blocks' site counts, sw_pileup_write_kernel.  No MGL_SW_KERNEL_* id: the timing record keeps its fill_kernel.
 */
typedef struct mgl_sw_site {
    int32_t pos, flags, depth, ref, call, call_count, alt, alt_count;
} mgl_sw_site;

int mgl_sw_pileup_sites_device(mgl_sw_ctx *ctx, void *stream, const uint32_t *d_counts, int64_t region_len, const uint8_t *d_targets,
                               int64_t region_beg, int min_depth, int min_alt, int min_frac, uint8_t *d_call_out, uint8_t *d_flags_out,
                               mgl_sw_site *d_sites_out, int64_t site_capacity, int64_t *d_n_sites_out);

/*
 * THE INSERTIONS AT THE SITES (NOT a reference function; opt-in): behind mgl_sw_pileup_sites_device, on the same stream, over the
 * alignments the pileup took.  Which lengths and which bases the insertions behind the candidate sites have.  Defined by
 * tests/calls_textbook.py; DESIGN.md section 9p.
 * The first fifteen arguments are exactly what mgl_sw_pileup_alignments_batch_device takes, with its validity rules, its COUNTED
 * rule, its per-alignment check before the first add, its status passing, its MGL_SW_FLAG_BINARY_CIGAR (the only flag read) and its
 * OVER-READ RULE.  region_beg is that entry's: a site's pos counts from it.
 * THE ACTIVE SITES are the first S = min(max(d_n_sites[0], 0), site_capacity) records of d_sites, read on the device: nothing is read
 * back.  Their pos is taken as strictly ascending, as mgl_sw_pileup_sites_device writes it; the lookup stays inside those S records
 * whatever they hold -- an unsorted list gives unspecified counts, never an access outside the arrays.
 * d_ins: site_capacity rows of W = 6 * max_ins + 1 uint32.  The entry ADDS into it: the caller zeroes it, and several batches may
 * accumulate over one site list.  Counts wrap modulo 2^32.  In row s:
 *   word 0:                        the insertions longer than max_ins;
 *   word L (1 <= L <= max_ins):    the insertions of exactly L bases;
 *   word max_ins + 1 + 5 * j + ch: channel ch (A / a 0, C / c 1, G / g 2, T / t 3, every other byte 4) in column j of the insertions
 *                                  of at most max_ins bases.
 * An I element of length L of a counted alignment stands behind absolute position P - 1 (the pileup's rule) and matches site s iff
 * sites[s].pos == P - 1 - region_beg among the active sites, whatever flags the site has.  A match with L > max_ins adds 1 to word 0;
 * any other match adds 1 to word L and, per inserted base j < L, 1 to its column's channel word; no match adds nothing.
 * MGL_SW_ERR_BAD_ARG before any device work for the pileup entry's own refusals (there is no region_len and no d_counts), max_ins
 * outside 1 .. 64, a null d_sites, d_n_sites or d_ins and site_capacity outside 1 .. 2^30; MGL_SW_ERR_DEVICE without a GPU.  n = 0
 * is MGL_SW_OK.
 * Device work on `stream`, no synchronisation, no workspace: sw_insertions_kernel, one wave per alignment, every add a relaxed atomic
 * without return.  No MGL_SW_KERNEL_* id: the timing record keeps its fill_kernel.
 */
int mgl_sw_pileup_insertions_batch_device(mgl_sw_ctx *ctx, void *stream, int64_t n, const uint8_t *d_targets, const int64_t *d_t_start,
                                          const int32_t *d_t_len, const uint8_t *d_queries, const int64_t *d_q_start, const int32_t *d_q_len,
                                          const mgl_sw_chain_alignment *d_aln, const char *d_cigar, int cigar_stride, const int32_t *d_cigar_len,
                                          const int32_t *d_status_in, const int32_t *d_select, int64_t region_beg, const mgl_sw_site *d_sites,
                                          const int64_t *d_n_sites, int64_t site_capacity, int max_ins, uint32_t *d_ins, int32_t *d_status_out,
                                          int flags);

/*
 * EVENTS, GENOTYPES AND QUALITIES OF THE SITES (NOT a reference function; opt-in): what the planes of
 * mgl_sw_pileup_alignments_batch_device, the sites of mgl_sw_pileup_sites_device and the rows of
 * mgl_sw_pileup_insertions_batch_device (d_ins; NULL: no insertion is called) say per site.  Integers only.  Defined by
 * tests/calls_textbook.py; DESIGN.md section 9p.
 * The active sites are that entry's.  A site whose pos lies outside 0 .. region_len - 1 has no event.  With c[k] the planes at the
 * site's position read unclipped, depth = c[0] + .. + c[5] and ref the channel of d_targets[region_beg + pos], the EVENTS of active
 * site s, in this order:
 *   SNV (kind 1):       flags & 2, ref <= 3 and the site's alt in 0 .. 3.  r = c[ref], a = c[alt], len = 1.
 *   deletion (kind 2):  flags & 4, and site s - 1 is not a deletion site (flags & 4) at pos - 1: the first position of a run.  len =
 *                       the number of consecutive active sites from s with consecutive pos and flags & 4, counted up to max_del; call
 *                       flag 1 where the run goes on beyond max_del (the rest of the run gives no call).  r = c[ref] (plane 4 for
 *                       a reference byte outside ACGT), a = c[5], alt = -1.
 *   insertion (kind 3): flags & 8, d_ins given and some word 1 .. max_ins of row s non-zero.  len = the L with the largest word,
 *                       the smallest on a tie; a = that word, r = max(depth - c[6], 0), alt = -1.
 * THE GENOTYPE, in 64 bits: L0 = r * cost_match + a * cost_error, L1 = (r + a) * cost_het, L2 = a * cost_match + r * cost_error,
 * m = their minimum, PLg = min((Lg - m + 128) >> 8, 2^31 - 1); gt = the lowest g with Lg == m (0 = 0/0, 1 = 0/1, 2 = 1/1);
 * gq = min(99, the smaller PL of the other two); qual = PL0.  The costs are in 1/256 phred per read.  Every event is written, a 0/0
 * one included.
 * The calls are written in site order, inside a site SNV, deletion, insertion, into d_calls_out, only the first call_capacity of
 * them; d_n_calls_out[0] is the total, those beyond the capacity included, so call_capacity = 0 (d_calls_out may be NULL then) is a
 * sizing pass.  depth, ref_count and alt_count are clipped to 2^31 - 1 on the way out only.  d_ins_seq_out (required when d_ins is
 * given and call_capacity > 0, optional otherwise): call_capacity rows of max_ins bytes; the row of a written insertion call gets,
 * per column j < len, "ACGTN"[ch] of the channel with the largest count (the lowest on a tie) and 0 behind; the row of a written call
 * of another kind gets zeros.
 * MGL_SW_ERR_BAD_ARG before any device work for a null d_counts, d_targets, d_sites, d_n_sites or d_n_calls_out, region_len outside
 * 1 .. 2^31 - 1, region_beg < 0, site_capacity outside 1 .. 2^30, max_ins outside 1 .. 64, max_del outside 1 .. 4096, a cost outside
 * 1 .. 2^20 or not cost_match < cost_het < cost_error, call_capacity outside 0 .. 2^30, a null d_calls_out with call_capacity > 0
 * and a null d_ins_seq_out with d_ins and call_capacity > 0; MGL_SW_ERR_DEVICE without a GPU; MGL_SW_ERR_NOMEM where the workspace
 * limit does not hold 16 bytes per 256 site slots and the scan's storage.
 * Device work on `stream`, no synchronisation, one workspace: sw_genotype_count_kernel (a thread per site slot), a device-wide scan
 * of the blocks' event counts, sw_genotype_write_kernel.  No MGL_SW_KERNEL_* id: the timing record keeps its fill_kernel.
 */
typedef struct mgl_sw_call {
    int32_t pos, kind, len, ref, alt, depth, ref_count, alt_count, gt, gq, qual, pl0, pl1, pl2, flags, reserved;
} mgl_sw_call;

int mgl_sw_genotype_sites_device(mgl_sw_ctx *ctx, void *stream, const uint32_t *d_counts, int64_t region_len, const uint8_t *d_targets,
                                 int64_t region_beg, const mgl_sw_site *d_sites, const int64_t *d_n_sites, int64_t site_capacity,
                                 const uint32_t *d_ins, int max_ins, int max_del, int cost_match, int cost_het, int cost_error,
                                 mgl_sw_call *d_calls_out, int64_t call_capacity, int64_t *d_n_calls_out, uint8_t *d_ins_seq_out);

/*
 * Logical backtrack matrix of one pair, the reference's calculateMatrix
 * (sw_scalar.h:7 / sw.cpp:5-146): btr is (tl+1)*(ql+1) int32 row-major with
 * row 0 / column 0 zero, +k = k rows up (deletion run), -k = k columns left
 * (insertion run), 0 = diagonal; *ez as the reference fills it.  Expanded on
 * the GPU from the 4-bit-per-cell device traceback; a parity / debugging
 * entry, not a fast path.
 */
int mgl_sw_backtrack_matrix(const char *t, int tl, const char *q, int ql, int match, int mismatch,
                            int gopen, int gext, int strategy, int32_t *btr, mgl_sw_score *ez);

/*
 * Traceback + CIGAR text from a caller-supplied logical backtrack matrix and
 * ScoreMax: the reference's calculateCigar (sw_scalar.h:8 / sw.cpp:149-255) with
 * n = tl+1, m = ql+1.  The walk runs on the GPU (one lane).
 */
int mgl_sw_cigar_from_backtrack(const int32_t *btr, int tl, int ql, int strategy, const mgl_sw_score *ez,
                                char *cigar, int cigar_cap, int *cigar_len, int *offset);

/*
 * One band of the matrix fill over the caller's arrays: the reference's calculateMatrix_avx (sw_avx.h:7 /
 * sw_avx.cpp:110-322), the stage its driver runs once per band of default_bw = 8 target rows (sw_avx.cpp:71-80).
 * Layouts are the reference's, all host pointers: `target` one base per int32, zero padded to a
 * multiple of default_bw; `query` reversed, query[default_bw + query_length - 1 - j] = q[j], default_bw zeros on each
 * side; `gap` indexed like `query` (vertical run lengths per column); `score` / `step` = H and E of the row above the
 * band for columns 0 .. query_length (on return: of the band's last row); the band's backtrack values go to
 * bcktrack[(query_length + default_bw - 1) * default_bw * band_count + (j - 1 + J) * default_bw + J] for row J of the
 * band and column j -- cells of that region outside the matrix are left as the caller had them (the reference leaves
 * garbage there, and in the padding entries of `gap`; after a band of fewer than default_bw rows -- the last one --
 * `gap` holds the run lengths of the band's last real row where the reference leaves those of its padding rows:
 * nothing reads it any more); ez->mqe / ez->mqe_t are updated with the band's last-column
 * values ('>=': later rows win).  A compatibility entry for callers that drive the band loop themselves (one small
 * kernel and a round trip per band), not a fast path.
 */
int mgl_sw_band_fill(const int32_t *target, int target_length, const int32_t *query, int query_length,
                     int32_t *bcktrack, int band_count, int default_bw, int actual_bw, int32_t *score,
                     int32_t *step, int32_t *gap, int match, int mismatch, int gopen, int gext, int strategy,
                     mgl_sw_score *ez);

/*
 * Same expansion for pair `slot` of the LAST chunk a batch call processed on ctx
 * (slot = pair index when the whole batch fitted one chunk).  The traceback
 * workspace is only valid until the next call on ctx.  tl / ql must be that
 * pair's lengths.  Parity / debugging entry.  MGL_SW_ERR_UNSUPPORTED when the last call ran the
 * checkpointed lane kernel, which stores no traceback (large uniform batches by default:
 * mgl_sw_ctx_set_lane_checkpoint(ctx, 1) before the batch call keeps the flags of every cell).
 */
int mgl_sw_ctx_expand_slot(mgl_sw_ctx *ctx, int64_t slot, int tl, int ql, int32_t *btr);
/* Traceback layout pair `slot` of the last chunk was filled in: 0 = an int32 kernel, 1 = sw_dp16_kernel, 2 =
 * sw_dp16_lane_kernel, 3 = sw_dp_coop16_kernel (which reports 0 for a pair it had to redo in 32 bits).  Tests. */
int mgl_sw_ctx_slot_layout(mgl_sw_ctx *ctx, int64_t slot, int *layout);

/*
 * Host helper for MGL_SW_FLAG_GROUPED_GEOMETRY (no device work, usable without a GPU): a permutation of 0 .. n-1 that
 * puts pairs of equal (t_len, q_len) next to each other.  order_out[0 .. *n_grouped_out) are FULL blocks of eight pairs
 * with one geometry each (a multiple of eight entries: pass them, through the (start, length) arrays of
 * mgl_sw_align_batch_device_indexed / _2bit permuted by order_out, with the flag set); the rest -- fewer than eight
 * pairs per distinct geometry -- follows, sorted by geometry (an ordinary mixed batch, no flag).  O(n) when the lengths
 * span at most 2^22 distinct (t_len, q_len) cells, else O(n log n).
 */
int mgl_sw_group_by_geometry(int64_t n, const int32_t *t_len, const int32_t *q_len, int64_t *order_out, int64_t *n_grouped_out);

#ifdef __cplusplus
}
#endif
#endif /* MGL_SW_H */
