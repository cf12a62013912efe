"""Constructed inputs that tests/test_rank_textbook.py (CPU), tests/test_gpu_rank_chains.py (GPU) and scripts/rank_fuzz.py share.
A row is (ql, [(t, q, l)], f, pred, row_status); a read is a list of `strands` rows; a batch is (strands, row_q_len, cand_start, cand_t,
cand_q, cand_len, f, pred, row_status); parameters are (max_cand, max_chains, min_score, min_cnt, mask_level).  Seeded by the caller: all
see the same numbers."""
import functools

import numpy as np

import chain_dp_cases as dpc
import chain_dp_textbook as ctb
import rank_textbook as rtb

CANARY = dpc.CANARY
POISON = 0x7F7F7F7F  # what the f / pred of a row the chain stage refused hold in the tests: never read
SEAM_SIZES = (0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4095, 4096, 4097, 8192)  # the ballot, sort and LDS seams
DEFAULTS = (4096, 4, 40, 3, 128)


def row(ql, items, status=0):
    """[(t, q, l, f, pred)] -> a row"""
    return (ql, [tuple(x[:3]) for x in items], [x[3] for x in items], [x[4] for x in items], status)


def forest_row(rng, n, roots=0.1, lo=-3, hi=25, status=0):
    """n candidates along a drifting diagonal with a made-up f and pred: a forest in which many candidates share a predecessor (so walks
    stop at used candidates), gains of lo .. hi - 1 (so f ties, and falls now and then), predecessors up to 64 behind"""
    cands, f, pred, t, d = [], [], [], 0, int(rng.integers(0, 40))
    for i in range(n):
        t += int(rng.integers(1, 40))
        d = max(0, d + int(rng.integers(-4, 5)))
        l = int(rng.integers(1, 31))
        cands.append((t, t + d, l))
        p = -1 if i == 0 or rng.random() < roots else i - int(rng.integers(1, min(i, 64) + 1))
        pred.append(p)
        f.append(l if p < 0 else f[p] + int(rng.integers(lo, hi)))
    ql = max([q + l for _, q, l in cands] + [1]) + int(rng.integers(0, 3))
    return (ql, cands, f, pred, status)


def dp_row(rng, n, params=(64, 200, 200, 50, 38, 3)):
    """a row as the chain stage leaves it: chain_dp_cases.random_read chained by the textbook"""
    tl, ql, cands = dpc.random_read(rng, n, spread=int(rng.choice((3, 40, 300))), jitter=int(rng.choice((0, 6, 40))))
    r = ctb.chain_dp(tl, ql, cands, *params)
    return (ql, [tuple(c) for c in cands], r.f, r.pred, 0)


def line_row(n, ql=None):
    """one chain of n anchors: the walk of N steps"""
    return (ql or 10 * n + 10, [(10 * i, 10 * i, 5) for i in range(n)], [5 * (i + 1) for i in range(n)], [i - 1 for i in range(n)], 0)


def singles_row(n):
    """n chains of one anchor each, all of them kept at min_cnt = 1, scores 40 + (i * 7) % 23: ties, and no order in the indices"""
    return (20 * n + 20, [(20 * i, 20 * i, 10) for i in range(n)], [40 + (i * 7) % 23 for i in range(n)], [-1] * n, 0)


def batch(reads, strands):
    """[[row] * strands] -> a batch"""
    ql, start, ct, cq, cl, f, pred, st = [], [0], [], [], [], [], [], []
    for rd in reads:
        assert len(rd) == strands
        for q, cands, rf, rp, rs in rd:
            ql.append(q), st.append(rs)
            for (t, qq, l), x, y in zip(cands, rf, rp):
                ct.append(t), cq.append(qq), cl.append(l), f.append(x), pred.append(y)
            start.append(len(ct))
    return (strands, ql, start, ct, cq, cl, f, pred, st)


def textbook(b, params, row_status=True):
    strands, ql, start, ct, cq, cl, f, pred, st = b
    return rtb.rank_batch(strands, ql, start, ct, cq, cl, f, pred, st if row_status else None, *params)


def expected(b, params, pad=16, row_status=True):
    """What the entry must leave in output arrays that were CANARY everywhere and `pad` entries longer than their capacity:
    (n_chains, records [n * max_chains * 12], ranked_start, ranked_t, ranked_q, ranked_len, status)"""
    n, total, max_chains = len(b[1]) // b[0], len(b[3]), params[1]
    nc, recs, rs, rt, rq, rl, status = textbook(b, params, row_status)

    def arr(size, values, dtype=np.int32):
        a = np.full(size + pad, CANARY, dtype)
        a[:len(values)] = values
        return a
    rec = np.full((n * max_chains + pad) * 12, CANARY, np.int32)
    for p, chains in enumerate(recs):
        for c, r in enumerate(chains):
            at = (p * max_chains + c) * 12
            rec[at:at + 12] = r
    return (arr(n, nc), rec, arr(n + 1, rs, np.int64), arr(total, rt), arr(total, rq), arr(total, rl), arr(n, status))


# ---- hand cases: (name, strands, the read's rows, (min_score, min_cnt, mask_level), the chains the textbook must give at max_chains = 16 as
# (score, strand, end_index, K, parent, n_sub, subsc) -- worked out by hand)
def _c(i, f, pred, q=None, l=10, t=None):
    return (100 * i if t is None else t, 100 * i if q is None else q, l, f, pred)


PREFIX = [_c(0, 10, -1), _c(1, 20, 0), _c(2, 30, 1), _c(3, 28, 1, q=250), _c(4, 38, 3)]
ONE = [_c(0, 10, -1), _c(1, 20, 0), _c(2, 40, 1)]
HAND = [
    # 4 -> 3 -> 1 -> 0 first (38); then 2 stops at the used 1: 30 - 20 = 10 with its own anchor alone.  On the read they overlap in [200, 210):
    # 10 of min(410, 10), so the second is the first's secondary
    ("shared prefix", 1, [row(500, PREFIX)], (10, 1, 128), [(38, 0, 4, 4, 0, 1, 10), (10, 0, 2, 1, 0, 0, 0)]),
    # min_cnt = 2 drops the chain of 2 alone; 5 (f = 25, pred 2) then stops at 2 at once: 25 - 30 < 5.  Had 2 been freed, 5 -> 2 would stop at
    # 1 with 25 - 20 = 5 and K = 2: kept
    ("a dropped chain's anchors stay used", 1, [row(700, PREFIX + [_c(5, 25, 2)])], (5, 2, 128), [(38, 0, 4, 4, 0, 0, 0)]),
    ("score = min_score", 1, [row(300, ONE)], (40, 3, 128), [(40, 0, 2, 3, 0, 0, 0)]),
    ("score = min_score - 1", 1, [row(300, ONE)], (41, 3, 128), []),
    ("K = min_cnt - 1", 1, [row(300, ONE)], (40, 4, 128), []),
    # 2 (f = 39 < 40) ends the visit; had it been walked it would stop at the used 0 with 39 - -5 = 44: kept
    ("the visit ends at f < min_score", 1, [row(300, [_c(0, -5, -1), _c(1, 50, 0), _c(2, 39, 0, q=150)])], (40, 1, 128), [(50, 0, 1, 2, 0, 0, 0)]),
    # 1 and 2 both hold 50 and both follow 0: the smaller index walks first and takes 0 with it
    ("equal f: the smaller index first", 1, [row(400, [_c(0, 20, -1), _c(1, 50, 0), _c(2, 50, 0, q=300, t=5000)])], (30, 1, 128),
     [(50, 0, 1, 2, 0, 0, 0), (30, 0, 2, 1, 1, 0, 0)]),
    # the same chain on both rows: strand 0 ranks first; 1000 - 210 .. 1000 - 0 does not meet 0 .. 210
    ("equal scores across strands", 2, [row(1000, ONE), row(1000, ONE)], (40, 3, 128), [(40, 0, 2, 3, 0, 0, 0), (40, 1, 2, 3, 1, 0, 0)]),
    # [0, 100) and [50, 150): 50 * 256 = 128 * 100
    ("ov * 256 = mask_level * minlen", 1, [row(500, [_c(0, 100, -1, q=0, l=100), _c(1, 90, -1, q=50, l=100, t=5000)])], (40, 1, 128),
     [(100, 0, 0, 1, 0, 1, 90), (90, 0, 1, 1, 0, 0, 0)]),
    ("ov * 256 one below", 1, [row(500, [_c(0, 100, -1, q=0, l=100), _c(1, 90, -1, q=51, l=100, t=5000)])], (40, 1, 128),
     [(100, 0, 0, 1, 0, 0, 0), (90, 0, 1, 1, 1, 0, 0)]),
    # strand 1's [900, 1000) is [0, 100) on the forward read
    ("strand 1 flipped", 2, [row(1000, [_c(0, 100, -1, q=0, l=100)]), row(1000, [_c(0, 90, -1, q=900, l=100)])], (40, 1, 128),
     [(100, 0, 0, 1, 0, 1, 90), (90, 1, 0, 1, 0, 0, 0)]),
    ("strand 1 at the same q does not overlap", 2, [row(1000, [_c(0, 100, -1, q=0, l=100)]), row(1000, [_c(0, 90, -1, q=0, l=100)])], (40, 1, 128),
     [(100, 0, 0, 1, 0, 0, 0), (90, 1, 0, 1, 1, 0, 0)]),
    ("n_sub = 3", 1, [row(500, [_c(0, 100, -1, q=0, l=100)] + [_c(i, 100 - 10 * i, -1, q=0, l=100, t=3000 * i) for i in (1, 2, 3)])], (40, 1, 128),
     [(100, 0, 0, 1, 0, 3, 90), (90, 0, 1, 1, 0, 0, 0), (80, 0, 2, 1, 0, 0, 0), (70, 0, 3, 1, 0, 0, 0)]),
    ("the first fitting primary is rank 1", 1,
     [row(500, [_c(0, 100, -1, q=0, l=100), _c(1, 90, -1, q=200, l=100, t=3000), _c(2, 80, -1, q=210, l=100, t=6000)])], (40, 1, 128),
     [(100, 0, 0, 1, 0, 0, 0), (90, 0, 1, 1, 1, 1, 80), (80, 0, 2, 1, 1, 0, 0)]),
]
MAPQ_TABLE = [((1000, 40, 50, 0), 60), ((1000, 900, 50, 1), 24), ((1000, 1000, 50, 1), 0), ((100, 40, 3, 0), 32), ((15, 1, 1, 0), 10), ((9000, 8500, 45, 3), 14)]

# ---- refusals: (name, strands, rows, max_cand, expected status); the ranges are the batch's own, see mixed_batch for the range cases
GOOD = row(300, ONE)
BAD_PREDS = [("pred = i", [-1, 1, 1]), ("pred > i", [-1, 2, 1]), ("pred < -1", [-1, -2, 1]), ("pred 65 behind", None)]


def bad_pred_row(kind):
    name, pred = BAD_PREDS[kind]
    if pred is not None:
        return (300, GOOD[1], GOOD[2], pred, 0)
    r = line_row(70)
    return (r[0], r[1], r[2], r[3][:69] + [4], 0)  # 69 - 4 = 65


def refusals():
    out = [("ql = 0", 1, [row(0, ONE)], 10, rtb.BAD_ARG), ("ql = 0 on strand 1", 2, [GOOD, row(0, ONE)], 10, rtb.BAD_ARG),
           ("above max_cand", 1, [GOOD], 2, rtb.UNSUPPORTED), ("at max_cand", 1, [GOOD], 3, 0),
           ("above max_cand on a row with a status", 2, [GOOD, row(300, ONE, status=5)], 2, rtb.UNSUPPORTED),
           ("64 behind", 1, [(lambda r: (r[0], r[1], r[2], r[3][:69] + [5], 0))(line_row(70))], 100, 0)]
    out += [(BAD_PREDS[k][0], 1, [bad_pred_row(k)], 100, rtb.BAD_ARG) for k in range(4)]
    out += [("a bad pred before max_cand", 1, [bad_pred_row(0)], 2, rtb.BAD_ARG),
            ("a bad pred behind a status is not read", 2, [GOOD, (300, GOOD[1], [POISON] * 3, [POISON] * 3, 1)], 10, 0)]
    return out


def mixed_batch(rng, strands=2, max_cand=150):
    """39 reads (40 on one strand): empty ones at the front, in the middle and at the end, a bad pred of each kind, ql = 0, a descending range, a row above
    max_cand, a row with a status whose f / pred hold poison.  -> a batch"""
    def read(*rows_):
        rows_ = list(rows_)[:strands]
        return rows_ + [(rows_[0][0], [], [], [], 0)] * (strands - len(rows_))
    some = lambda: forest_row(rng, int(rng.integers(1, 120)))  # noqa: E731
    empty = (9, [], [], [], 0)
    reads = [read(empty, empty), read(empty, empty)]
    reads += [read(some(), some()) for _ in range(6)]
    reads += [read(some(), bad_pred_row(k)) if strands == 2 else read(bad_pred_row(k)) for k in range(4)]
    reads += [read(empty, empty)]
    reads += [read(dp_row(rng, int(rng.integers(1, 150))), dp_row(rng, int(rng.integers(1, 150)))) for _ in range(5)]
    reads += [read(some(), (-3, *some()[1:])), read((0, *some()[1:]), some())]
    marker = len(reads)  # the descending range goes in front of this read
    reads += [read(some(), some()), read(forest_row(rng, max_cand + 1), some()), read(some(), forest_row(rng, max_cand)), read(some(), empty)]
    poisoned = forest_row(rng, 60)
    reads += [read((poisoned[0], poisoned[1], [POISON] * 60, [POISON] * 60, 5), some()), read(some(), (poisoned[0], poisoned[1], [POISON] * 60, [-7] * 60, 1))]
    reads += [read(singles_row(40), singles_row(33)), read(line_row(100), some())]
    reads += [read(some(), some()) for _ in range(37 - len(reads))]
    reads += [read(empty, empty)]
    strands_, ql, start, ct, cq, cl, f, pred, st = batch(reads, strands)
    # the descending range: two new rows in front of read `marker`, [b, a) and [a, b), over the candidates of the read in front of them,
    # which is refused (ql = 0), so that no two accepted reads share a candidate.  Two strands: one new read, refused for its first row.
    # One strand: two new reads, the first refused, the second a good one.  The read behind them starts at b as before
    r = marker * strands
    a, b = start[r - strands], start[r]
    start[r + 1:r + 1] = [a, b]
    ql[r:r] = [50, 50]
    st[r:r] = [0, 0]
    assert len(ql) == (78 if strands == 2 else 40) and len(start) == len(ql) + 1 and a < b
    return (strands_, ql, start, ct, cq, cl, f, pred, st)


@functools.lru_cache(maxsize=None)
def repeat_set(divergence):
    """section 9k's reads: mapping_set(11, 8, 2000, 3000) with the first 4 windows appended as copies"""
    from mgl_amd import synth

    return synth.repeat_mapping_set(11, 8, length=2000, spacer=3000, copies=4, divergence=divergence)


K, W = 15, 10
RANKING = dict(max_chains=4, min_score=40, min_cnt=3, mask_level=128)


@functools.lru_cache(maxsize=None)
def repeat_mapped(divergence, extra=()):
    """the textbook composition over those reads (and `extra` ones behind them) -> (ref, reads, truth, copy, index_textbook.map_reads'
    tuple, rank_batch's tuple)"""
    import index_cases as ic
    import index_textbook as itb

    ref, reads, truth, copy = repeat_set(divergence)
    reads = list(reads) + list(extra)
    c, s = ic.CHAINING, ic.SEEDING
    got = itb.map_reads(itb.build_index(ref, K, W), len(ref), reads, K, W, 2, s["max_occ"], s["max_occ_ref"], s["merge"], s["max_cand"],
                        2 * len(reads) * s["max_cand"], c["max_pred"], c["max_dist"], c["max_dist"], c["bw"], c["pen_gap"], c["pen_skip"], ic.SLACK, ic.MAX_TL)
    seeded, chained = got[0], got[1]
    ranked = rtb.rank_batch(2, seeded[6], seeded[0], seeded[1], seeded[2], seeded[3], chained[5], chained[6], chained[7], s["max_cand"], RANKING["max_chains"],
                            RANKING["min_score"], RANKING["min_cnt"], RANKING["mask_level"])
    return ref, reads, truth, copy, got, ranked
