"""Constructed inputs that tests/test_chain_dp_textbook.py (CPU), tests/test_gpu_chain_dp.py (GPU) and scripts/chain_dp_fuzz.py share.
A read is (tl, ql, [(t, q, l)]); parameters are (max_pred, max_dist_t, max_dist_q, bw, pen_gap, pen_skip).  Seeded by the caller: all see
the same numbers."""
import numpy as np

import chain_dp_textbook as tb

CANARY = -0x5A5A5A5B
RING_SIZES = (0, 1, 2, 63, 64, 65, 127, 128, 129, 200)
RING_PREDS = (1, 2, 63, 64)
MINIMAP = (64, 5000, 5000, 500, 38, 0)
RING = (200, 200, 50, 38, 3)  # behind max_pred: what the ring reads are chained with


def random_read(rng, n, spread=40, jitter=6):
    """n candidates of 1 .. 30 bases along a drifting diagonal, in target order up to some disorder: many valid predecessors each, now
    and then an overlap, a step back or a jump off the band"""
    cands, t, d = [], 0, int(rng.integers(0, 50))
    for _ in range(n):
        t = max(0, t + int(rng.integers(-5, spread)))
        d = max(0, d + int(rng.integers(-jitter, jitter + 1)) + (int(rng.integers(-80, 81)) if rng.random() < 0.05 else 0))
        cands.append((t, max(0, t + d - 25), int(rng.integers(1, 31))))
    tl = max([t + l for t, _, l in cands] + [1]) + int(rng.integers(0, 3))
    ql = max([q + l for _, q, l in cands] + [1]) + int(rng.integers(0, 3))
    return tl, ql, cands


def random_params(rng, max_pred=None):
    return (int(max_pred or rng.choice((1, 2, 3, 17, 63, 64))), int(rng.choice((0, 30, 200, 5000))), int(rng.choice((0, 30, 200, 5000))),
            int(rng.choice((0, 1, 7, 50, 500))), int(rng.choice((0, 1, 38, 256, 3000))), int(rng.choice((0, 1, 25, 300))))


def spaced(apart, links, junk=(9000, 0, 1)):
    """`links` + 1 colinear candidates of 10 bases, `apart` indices from one another, all others a junk candidate that can neither
    precede nor follow anything: the chain links candidates exactly `apart` indices apart, or -- max_pred < apart -- nothing"""
    cands = [junk] * (apart * links + 1)
    for m in range(links + 1):
        cands[m * apart] = (100 * m, 100 * m + 3 * m, 10)
    return 9001, 100 * links + 3 * links + 10, cands


# ---- the rule's edges: (name, parameters, read, the pred the textbook must give -- worked out by hand)
EDGE = (64, 40, 30, 12, 100, 1)
A = (0, 0, 20)
RULE_CASES = [
    ("dt at max_dist_t", EDGE, (200, 200, [A, (60, 50, 5)]), [-1, 0]),
    ("dt above max_dist_t", EDGE, (200, 200, [A, (61, 50, 5)]), [-1, -1]),
    ("dq at max_dist_q", EDGE, (200, 200, [A, (58, 50, 5)]), [-1, 0]),
    ("dq above max_dist_q", EDGE, (200, 200, [A, (59, 51, 5)]), [-1, -1]),
    ("dd at bw", EDGE, (200, 200, [A, (50, 38, 5)]), [-1, 0]),
    ("dd above bw", EDGE, (200, 200, [A, (51, 38, 5)]), [-1, -1]),
    ("dd at bw, query ahead", EDGE, (200, 200, [A, (38, 50, 5)]), [-1, 0]),
    ("touching", EDGE, (200, 200, [A, (20, 20, 5)]), [-1, 0]),
    ("overlap by one in t", EDGE, (200, 200, [A, (19, 20, 5)]), [-1, -1]),
    ("overlap by one in q", EDGE, (200, 200, [A, (20, 19, 5)]), [-1, -1]),
    # three hits that overlap on one diagonal are never chained to each other; each gives the fourth 30 (dt = dq = 10, 5, 0: pen 0),
    # a tie that goes to the nearest
    ("overlaps on one diagonal", EDGE, (200, 200, [A, (5, 5, 20), (10, 10, 20), (30, 30, 10)]), [-1, -1, -1, 2]),
    # two predecessors that give the same score: the nearer (larger j)
    ("tie between predecessors", EDGE, (200, 200, [(0, 0, 10), (1, 1, 10), (40, 40, 5)]), [-1, -1, 1]),
    # f(j) + l - pen == l: the predecessor, not the start (f(j) = 1; dt = 1, dq = 2: pen = (256 * 1 >> 8) + (ilog2(2) >> 1) = 1)
    ("tie with the start", (64, 40, 30, 12, 256, 0), (200, 200, [(0, 0, 1), (2, 3, 5)]), [-1, 0]),
    ("start wins by one", (64, 40, 30, 12, 256, 0), (200, 200, [(0, 0, 1), (2, 4, 5)]), [-1, -1]),
    # two chains of the same score: the end is the smaller index
    ("tie for the end", EDGE, (300, 300, [(0, 0, 10), (100, 0, 10), (10, 10, 10), (110, 10, 10)]), [-1, -1, 0, 1]),
    ("no penalties", (64, 1000, 1000, 1000, 0, 0), (3000, 3000, [(0, 0, 5), (900, 10, 5), (1000, 1000, 5), (1005, 2005, 5)]), [-1, 0, 0, 2]),
    # the int32 guard's edge: pen_gap * bw = 2^31 - 1; dd = 1 costs 8388607 and is never worth it, dd = 0 is free
    ("guard edge, pen_gap", (64, 100, 100, 1, (1 << 31) - 1, 0), (300, 300, [(0, 0, 20), (30, 31, 20), (60, 60, 20)]), [-1, -1, 0]),
    ("guard edge, pen_skip", (64, 1000, 1000, 0, 0, 2147483), (3000, 3000, [(0, 0, 20), (1020, 1020, 20), (1040, 1040, 20)]), [-1, -1, 1]),
]
# the ilog2 steps: dd = 0, 1, 2, 3, 4, 7, 8, 15 behind one anchor of 40 (pen_gap = pen_skip = 0: the penalty is the log term alone)
LOG_CASES = [("ilog2 at dd = %d" % dd, (64, 100, 100, 50, 0, 0), (300, 300, [(0, 0, 40), (50 + dd, 50, 5)]), [-1, 0]) for dd in (0, 1, 2, 3, 4, 7, 8, 15)]


def ring_reads(rng, max_pred):
    """the reads of one call at max_pred: every ring size, the 64-apart chain, the only predecessor at max_pred and at max_pred + 1"""
    return [random_read(rng, n) for n in RING_SIZES] + [spaced(64, 2), spaced(max_pred, 2), spaced(max_pred + 1, 2)]


def mixed_batch(rng, max_cand=150):
    """about 40 reads: empty ones at the front, in the middle and at the end, one bad candidate of each kind, lengths below 1, a
    descending range (behind a refused read over the same candidates, so that no two accepted reads share one), a read above
    max_cand.  -> (t_lens, q_lens, cand_start, cand_t, cand_q, cand_len)"""
    reads = [(5, 5, []), (7, 7, [])]
    reads += [random_read(rng, int(rng.integers(1, 90))) for _ in range(8)]
    for kind in range(5):
        tl, ql, c = random_read(rng, 70)
        t, q, l = c[40]
        c[40] = [(t, q, 0), (-1, q, l), (t, -1, l), (tl - l + 1, q, l), (t, ql - l + 1, l)][kind]
        reads.append((tl, ql, c))
    reads += [(9, 9, [])] + [random_read(rng, int(rng.integers(1, 90))) for _ in range(5)]
    tl, ql, c = random_read(rng, 20)
    reads += [(0, ql, c), (tl, 0, c), (tl, ql, c)]
    reads += [random_read(rng, max_cand + 1), random_read(rng, max_cand), (3, 3, []), random_read(rng, 129)]
    reads += [random_read(rng, int(rng.integers(1, 90))) for _ in range(8)] + [(4, 4, []), (4, 4, [])]
    t_lens, q_lens, start, flat = [], [], [0], []
    for tl, ql, c in reads:
        t_lens.append(tl), q_lens.append(ql)
        flat += c
        start.append(len(flat))
    # the descending range: read k (tl = 0, refused) keeps [b, a), a new read k + 1 is [a, b), and the read behind it is [b, ..)
    k = next(i for i, r in enumerate(reads) if r[0] == 0)
    start.insert(k + 2, start[k])
    t_lens.insert(k + 1, 50), q_lens.insert(k + 1, 50)
    # (what was read k + 1, ql = 0 over the next copy of c, is read k + 2 now: [b, its end) -- refused as well; read k + 3 is the good one)
    flat = np.asarray(flat, np.int32).reshape(-1, 3)
    return t_lens, q_lens, start, flat[:, 0].tolist(), flat[:, 1].tolist(), flat[:, 2].tolist()


def csr(reads):
    """[(tl, ql, cands)] -> (t_lens, q_lens, cand_start, cand_t, cand_q, cand_len)"""
    start = [0]
    for _, _, c in reads:
        start.append(start[-1] + len(c))
    flat = [x for _, _, c in reads for x in c]
    return ([r[0] for r in reads], [r[1] for r in reads], start, [x[0] for x in flat], [x[1] for x in flat], [x[2] for x in flat])


def expected(batch, max_cand, params, pad=16):
    """What the entry must leave in output arrays that were CANARY everywhere and `pad` entries longer than their capacity:
    (chain_start, chain_t, chain_q, chain_len, score, f, pred, status) as int64 / int32 arrays"""
    t_lens, q_lens, start, ct, cq, cl = batch
    n, total = len(t_lens), len(ct)
    cs, xt, xq, xl, score, f, pred, status = tb.chain_batch(t_lens, q_lens, start, ct, cq, cl, max_cand, *params)

    def arr(size, values, dtype=np.int32):
        a = np.full(size + pad, CANARY, dtype)
        for i, v in enumerate(values):
            if v is not None:
                a[i] = v
        return a
    return (arr(n + 1, cs, np.int64), arr(total, xt), arr(total, xq), arr(total, xl), arr(n, score), arr(total, f), arr(total, pred), arr(n, status))
