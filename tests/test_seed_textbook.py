"""tests/seed_textbook.py, the definition of mgl_sw_seed_batch_device, against an independent brute-force restatement: the per-window
minimum by definition, the candidates as the maximal runs of covered cells per diagonal; and the properties and edges the definition
states (no GPU)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_dp_textbook as ctb  # noqa: E402
import seed_cases as cases  # noqa: E402
import seed_textbook as tb  # noqa: E402
from mgl_amd import synth  # noqa: E402

DIGIT = bytes.maketrans(b"ACGT", b"0123")
CHAINING = (64, 1000, 1000, 500, 38, 0)  # DESIGN 9g's: max_pred, max_dist_t, max_dist_q, bw, pen_gap, pen_skip


def brute_hash(key):
    with np.errstate(over="ignore"):
        h = np.uint32(key) ^ np.uint32(0x9E3779B9)
        h ^= h >> np.uint32(16)
        h *= np.uint32(0x85EBCA6B)
        h ^= h >> np.uint32(13)
        h *= np.uint32(0xC2B2AE35)
        h ^= h >> np.uint32(16)
    return int(h)


def brute_sketch(seq, k, w):
    """{position: key}"""
    nk = len(seq) - k + 1
    if nk < 1:
        return {}
    key = {i: int(seq[i:i + k].translate(DIGIT), 4) for i in range(nk) if not seq[i:i + k].strip(b"ACGT")}
    order = {i: (brute_hash(x), i) for i, x in key.items()}
    windows = [range(a, a + w) for a in range(nk - w + 1)] if nk >= w else [range(nk)]
    picked = {min(order[i] for i in win if i in order)[1] for win in windows if any(i in order for i in win)}
    return {i: key[i] for i in picked}


def brute(T, Q, k, w, max_occ, merge):
    """-> (candidates, raw hits), both sorted"""
    ts, qs = brute_sketch(T, k, w), brute_sketch(Q, k, w)
    occ = {}
    for x in qs.values():
        occ[x] = occ.get(x, 0) + 1
    raw = sorted((t, q, k) for t, x in ts.items() for q, y in qs.items() if x == y and occ[x] <= max_occ)
    if not merge:
        return raw, raw
    cells = {(t + j, q + j) for t, q, _ in raw for j in range(k)}
    runs = []
    for a, b in cells:
        if (a - 1, b - 1) not in cells:
            n = 1
            while (a + n, b + n) in cells:
                n += 1
            runs.append((a, b, n))
    return sorted(runs), raw


def check_properties(T, Q, r, k):
    assert r.status == 0
    for t, q, l in r.cands:
        assert l >= k and 0 <= t and t + l <= len(T) and 0 <= q and q + l <= len(Q) and T[t:t + l] == Q[q:q + l]  # an exact match inside both
        assert not T[t:t + l].strip(b"ACGT")
    assert all(a[:2] < b[:2] for a, b in zip(r.cands, r.cands[1:]))  # strictly ascending in (t, q)
    assert sorted(r.raw) == r.raw and len(set(r.raw)) == len(r.raw)


def both(T, Q, k, w, max_occ):
    for merge in (0, 1):
        r = tb.seed_pair(T, Q, k, w, max_occ, merge, 8192)
        if len(T) < 1 or len(Q) < 1:
            assert r.status == tb.BAD_ARG and not r.cands
            continue
        want, raw = brute(T, Q, k, w, max_occ, merge)
        assert r.cands == want and r.raw == raw, (k, w, max_occ, merge)
        check_properties(T, Q, r, k)
    return r


def test_hash_and_key():
    assert tb.fmix32(0) == 0 and tb.fmix32(1) == 0x514E28B7  # murmur3's finaliser
    assert tb.kmers(b"ACGT", 4) == [0b00011011] and tb.kmers(b"TTTTTTTTTTTTTTTT", 16) == [0xFFFFFFFF]
    assert tb.kmers(b"GACGTACGTACGTACGT", 16)[0] >> 31 == 1  # k = 16: the first base in the top bits
    assert tb.kmers(b"ACNTA", 2) == [1, None, None, 12] and tb.kmers(b"acgt", 2) == [None] * 3
    for key in (0, 1, 0x80000000, 0xFFFFFFFF, 12345):
        assert tb.kmer_hash(key) == brute_hash(key)


def test_random_pairs_every_k_and_w():
    seen = set()
    for name, (k, w, occ), T, Q in cases.random_cases():
        both(T, Q, k, w, occ)
        seen.add((k, w))
    assert seen == {(k, w) for k in cases.K_ALL for w in cases.W_ALL}


def test_edge_cases_against_the_brute_force():
    for name, (k, w, occ), T, Q in cases.edge_cases():
        both(T, Q, k, w, occ)


def test_lengths_around_k_and_the_window():
    k, w = 6, 5
    s = cases.rand_seq(np.random.default_rng(1), 30)
    assert tb.sketch(s[:k - 1], k, w) == [] and len(tb.sketch(s[:k], k, w)) == 1
    for n in (k + 1, k + w - 2):  # fewer positions than w: the one window [0, nk)
        assert len(tb.sketch(s[:n], k, w)) == 1
    assert len(tb.sketch(s[:k + w - 1], k, w)) == 1 and 1 <= len(tb.sketch(s[:k + w], k, w)) <= 2  # one window, two windows
    assert tb.seed_pair(b"", s, k, w, 8, 1, 64).status == tb.BAD_ARG and tb.seed_pair(s, b"", k, w, 8, 1, 64).status == tb.BAD_ARG


def test_ties_go_to_the_smallest_position_and_max_occ_counts_the_querys_sketch():
    # a homopolymer: every window's minimum is its first position, so the sketch is every window start
    assert [i for i, _ in tb.sketch(b"A" * 40, 6, 4)] == list(range(40 - 6 + 1 - 4 + 1))
    nq = 37 - 6 + 1 - 4 + 1
    assert tb.seed_pair(b"A" * 40, b"A" * 37, 6, 4, nq - 1, 0, 8192).raw == []
    assert len(tb.seed_pair(b"A" * 40, b"A" * 37, 6, 4, nq, 0, 8192).raw) == 32 * nq
    by_name = {name: (p, T, Q) for name, p, T, Q in cases.edge_cases()}
    at5 = lambda T, Q, k, w, occ: sum(t == 5 for t, _, _ in tb.seed_pair(T, Q, k, w, occ, 0, 8192).raw)  # noqa: E731  (the k-mer lies at T[5 ..])
    (k, w, occ), T, Q = by_name["occ3of3"]
    assert at5(T, Q, k, w, occ) == 3 and at5(T, Q, k, w, occ - 1) == 0
    (k, w, occ), T, Q = by_name["occ4of3"]
    assert at5(T, Q, k, w, occ) == 0 and at5(T, Q, k, w, occ + 1) == 4


def test_merge_joins_overlapping_and_touching_hits_only():
    for d, joined in ((7, True), (8, True), (9, False)):
        T, Q = cases.gap_pair(d)
        r = tb.seed_pair(T, Q, 8, 12, 8, 1, 8192)
        diag = [t for t, q, _ in r.raw if t == q]
        a = next(a for a, b in zip(diag, diag[1:]) if b - a == d)
        run = next((t, l) for t, q, l in r.cands if t == q and t <= a < t + l)
        assert (run[0] + run[1] >= a + d + 8) == joined
    by_name = {name: (p, T, Q) for name, p, T, Q in cases.edge_cases()}
    (k, w, occ), T, Q = by_name["interleaved"]
    r = tb.seed_pair(T, Q, k, w, occ, 1, 8192)
    assert r.cands == [(0, 0, 60), (20, 60, 20)]
    assert [t - q for t, q, _ in r.raw[20:24]] == [0, -40, 0, -40]  # the two diagonals alternate in (t, q) order


def test_the_bounds_on_raw_hits_and_on_the_querys_sketch():
    rng = np.random.default_rng(3)
    T, Q = cases.rand_seq(rng, 200, b"AC"), cases.rand_seq(rng, 200, b"AC")
    R = len(tb.seed_pair(T, Q, 4, 1, 64, 1, 8192).raw)
    assert R > 1000
    at, over = tb.seed_pair(T, Q, 4, 1, 64, 1, R), tb.seed_pair(T, Q, 4, 1, 64, 1, R - 1)
    assert at.status == 0 and at.cands and over.status == tb.UNSUPPORTED and over.cands == []
    assert len(at.cands) < R  # the bound is on the raw hits, not on the merged candidates
    q = cases.rand_seq(rng, tb.MAX_QUERY_SEEDS + 16)
    fits, not_ = tb.seed_pair(q[:50], q[:-1], 16, 1, 8, 1, 8192), tb.seed_pair(q[:50], q, 16, 1, 8, 1, 8192)
    assert fits.status == 0 and fits.query_seeds == 8192 and fits.cands == [(0, 0, 50)]
    assert not_.status == tb.UNSUPPORTED and not_.query_seeds == 8193 and not_.cands == []


def test_the_capacity_rule():
    rng = np.random.default_rng(4)
    s = [cases.rand_seq(rng, 40) for _ in range(4)]
    #     two candidates,         none,            refused,   one,          none,                       one,         refused, none
    Ts = [s[0] + b"N" + s[1], s[2], b"", s[3], s[0], s[1], b"", s[2]]
    Qs = [s[0] + s[1], s[3], s[0], s[3], s[1], s[1], s[1], s[0]]
    run = lambda cap: tb.seed_batch(Ts, Qs, 8, 1, 8, 1, 256, cap)  # noqa: E731
    start, ct, cq, cl, st = run(4)  # a fit to the last entry
    assert start == [0, 2, 2, 2, 3, 3, 4, 4, 4] and st == [0, 0, 1, 0, 0, 0, 1, 0] and len(ct) == len(cq) == len(cl) == 4
    assert run(1 << 30)[0] == start
    start, ct, cq, cl, st = run(3)  # one short: pair 5 is P*, the empty pair behind it is cut too, the refused one keeps its status
    assert start == [0, 2, 2, 2, 3, 3, 3, 3, 3] and st == [0, 0, 1, 0, 0, 3, 1, 3] and len(ct) == 3
    start, ct, cq, cl, st = run(2)
    assert start == [0, 2, 2, 2, 2, 2, 2, 2, 2] and st == [0, 0, 1, 3, 3, 3, 1, 3]
    start, ct, cq, cl, st = run(0)  # nothing fits: every pair from the first on
    assert start == [0] * 9 and st == [3, 3, 1, 3, 3, 3, 1, 3] and ct == []
    assert tb.seed_batch([s[2]], [s[3]], 8, 1, 8, 1, 256, 0) == ([0, 0], [], [], [], [0])  # an empty pair fits a capacity of 0


@pytest.mark.parametrize("k,w", [(15, 10), (11, 5)])
def test_the_chains_of_seeded_pairs_span_their_windows(k, w):
    pairs = synth.chain_pairs(11, 16, length=2000)
    for T, Q, _ in pairs:
        r = tb.seed_pair(T, Q, k, w, 8, 1, 4096)
        check_properties(T, Q, r, k)
        c = ctb.chain_dp(len(T), len(Q), r.cands, *CHAINING)
        assert c.status == 0 and c.chain[0][0] <= 200 and c.chain[-1][0] + c.chain[-1][2] >= len(T) - 200
