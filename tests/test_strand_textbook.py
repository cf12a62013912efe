"""tests/strand_textbook.py against what it is built on: the reverse complement, the rows of seed_strands_batch against
seed_textbook.seed_batch, and the choice of the strand -- on pairs with known chains of which every odd read is given reverse-complemented
the textbook finds the true strand of every read."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seed_cases as cases  # noqa: E402
import seed_textbook as tb  # noqa: E402
import strand_textbook as stb  # noqa: E402
from mgl_amd import synth  # noqa: E402

CHAINING = (64, 1000, 1000, 500, 38, 0)  # max_pred, max_dist_t, max_dist_q, bw, pen_gap, pen_skip


def test_revcomp_twice_is_the_identity_and_keeps_what_is_no_base():
    rng = np.random.default_rng(1)
    for n in (0, 1, 2, 17, 300):
        b = bytes(rng.integers(0, 256, n, dtype=np.uint8))
        assert stb.revcomp(stb.revcomp(b)) == b and synth.revcomp(b) == stb.revcomp(b)
        s = cases.rand_seq(rng, n, b"ACGTNacgtn-")
        assert stb.revcomp(stb.revcomp(s)) == s and synth.revcomp(s) == stb.revcomp(s)
    assert stb.revcomp(b"AACGTNacgtX") == b"XtgcaNACGTT"
    # a k-mer that is not valid stays so at its mirrored place
    s = b"ACGTNACGTTacGT"
    fwd, rev = tb.kmers(s, 4), tb.kmers(stb.revcomp(s), 4)
    assert [x is None for x in fwd] == [x is None for x in rev[::-1]]


def test_the_even_rows_are_the_one_strand_textbooks():
    groups = cases.by_params(cases.edge_cases() + cases.random_cases())
    for params, group in list(groups.items())[::5]:
        Ts, Qs = [T for _, T, _ in group], [Q for _, _, Q in group]
        for merge in (0, 1):
            start, ct, cq, cl, status, t_len, q_len = stb.seed_strands_batch(Ts, Qs, *params, merge, 4096, 1 << 30)
            one = tb.seed_batch(Ts, Qs, *params, merge, 4096, 1 << 30)
            assert len(start) == 2 * len(Ts) + 1 and t_len == [len(T) for T in Ts for _ in (0, 1)] and q_len == t_len[:0] + [len(Q) for Q in Qs for _ in (0, 1)]
            for p in range(len(Ts)):
                a, b, c, d = start[2 * p], start[2 * p + 1], one[0][p], one[0][p + 1]
                assert (ct[a:b], cq[a:b], cl[a:b], status[2 * p]) == (one[1][c:d], one[2][c:d], one[3][c:d], one[4][p])
    # the odd row is the even row of the reverse-complemented read
    T, Q = cases.rand_seq(np.random.default_rng(2), 80), cases.rand_seq(np.random.default_rng(3), 60)
    T = T + stb.revcomp(Q)[10:50]
    a = stb.seed_strands_batch([T], [Q], 8, 3, 8, 1, 256, 1 << 30)
    b = stb.seed_strands_batch([T], [stb.revcomp(Q)], 8, 3, 8, 1, 256, 1 << 30)
    assert a[0][2] - a[0][1] > 0 and [x[a[0][1]:a[0][2]] for x in a[1:4]] == [x[b[0][0]:b[0][1]] for x in b[1:4]]


@functools.lru_cache(maxsize=None)
def stranded_pairs():
    """synth.chain_pairs(11, 16, length=2000) with every odd read replaced by its reverse complement -> (Ts, Qs as given, true strands)"""
    pairs = synth.chain_pairs(11, 16, length=2000)
    Ts = [p[0] for p in pairs]
    Qs = [synth.revcomp(p[1]) if i % 2 else p[1] for i, p in enumerate(pairs)]
    return Ts, Qs, [i % 2 for i in range(len(pairs))]


def choose(Ts, Qs, k, w):
    seeded = stb.seed_strands_batch(Ts, Qs, k, w, 8, 1, 2048, 1 << 30)
    chained = stb.chain_rows(seeded, 2048, *CHAINING)
    data, off = b"".join(Qs), np.cumsum([0] + [len(Q) for Q in Qs])
    return seeded, chained, stb.select_strand(data, off[:-1], [len(Q) for Q in Qs], *chained[:5])


@pytest.mark.parametrize("k,w", [(15, 10), (11, 5)])
def test_the_true_strand_on_16_of_16(k, w):
    Ts, Qs, truth = stranded_pairs()
    seeded, chained, (strand, out, start, at, aq, al, score, status) = choose(Ts, Qs, k, w)
    scores = chained[4]
    print("true rows", sorted(scores[2 * p + s] for p, s in enumerate(truth)), "wrong rows", sorted(scores[2 * p + 1 - s] for p, s in enumerate(truth)))
    assert strand == truth and status == [0] * 16 and seeded[4] == [0] * 32 and chained[7] == [0] * 32
    pairs = synth.chain_pairs(11, 16, length=2000)
    assert out == b"".join(p[1] for p in pairs)  # every read comes out on the window's strand
    for p in range(16):
        r = 2 * p + truth[p]
        assert score[p] == scores[r] and (at[start[p]:start[p + 1]], aq[start[p]:start[p + 1]]) == (chained[1][chained[0][r]:chained[0][r + 1]],
                                                                                                   chained[2][chained[0][r]:chained[0][r + 1]])


def test_ties_and_reads_without_a_chain_are_strand_0():
    x = cases.rand_seq(np.random.default_rng(4), 150)
    own = x + stb.revcomp(x)  # its own reverse complement: the rows are equal, the scores tie
    other = cases.rand_seq(np.random.default_rng(5), 200)
    none = cases.rand_seq(np.random.default_rng(6), 120)  # unrelated to its window: chains on neither row
    assert stb.revcomp(own) == own
    _, chained, (strand, out, start, at, aq, al, score, status) = choose([own, other, none + b"N" + other], [own, none, stb.revcomp(other)], 11, 5)
    assert chained[4][0] == chained[4][1] > 100 and chained[4][2] == chained[4][3] == 0
    assert strand == [0, 0, 1] and status == [0, 0, 0] and score == [chained[4][0], 0, chained[4][5]]
    assert start[1] - start[0] == chained[0][1] - chained[0][0] and start[2] == start[1] and start[3] > start[2]
    assert out == own + none + other


def test_refused_pairs_of_the_choice():
    q = b"ACGTTGCA" + b"GGGA"
    cs = [0, 1, 1, 1, 2, 2, 1, 3, 3]  # pair 2: a descending range; pair 3: fine again
    ct, cq, cl, sc = [1, 2, 3, 4], [0, 0, 0, 0], [4, 4, 4, 4], [9, 7, 5, 6, 1, 1, 2, 0]
    got = stb.select_strand(q, [0, 8, 8, 8], [8, 4, 4, 4], cs, ct, cq, cl, sc, total_chain=3)
    # pair 0: row 0; pair 1: row 3, one anchor; pair 2: refused; pair 3: K = 2 on row 6 against none on row 7
    assert got[0] == [0, 1, 0, 0] and got[7] == [0, 0, 1, 0] and got[2] == [0, 1, 2, 2, 4] and got[3] == [1, 2, 2, 3] and got[6] == [9, 6, 0, 2]
    assert got[1] == q[:8] + q[8:]  # (pair 1's TCCC came first and pair 3's GGGA over it: overlapping reads are the caller's error)
    got = stb.select_strand(q, [0, 9, -1], [0, 4, 4], [0, 1, 1, 1, 2, 2, 2], ct, cq, cl, [5, 0, 0, 5, 0, 0])
    assert got[7] == [1, 1, 1] and got[0] == [0, 0, 0] and got[2] == [0, 0, 0, 0] and got[1] == bytes(12)
