"""tests/chain_textbook.py against what it is composed of and against independent checks: K = 1 is the seed extension, a gap's CIGAR is
the banded textbook's under INDEL, a gap's score at a full band is a three-matrix global DP written here, the joined CIGAR re-scored
gives the record's score, reversing both sequences keeps score and spans, every degenerate gap, and a drifting pair that one seed at
band 64 loses and the chain follows."""
import numpy as np
import pytest

import banded_textbook as bt
import chain_textbook as ct
from chain_cases import chain_pair
import extend_adaptive_cases as cases
import extend_textbook as et
import seed_extend_textbook as stb

GATK = cases.GATK
PARAM_SETS = [GATK, (3, -1, 4, 3), (1, -4, 6, 1)]


def global_affine(t, q, match, mismatch, gopen, gext):
    """the global alignment score of t and q with affine gaps: three matrices, nothing shared with the textbooks"""
    match, mismatch, o, e = abs(match), -abs(mismatch), abs(gopen), abs(gext)
    NEG = -10 ** 15
    n, m = len(t), len(q)
    M = [[NEG] * (m + 1) for _ in range(n + 1)]
    X = [[NEG] * (m + 1) for _ in range(n + 1)]  # ends in a deletion (a target base against nothing)
    Y = [[NEG] * (m + 1) for _ in range(n + 1)]  # ends in an insertion
    M[0][0] = 0
    for i in range(1, n + 1):
        X[i][0] = -o - (i - 1) * e
    for j in range(1, m + 1):
        Y[0][j] = -o - (j - 1) * e
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            s = match if t[i - 1] == q[j - 1] else mismatch
            M[i][j] = max(M[i - 1][j - 1], X[i - 1][j - 1], Y[i - 1][j - 1]) + s
            X[i][j] = max(max(M[i - 1][j], Y[i - 1][j]) - o, X[i - 1][j] - e)
            Y[i][j] = max(max(M[i][j - 1], X[i][j - 1]) - o, Y[i][j - 1] - e)
    return max(M[n][m], X[n][m], Y[n][m])


def test_one_anchor_is_the_seed_extension():
    rng = np.random.default_rng(3)
    n = 0
    for flanks in ((0, 0, 0, 0), (5, 0, 0, 4), (0, 3, 2, 0), (40, 38, 70, 73), (65, 64, 1, 1), (130, 127, 64, 66)):
        for sl in (1, 20):
            T, Q, anchors = chain_pair(rng, flanks, [], [sl], exact=n % 3 != 0)
            for band, zdrop, to_qend, adaptive in ((0, -1, False, False), (8, 520, True, False), (31, -1, True, True), (200, 2000, False, True)):
                params = PARAM_SETS[n % 3]
                aln, cigar, left, right, gaps = ct.chain_align(T, Q, anchors, *params, band, zdrop, to_qend, adaptive)
                want = stb.seed_extend(T, Q, anchors[0], *params, band, zdrop, to_qend, adaptive)
                assert (tuple(aln), cigar, left, right) == (tuple(want[0]), want[1], want[2], want[3]) and gaps == [0]
                assert aln._fields == stb.SeedAln._fields[:5] + ("anchor_score",) + stb.SeedAln._fields[6:]
                n += 1


GAPS = [(1, 1), (1, 65), (65, 1), (63, 64), (64, 64), (65, 63), (129, 63), (30, 129), (17, 17)]


def test_a_gap_is_the_banded_textbook_under_indel_plus_the_corner():
    rng = np.random.default_rng(4)
    for n, (gt, gq) in enumerate(GAPS):
        t, q = cases.noisy_pair(rng, gt, gq, b"AC" if n % 3 == 0 else b"ACGT")
        for params in PARAM_SETS:
            for band in (0, 1, 31, 200):
                score, cigar = ct.gap_fill(t, q, *params, band)
                off, _, want = bt.banded_align(t, q, *params, bt.INDEL, band)
                off2, _, want2 = bt.banded_align_np(t, q, *params, bt.INDEL, band)
                assert off == off2 == 0 and cigar == want == want2
                assert et.cigar_score(cigar, t, q, *params) == score
                if band >= max(gt, gq):
                    assert score == global_affine(t, q, *params), (gt, gq, params, band)
                else:
                    assert score <= global_affine(t, q, *params)


def test_degenerate_gaps_and_their_scores():
    o, e = GATK[2], GATK[3]
    assert ct.gap_fill(b"", b"", *GATK, 5) == (0, "")
    assert ct.gap_fill(b"", b"ACG", *GATK, 5) == (-(o + 2 * e), "3I")
    assert ct.gap_fill(b"ACGTA", b"", *GATK, 0) == (-(o + 4 * e), "5D")
    assert ct.gap_fill(b"A", b"", *GATK, 0) == (-o, "1D")
    # anchors of one base, every kind of gap between them, an anchor at each edge of the window and the query
    T, Q = b"ACGTACGTAC", b"ACTACGGGTA"
    anchors = [(0, 0, 1), (1, 1, 1), (2, 2, 1), (4, 3, 1), (5, 4, 2), (7, 9, 1)]  # gaps 0/0, 0/0, 1/0, 0/0, 0/3, then the right side
    aln, cigar, left, right, gaps = ct.chain_align(T, Q, anchors, *GATK, 3, -1)
    assert gaps == [0, 0, -o, 0, -(o + 2 * e), 0]
    assert cigar.startswith("3M1D3M3I1M") and (aln.t_beg, aln.q_beg) == (0, 0) and left == stb.EMPTY_QUERY_FLANK
    assert aln.anchor_score == sum(200 if T[st] == Q[sq] else -150 for st, sq, sl in anchors for st, sq in [(st + k, sq + k) for k in range(sl)])
    # the last anchor ends the query: the right side is the empty extension; and one that ends the window alone
    aln, cigar, left, right, gaps = ct.chain_align(T, Q, [(0, 0, 2), (6, 8, 2)], *GATK, 3, -1)
    assert right == stb.EMPTY_QUERY_FLANK and (aln.t_end, aln.q_end) == (8, 10)
    aln, cigar, left, right, gaps = ct.chain_align(T, Q[:6], [(0, 0, 2), (8, 3, 2)], *GATK, 3, -1)
    assert right == stb.EMPTY_TARGET_FLANK and (aln.t_end, aln.q_end) == (10, 5)


def _sweep():
    rng = np.random.default_rng(5)
    out = []
    for n in range(24):
        k = (1, 2, 3, 5)[n % 4]
        gaps = [GAPS[(n + 2 * x) % len(GAPS)] if (n + x) % 4 else ((0, 0), (0, 3), (4, 0))[x % 3] for x in range(k - 1)]
        lens = [(1, 20)[(n + x) & 1] for x in range(k)]
        flanks = ((0, 0, 0, 0), (1, 1, 64, 65), (65, 63, 0, 2), (40, 44, 70, 66))[n % 4]
        out.append(chain_pair(rng, flanks, gaps, lens, exact=n % 5 != 0))
    return out


def test_the_joined_cigar_rescored_is_the_score_and_spends_the_spans():
    for n, (T, Q, anchors) in enumerate(_sweep()):
        params = PARAM_SETS[n % 3]
        for band, zdrop, to_qend, adaptive in ((0, -1, False, False), (31, 3 * params[2], True, n % 2 == 1), (200, -1, True, False)):
            aln, cigar, left, right, gaps = ct.chain_align(T, Q, anchors, *params, band, zdrop, to_qend, adaptive)
            t, q = T[aln.t_beg:aln.t_end], Q[aln.q_beg:aln.q_end]
            assert et.cigar_spans(cigar) == (len(t), len(q))
            assert et.cigar_score(cigar, t, q, *params) == aln.score
            ops = [op for _, op in stb.elements(cigar)]
            assert all(a != b for a, b in zip(ops, ops[1:])) and set(ops) <= set("MID")
            assert len(gaps) == len(anchors) and gaps[-1] == 0


def test_reversing_both_sequences_keeps_the_score_and_mirrors_the_spans():
    """Only the score and the spans: among equally good paths the walk prefers the diagonal, then the insertion, from the END of a
    segment, so a gap's (and a side's) CIGAR may differ on ties when the sequences are reversed.  At a band that covers every gap and
    with the Z-drop off, a side of the mirrored pair is the other side of the pair, and every gap's corner is the optimum either way."""
    for n, (T, Q, anchors) in enumerate(_sweep()):
        params = PARAM_SETS[n % 3]
        aln, *_ = ct.chain_align(T, Q, anchors, *params, 400, -1, True)
        rev, *_ = ct.chain_align(T[::-1], Q[::-1], ct.mirror_anchors(len(T), len(Q), anchors), *params, 400, -1, True)
        assert rev.score == aln.score and rev.anchor_score == aln.anchor_score
        assert (rev.t_beg, rev.t_end, rev.q_beg, rev.q_end) == (len(T) - aln.t_end, len(T) - aln.t_beg, len(Q) - aln.q_end, len(Q) - aln.q_beg)


def kmer_chain(t, q, every=200, sl=20):
    """anchors of sl bases about every `every` bases of q: exact copies with one occurrence in t, kept where they are colinear"""
    anchors = []
    for p in range(every // 2, len(q) - sl, every):
        u = t.find(q[p:p + sl])
        if u >= 0 and t.find(q[p:p + sl], u + 1) < 0 and (not anchors or (u >= anchors[-1][0] + sl and p >= anchors[-1][1] + sl)):
            anchors.append((u, p, sl))
    return anchors


@pytest.mark.parametrize("name", ("deletions", "insertions"))
def test_a_drifting_pair_that_one_seed_at_band_64_loses_and_the_chain_follows(name):
    t, q = cases.drift_pairs()[name]  # ten indels of 20 bases: the path ends 200 diagonals away
    anchors = kmer_chain(t, q)
    assert len(anchors) >= 12
    aln, cigar, left, right, gaps = ct.chain_align(t, q, anchors, *GATK, 64, -1, True)
    o, e = GATK[2], GATK[3]
    assert (aln.t_beg, aln.t_end, aln.q_beg, aln.q_end) == (0, len(t), 0, len(q))
    assert aln.score == 200 * min(len(t), len(q)) - 10 * (o + 19 * e) and sum(1 for _, op in stb.elements(cigar) if op != "M") == 10
    seed, *_ = stb.seed_extend(t, q, anchors[len(anchors) // 2], *GATK, 64, -1, True)
    assert seed.score < aln.score - 100000
