"""Pins the local Smith-Waterman checker itself (tests/local_textbook.py) -- no GPU: a brute force over substring pairs, CIGAR replay,
hand-built ties, the two textbook forms against each other, and the mirror of kernel A's range guard at its edges."""
import itertools
import random

import numpy as np

import local_textbook as lt

AA = b"ARNDCQEGHILKMFPSTWYV"


def _blosum():
    from mgl_amd import protein

    return protein.blosum62()


def _gotoh_global(t, q, code, matrix, o, e):
    """Best global affine score of t against q (both may be empty), the three-state textbook form."""
    NEG = -(1 << 40)
    tl, ql = len(t), len(q)
    M = [[NEG] * (ql + 1) for _ in range(tl + 1)]
    X = [[NEG] * (ql + 1) for _ in range(tl + 1)]  # ends in D (consumes target)
    Y = [[NEG] * (ql + 1) for _ in range(tl + 1)]  # ends in I
    M[0][0] = 0
    for i in range(tl + 1):
        for j in range(ql + 1):
            if i and j:
                M[i][j] = max(M[i - 1][j - 1], X[i - 1][j - 1], Y[i - 1][j - 1]) + int(matrix[code[t[i - 1]]][code[q[j - 1]]])
            if i:
                X[i][j] = max(M[i - 1][j] - o, Y[i - 1][j] - o, X[i - 1][j] - e)
            if j:
                Y[i][j] = max(M[i][j - 1] - o, X[i][j - 1] - o, Y[i][j - 1] - e)
    return max(M[tl][ql], X[tl][ql], Y[tl][ql])


def test_score_equals_brute_force_over_substrings():
    code, mat = _blosum()
    rng = random.Random(3)
    for _ in range(150):
        t = bytes(rng.choice(AA[:6]) for _ in range(rng.randint(0, 6)))
        q = bytes(rng.choice(AA[:6]) for _ in range(rng.randint(0, 6)))
        for o, e in [(11, 1), (3, 1), (2, 2), (1, 0), (0, 0)]:
            best = 0
            for a, b in itertools.combinations(range(len(t) + 1), 2):
                for c, d in itertools.combinations(range(len(q) + 1), 2):
                    best = max(best, _gotoh_global(t[a:b], q[c:d], code, mat, o, e))
            assert lt.local_align(t, q, code, mat, o, e)[0] == best, (t, q, o, e)


def test_cigars_replay_to_the_score_and_coordinates():
    code, mat = _blosum()
    rng = random.Random(4)
    for _ in range(300):
        t = bytes(rng.choice(AA) for _ in range(rng.randint(0, 40)))
        q = bytes(rng.choice(AA) for _ in range(rng.randint(0, 40)))
        if rng.random() < 0.5 and t:
            q = t[rng.randint(0, len(t) - 1):][: 30] + q[:5]
        for o, e in [(11, 1), (10, 2), (5, 5), (9, 0), (0, 0)]:
            sc, tb, te, qb, qe, cg = lt.local_align(t, q, code, mat, o, e)
            if sc == 0:
                assert (tb, te, qb, qe, cg) == (0, 0, 0, 0, "")
                continue
            assert lt.replay(t, q, code, mat, o, e, tb, qb, cg) == (sc, te, qe)


def test_end_is_the_smallest_cell_row_first():
    code, mat = lt.dna_matrix(1, -1)
    # "A" against "AA": H[1][1] == H[1][2] == 1 -> the end is (1, 1)
    assert lt.local_align(b"A", b"AA", code, mat, 5, 1)[:5] == (1, 0, 1, 0, 1)
    # "AA" against "A": H[1][1] == H[2][1] == 1 -> (1, 1) (row first)
    assert lt.local_align(b"AA", b"A", code, mat, 5, 1)[:5] == (1, 0, 1, 0, 1)
    # two equal islands: the one in the smaller row wins, even at a larger column
    assert lt.local_align(b"CCGG", b"GGCC", code, mat, 9, 9) == (2, 0, 2, 2, 4, "2M")


def test_walk_stops_at_zero():
    code, mat = lt.dna_matrix(1, -1)
    # 'CA' vs 'GA': the walk from the A/A cell meets H == 0 on the diagonal: one M, begins (1, 1)
    assert lt.local_align(b"CA", b"GA", code, mat, 5, 1) == (1, 1, 2, 1, 2, "1M")
    # a mismatch between matches that the prefix pays for: AAAA C AAAA -> the walk crosses it
    r = lt.local_align(b"AAAACAAAA", b"AAAAGAAAA", code, mat, 5, 1)
    assert r == (7, 0, 9, 0, 9, "9M")


def test_extension_wins_ties_and_zero_penalties():
    code, mat = lt.dna_matrix(2, -3)
    # o == e: opening again and extending cost the same -> extension wins: one run of 2D, not 1D1D (same CIGAR text); the begin is
    # found through the extension chain
    r = lt.local_align(b"AAAACCAAAA", b"AAAAAAAA", code, mat, 2, 2)
    assert r[0] == 12 and r[5] == "4M2D4M"
    # o == 0, e == 0: gaps are free, the best path gathers every match
    r = lt.local_align(b"ACGTACGT", b"AGAG", code, mat, 0, 0)
    assert r[0] == 8 and lt.replay(b"ACGTACGT", b"AGAG", code, mat, 0, 0, r[1], r[3], r[5]) == (8, r[2], r[4])
    # e == 0: one long gap costs o
    r = lt.local_align(b"AAAAAGGGGGGGGGGAAAAA", b"AAAAAAAAAA", code, mat, 3, 0)
    assert r[0] == 17 and r[5] == "5M10D5M"


def test_the_two_textbook_forms_agree():
    code, mat = _blosum()
    rng = random.Random(5)
    amat = np.random.default_rng(5).integers(-7, 9, size=(32, 32)).astype(np.int8)
    acode = (np.arange(256) % 32).astype(np.uint8)
    for _ in range(120):
        t = bytes(rng.choice(AA) for _ in range(rng.randint(0, 60)))
        q = bytes(rng.choice(AA) for _ in range(rng.randint(0, 60)))
        for c, m in ((code, mat), (acode, amat)):
            for o, e in [(11, 1), (10, 2), (5, 5), (9, 0), (0, 0), (1, 4)]:
                assert lt.local_align(t, q, c, m, o, e) == lt.local_align_np(t, q, c, m, o, e), (t, q, o, e)


def test_tile_scores_equal_the_plain_form():
    """local_scores_np (one target, all queries of a tile at once) against local_align(): random protein, random bytes under an
    asymmetric matrix, and tied DNA repeats; empty queries and an empty target among them; the six gap models of the test above."""
    code, mat = _blosum()
    rng = random.Random(6)
    amat = np.random.default_rng(6).integers(-7, 9, size=(32, 32)).astype(np.int8)
    acode = (np.arange(256) % 32).astype(np.uint8)
    dcode, dmat = lt.dna_matrix(1, -1)
    pairs = 0
    for r in range(42):
        if r % 3 == 0:
            c, m = code, mat
            t = bytes(rng.choice(AA) for _ in range(rng.randint(0, 50)))
            qs = [bytes(rng.choice(AA) for _ in range(rng.randint(0, 50))) for _ in range(5)] + [t[rng.randint(0, 20):][:40], b"", t]
        elif r % 3 == 1:
            c, m = acode, amat
            t = bytes(rng.randrange(256) for _ in range(rng.randint(1, 50)))
            qs = [bytes(rng.randrange(256) for _ in range(rng.randint(0, 50))) for _ in range(6)] + [b"", t[::-1]]
        else:
            c, m = dcode, dmat
            t = b"ACGT" * rng.randint(1, 12) + b"A" * rng.randint(0, 9)
            qs = [b"ACGT" * rng.randint(1, 9), b"A" * rng.randint(1, 12), b"", b"GTAC" * 3 + b"N" * 14 + b"GTAC" * 3, b"ACGGT" * 4, b"T"]
        if r == 41:
            t = b""
        for o, e in [(11, 1), (10, 2), (5, 5), (9, 0), (0, 0), (1, 4)]:
            got = lt.local_scores_np(t, qs, c, m, o, e)
            assert got.dtype == np.int64 and got.tolist() == [lt.local_align(t, q, c, m, o, e)[0] for q in qs], (t, qs, o, e)
        pairs += len(qs)
    assert pairs >= 250
    assert lt.local_scores_np(b"ACGT", [], dcode, dmat, 5, 1).shape == (0,)
    assert lt.local_scores_np(b"ACGT", [b"", b""], dcode, dmat, 5, 1).tolist() == [0, 0]


def test_top_k_orders_ties_by_database_index():
    s = np.array([[5, 9, 9, 1, 9], [0, 0, 0, 0, 0]])
    assert lt.top_k(s, 3).tolist() == [[1, 2, 4], [0, 1, 2]]


def test_range_guard_mirror_edges():
    ok = lt.local_lane_ok
    # the profile byte: S + K with K = max(0, -min S)
    assert ok(-128, 127, 11, 1, 100, 100)  # 127 + 128 = 255: every int8 matrix fits a byte
    assert ok(5, 127, 11, 1, 100, 100) and lt.local_lane_bias(5) == 0 and lt.local_lane_bias(-4) == 4
    # 16 bits: max(S) * min(tl, ql) + 255 <= 65535
    assert ok(-4, 11, 11, 1, 5934, 5934) and not ok(-4, 11, 11, 1, 5935, 5935)
    assert ok(-8, 120, 11, 1, 520, 520) and not ok(-8, 127, 11, 1, 520, 520)
    assert ok(-8, 127, 11, 1, 514, 10000) and not ok(-8, 127, 11, 1, 515, 10000)
    assert ok(-8, 127, 11, 1, 10000, 514) and not ok(-8, 127, 11, 1, 10000, 515)
    assert ok(-8, -1, 11, 1, 30000, 30000)  # no positive score: H stays 0
    # the gap constants
    assert ok(-4, 11, 65535, 1, 100, 100) and not ok(-4, 11, 65536, 1, 100, 100) and not ok(-4, 11, 1, 65536, 100, 100)
    # the LDS carve: 256 + 1024 + 33 * 32 + the target's codes (strips of 32, to 16 bytes) within 64 KiB
    limit_tl = (65536 - 256 - 1024 - 33 * 32) // 32 * 32
    assert ok(-4, 1, 11, 1, limit_tl, 1) and not ok(-4, 1, 11, 1, limit_tl + 1, 1)
    assert lt.local_lane_lds_bytes(limit_tl) <= 65536 < lt.local_lane_lds_bytes(limit_tl + 1)
    # empty bounds never take kernel A
    assert not ok(-4, 11, 11, 1, 0, 10) and not ok(-4, 11, 11, 1, 10, 0)


def test_range_guard_mirror_matches_the_header():
    """The numbers local_textbook.py mirrors are the ones sw_local.h defines."""
    import os
    import re

    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mgl_amd", "csrc", "sw_local.h")).read()
    assert re.search(r"LOCAL_LANE_R = %d;" % lt.LOCAL_LANE_R, src)
    assert re.search(r"LOCAL_LANE_LDS_LIMIT = 64 \* 1024;", src) and lt.LOCAL_LANE_LDS_LIMIT == 64 * 1024
    assert "* lo + 255 > 65535" in src and "smax + k > 255" in src and "gopen > 65535 || gext > 65535" in src
