"""The extension textbook (tests/extend_textbook.py) without a GPU: the plain and the row-wise forms agree; with the band and the Z-drop
rule out of the way the scores are those of an independent three-matrix Gotoh global alignment over every prefix pair and the CIGAR
re-scores to what is reported; the last-column result is the golden records' mqe where GATK's borders are gap penalties; the Z-drop
rule cuts where it must and its gap term matters; the mirrored slot formula stands where mgl_amd/csrc/sw_extend.h puts it."""
import os
import random
import re

import extend_textbook as et
import golden_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_CELLS = 6000
GATK = (200, -150, 260, 11)
PARAM_SETS = [GATK, (25, -50, 110, 6), (10, -15, 30, 5), (3, -1, 4, 3), (1, -1, 1, 1), (1, -4, 6, 1), (5, -4, 10, 1)]
INDEL, LEADING_INDEL = 2, 4


def _small(suite, every=1):
    return [g for k, g in enumerate(golden_io.load(suite)) if k % every == 0 and len(g.t) * len(g.q) <= MAX_CELLS]


RECORDS = _small("tiny", 7) + _small("ties") + _small("shapes") + _small("random") + _small("known")


def _rand_pair(rng, tl, ql, alphabet=b"ACGT"):
    t = bytes(rng.choice(alphabet) for _ in range(tl))
    q = bytearray()
    for ch in t:
        r = rng.random()
        if r < 0.05:
            continue
        if r < 0.10:
            q.append(rng.choice(alphabet))
        q.append(rng.choice(alphabet) if rng.random() < 0.08 else ch)
    q = bytes(q[:ql]) + bytes(rng.choice(alphabet) for _ in range(max(0, ql - len(q))))
    return t, q


def test_plain_form_equals_the_row_wise_form_on_every_output():
    rng = random.Random(11)
    cases = [(g.t, g.q, g.params) for g in RECORDS]
    for _ in range(1500):
        tl, ql = rng.randint(1, 90), rng.randint(1, 90)
        cases.append(_rand_pair(rng, tl, ql, b"AC" if rng.random() < 0.3 else b"ACGT") + (rng.choice(PARAM_SETS),))
    assert len(cases) > 2500
    dropped = cut_by_band = qend = 0
    for t, q, params in cases:
        band = rng.choice((0, 1, 2, 5, 17, 64, max(len(t), len(q)), 1000))
        zdrop = rng.choice((-1, 0, params[3], 3 * params[2], 40 * params[0], 1 << 30))
        to_qend = rng.random() < 0.5
        a = et.extend_align(t, q, *params, band, zdrop, to_qend)
        b = et.extend_align_np(t, q, *params, band, zdrop, to_qend)
        assert a == b, (t, q, params, band, zdrop, to_qend, a, b)
        ext, cigar = a
        assert et.cigar_spans(cigar) == ((ext.t_end_qend, len(q)) if ext.cigar_from else (ext.t_end, ext.q_end))
        assert ext.score >= 0 and 0 <= ext.rows_done <= len(t) and ext.dropped == (ext.rows_done < len(t)) and (zdrop >= 0 or not ext.dropped)
        dropped += ext.dropped
        cut_by_band += len(t) > len(q) + band
        qend += ext.cigar_from
    assert dropped > 200 and cut_by_band > 50 and qend > 300


def _gotoh_prefix_scores(t, q, match, mismatch, gopen, gext):
    """G[i][j]: the score of the best global alignment of t[:i] and q[:j], three matrices (match / gap in the query / gap in the
    target), written from the textbook recurrence with no tie rule in it."""
    m, x, o, e = abs(match), -abs(mismatch), abs(gopen), abs(gext)
    inf = float("-inf")
    tl, ql = len(t), len(q)
    M = [[inf] * (ql + 1) for _ in range(tl + 1)]
    D = [[inf] * (ql + 1) for _ in range(tl + 1)]  # ends with a target base against a gap
    I = [[inf] * (ql + 1) for _ in range(tl + 1)]  # ends with a query base against a gap
    M[0][0] = 0
    for i in range(tl + 1):
        for j in range(ql + 1):
            if i > 0 and j > 0:
                M[i][j] = max(M[i - 1][j - 1], D[i - 1][j - 1], I[i - 1][j - 1]) + (m if t[i - 1] == q[j - 1] else x)
            if i > 0:
                D[i][j] = max(max(M[i - 1][j], I[i - 1][j]) - o, D[i - 1][j] - e)
            if j > 0:
                I[i][j] = max(max(M[i][j - 1], D[i][j - 1]) - o, I[i][j - 1] - e)
    return [[max(M[i][j], D[i][j], I[i][j]) for j in range(ql + 1)] for i in range(tl + 1)]


def test_full_band_without_zdrop_is_the_best_global_prefix_alignment():
    rng = random.Random(3)
    cases = [(g.t, g.q, g.params) for g in RECORDS[::9] if len(g.t) * len(g.q) <= 2500]
    for _ in range(150):
        cases.append(_rand_pair(rng, rng.randint(1, 40), rng.randint(1, 40), b"AC" if rng.random() < 0.4 else b"ACGT") + (rng.choice(PARAM_SETS),))
    assert len(cases) > 250
    nonempty = 0
    for t, q, params in cases:
        tl, ql = len(t), len(q)
        G = _gotoh_prefix_scores(t, q, *params)
        want = max((G[i][j], -i, -j) for i in range(tl + 1) for j in range(ql + 1))  # the smallest (i, j) in row-major order among the largest
        want_qend = max(G[i][ql] for i in range(1, tl + 1))
        for to_qend in (False, True):
            for f in (et.extend_align, et.extend_align_np):
                ext, cigar = f(t, q, *params, max(tl, ql), -1, to_qend)
                assert (ext.score, ext.t_end, ext.q_end) == (want[0], -want[1], -want[2]), (t, q, params, ext)
                assert ext.score_qend == want_qend and G[ext.t_end_qend][ql] == want_qend
                assert all(G[i][ql] < want_qend for i in range(ext.t_end_qend + 1, tl + 1))  # the later row among equals
                assert (ext.rows_done, ext.dropped, ext.cigar_from) == (tl, 0, int(to_qend))
                ti, qi, sc = (ext.t_end_qend, ql, ext.score_qend) if to_qend else (ext.t_end, ext.q_end, ext.score)
                assert et.cigar_spans(cigar) == (ti, qi)
                assert et.cigar_score(cigar, t, q, *params) == sc, (t, q, params, cigar, sc)
                nonempty += cigar != ""
    assert nonempty > 500


def test_last_column_result_is_the_golden_mqe_where_the_borders_are_gap_penalties():
    """INDEL and LEADING_INDEL give GATK's matrix the gap-penalty borders of the anchored start, and its mqe scan is the last column's
    with `>=`: the same cells, the same order."""
    recs = [g for g in RECORDS if g.strategy in (INDEL, LEADING_INDEL)]
    assert len(recs) > 300 and {g.strategy for g in recs} == {INDEL, LEADING_INDEL}
    for g in recs:
        ext, _ = et.extend_align(g.t, g.q, *g.params, max(len(g.t), len(g.q)), -1)
        assert (ext.score_qend, ext.t_end_qend) == (g.score[0], g.score[1]), (g, ext)


def test_a_zdrop_of_at_least_the_score_range_is_off():
    rng = random.Random(5)
    for _ in range(300):
        t, q = _rand_pair(rng, rng.randint(1, 70), rng.randint(1, 70))
        params = rng.choice(PARAM_SETS)
        band = rng.choice((0, 3, 20, 100))
        m, x, o, e = et.normalize(*params)
        span = max(m, -x) * min(len(t), len(q)) + 2 * o + e * max(len(t), len(q))  # the range of every finite H
        if len(t) > len(q) + band:
            continue  # (a row without cells drops whenever the rule is on)
        off = et.extend_align(t, q, *params, band, -1)
        assert et.extend_align(t, q, *params, band, span) == off
        assert et.extend_align_np(t, q, *params, band, 1 << 30) == off


def test_matching_prefix_then_unrelated_tails_drops_and_equals_the_truncated_target():
    rng = random.Random(9)
    seen = 0
    for p in (1, 5, 40, 63, 64, 65, 100):
        for params in PARAM_SETS:
            m, x, o, e = et.normalize(*params)
            core = bytes(rng.choice(b"ACGT") for _ in range(p))
            t = core + bytes(rng.choice(b"AC") for _ in range(120))
            q = core + bytes(rng.choice(b"GT") for _ in range(120))
            for band in (10, 20):
                zdrop = 2 * o + 3 * max(m, -x)
                for to_qend in (False, True):
                    for f in (et.extend_align, et.extend_align_np):
                        ext, cigar = f(t, q, *params, band, zdrop, to_qend)
                        assert ext.dropped == 1 and p <= ext.rows_done < len(t), (p, params, band, ext)
                        assert (ext.score, ext.t_end, ext.q_end) == (p * m, p, p)
                        cut, cut_cigar = f(t[:ext.rows_done], q, *params, band, -1, to_qend)
                        assert cut._replace(dropped=1) == ext and cut.dropped == 0 and cut_cigar == cigar
                        seen += 1
    assert seen == 7 * 7 * 2 * 2 * 2


def test_the_gap_term_keeps_a_long_deletion_alive():
    """60 target bases that the query skips: the rows inside the deletion have their maximum in the column of the best cell, on
    another diagonal, 909 below it at the far end; the gap term of the predicate allows exactly that, so a zdrop of gopen does not drop
    -- and one without the term would have."""
    rng = random.Random(2)
    m, x, o, e = et.normalize(*GATK)
    a, b = bytes(rng.choice(b"ACGT") for _ in range(80)), bytes(rng.choice(b"ACGT") for _ in range(80))
    t, q = a + b"N" * 60 + b, a + b
    trace = []
    ext, cigar = et.extend_align(t, q, *GATK, 100, o, trace=trace)
    assert ext.dropped == 0 and cigar == "80M60D80M" and (ext.score, ext.t_end, ext.q_end) == (160 * m - o - 59 * e, 220, 160)
    off_diagonal = [(i, rm, rj, best) for i, rm, rj, best in trace if (i - best[1]) - (rj - best[2]) != 0 and best[0] - rm > o]
    assert len(off_diagonal) >= 55  # rows whose fall alone exceeds zdrop: the input does what the docstring says
    assert any(best == (80 * m, 80, 80) and rj == 80 and i == 140 and best[0] - rm == o + 59 * e for i, rm, rj, best in off_diagonal)
    assert et.extend_align_np(t, q, *GATK, 100, o) == (ext, cigar)
    # a drop of the same depth on one diagonal (mismatches only, band 0) does stop
    t2, q2 = a + b"A" * 30, a + b"C" * 30
    ext2, _ = et.extend_align(t2, q2, *GATK, 0, o)
    assert ext2.dropped == 1 and ext2.rows_done == 81 and (ext2.score, ext2.t_end) == (80 * m, 80)


def test_rows_without_a_cell_in_the_band():
    t, q = b"ACGTACGTACGTACGT", b"ACGT"
    for f in (et.extend_align, et.extend_align_np):
        ext, cigar = f(t, q, *GATK, 2, -1)
        assert (ext.score, ext.t_end, ext.q_end, ext.rows_done, ext.dropped, cigar) == (800, 4, 4, 16, 0, "4M")
        ext, cigar = f(t, q, *GATK, 2, 1 << 20)
        assert (ext.rows_done, ext.dropped, ext.score_qend, ext.t_end_qend) == (6, 1, 800, 4)
        ext, _ = f(q, t, *GATK, 2, 1 << 20)  # the query's end out of the band: no last-column cell
        assert (ext.score_qend, ext.t_end_qend, ext.rows_done, ext.dropped) == (et.NO_QEND, -1, 4, 0)
        ext, cigar = f(q, t, *GATK, 2, 1 << 20, True)
        assert ext.cigar_from == 0 and cigar == "4M"


def test_best_cell_on_the_border_is_the_empty_extension():
    for f in (et.extend_align, et.extend_align_np):
        ext, cigar = f(b"AAAA", b"CCCC", *GATK, 4, -1)
        assert (ext.score, ext.t_end, ext.q_end, cigar) == (0, 0, 0, "")
        ext, cigar = f(b"AAAA", b"CCCC", *GATK, 4, -1, True)
        assert ext.cigar_from == 1 and et.cigar_spans(cigar) == (ext.t_end_qend, 4) and et.cigar_score(cigar, b"AAAA", b"CCCC", *GATK) == ext.score_qend


def test_slot_formula_mirror_at_its_edges_and_monotone():
    src = open(os.path.join(ROOT, "mgl_amd", "csrc", "sw_extend.h")).read()
    assert re.search(r"\(\(int64_t\)ql < w \? \(int64_t\)ql : w\) \+ 63 \+ 7\) & ~\(int64_t\)7", src) and "2 * (int64_t)band + 64" in src
    assert et.extend_strip_steps(1, 0) == 64 and et.extend_strip_steps(2, 0) == 72 and et.extend_strip_steps(64, 0) == 128
    assert et.extend_strip_steps(65, 0) == 128 and et.extend_strip_steps(10 ** 6, 0) == 128 and et.extend_strip_steps(10 ** 6, 1) == 136
    assert et.extend_strip_steps(1088, 512) == et.extend_strip_steps(10 ** 4, 512) == 1152 and et.extend_strip_steps(1087, 512) == 1152 and et.extend_strip_steps(1081, 512) == 1144
    assert et.extend_pair_bytes(1, 1, 0) == 256 + 256 + 32 * 64
    assert et.extend_pair_bytes(64, 31, 0) == 256 + 512 + 32 * 96 and et.extend_pair_bytes(65, 32, 0) == 512 + 512 + 2 * 32 * 96
    assert et.extend_pair_bytes(10000, 10000, 512) == 80128 + 80128 + 157 * 1152 * 32 == 5947904   # 5.7 MiB (the banded entry's bound: 27 MiB)
    assert et.extend_pair_bytes(10000, 10000, 512, True) == 80128
    assert et.extend_slot_bytes(100, 50, 10 ** 9) == et.extend_pair_bytes(100, 50, 100)
    # every pair within the maxima fits the slot sized at the maxima, by brute force; and the formula never falls as a length grows
    for band in (0, 1, 31, 32, 33, 200):
        for score_only in (False, True):
            for max_tl in (1, 63, 64, 65, 130):
                for max_ql in (1, 64, 65, 127, 129, 140):
                    slot = et.extend_slot_bytes(max_tl, max_ql, band, score_only)
                    clamped = min(band, max(max_tl, max_ql))
                    prev_row = None
                    for tl in range(1, max_tl + 1):
                        row = [et.extend_pair_bytes(tl, ql, clamped, score_only) for ql in range(1, max_ql + 1)]
                        assert max(row) <= slot and row == sorted(row)
                        assert prev_row is None or all(x >= y for x, y in zip(row, prev_row))
                        prev_row = row
                    assert prev_row[-1] == slot
