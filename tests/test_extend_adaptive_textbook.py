"""The adaptive-band extension textbook (tests/extend_adaptive_textbook.py) without a GPU: the plain and the row-wise forms agree on every
output; the two identities that tie it to tests/extend_textbook.py; the bound on a shift is reached in both directions; a band of 64
follows ten indels of 20 bases where a fixed band of 64 loses the path; the border column, the right end, ties; the slot mirror."""
import os
import random
import re

import extend_adaptive_cases as ac
import extend_adaptive_textbook as at
import extend_textbook as et
import golden_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_CELLS = 6000
GATK = ac.GATK
PARAM_SETS = ac.PARAM_SETS


def _small(suite, every=1):
    return [g for k, g in enumerate(golden_io.load(suite)) if k % every == 0 and len(g.t) * len(g.q) <= MAX_CELLS]


RECORDS = _small("tiny", 7) + _small("ties") + _small("shapes") + _small("random") + _small("known")  # tests/test_extend_textbook.py's


def _rand_pair(rng, tl, ql, alphabet=b"ACGT"):
    """a noisy copy with deleted and inserted runs long enough to move a narrow band"""
    t = bytes(rng.choice(alphabet) for _ in range(tl))
    q, skip = bytearray(), 0
    for ch in t:
        if skip:
            skip -= 1
            continue
        r = rng.random()
        if r < 0.04:
            skip = rng.randint(0, 12)
            continue
        if r < 0.08:
            q += bytes(rng.choice(alphabet) for _ in range(rng.randint(1, 12)))
        q.append(rng.choice(alphabet) if rng.random() < 0.08 else ch)
    q = bytes(q[:ql]) + bytes(rng.choice(alphabet) for _ in range(max(0, ql - len(q))))
    return t, q


def _both(t, q, params, band, zdrop, to_qend=False):
    c1, c2 = [], []
    a = at.extend_adaptive_align(t, q, *params, band, zdrop, to_qend, centres=c1)
    b = at.extend_adaptive_align_np(t, q, *params, band, zdrop, to_qend, centres=c2)
    assert a == b and c1 == c2, (t, q, params, band, zdrop, to_qend, a, b, c1, c2)
    return a, c1


def test_plain_form_equals_the_row_wise_form_on_every_output():
    rng = random.Random(21)
    cases = [(g.t, g.q, g.params) for g in RECORDS]
    for _ in range(500):
        tl, ql = rng.randint(1, 300), rng.randint(1, 300)
        cases.append(_rand_pair(rng, tl, ql, b"AC" if rng.random() < 0.3 else b"ACGT") + (rng.choice(PARAM_SETS),))
    assert len(cases) > 1500
    dropped = moved = qend = 0
    for t, q, params in cases:
        band = rng.choice((0, 1, 2, 5, 17, 40, 64, max(len(t), len(q)), 1000))
        zdrop = rng.choice((-1, 0, params[3], 3 * params[2], 40 * params[0], 1 << 30))
        to_qend = rng.random() < 0.5
        (ext, cigar), centres = _both(t, q, params, band, zdrop, to_qend)
        assert et.cigar_spans(cigar) == ((ext.t_end_qend, len(q)) if ext.cigar_from else (ext.t_end, ext.q_end))
        assert ext.score >= 0 and 0 <= ext.rows_done <= len(t) and ext.dropped == (ext.rows_done < len(t)) and (zdrop >= 0 or not ext.dropped)
        if zdrop < 0 and not to_qend:
            assert et.cigar_score(cigar, t, q, *params) == ext.score
        dropped += ext.dropped
        moved += len(set(centres)) > 1
        qend += ext.cigar_from
    assert dropped > 100 and moved > 100 and qend > 200


def test_within_one_block_and_with_a_band_that_covers_the_pair_the_flag_changes_nothing():
    rng = random.Random(22)
    n = 0
    for g in RECORDS[::3]:
        if len(g.t) <= 64:
            band, zdrop, to_qend = rng.choice((0, 2, 9, 100)), rng.choice((-1, 300, 1 << 30)), rng.random() < 0.5
            assert at.extend_adaptive_align(g.t, g.q, *g.params, band, zdrop, to_qend) == et.extend_align(g.t, g.q, *g.params, band, zdrop, to_qend)
            n += 1
    assert n > 300
    for _ in range(150):
        tl, ql = rng.randint(1, 250), rng.randint(1, 250)
        t, q = _rand_pair(rng, tl, ql)
        params, zdrop, to_qend = rng.choice(PARAM_SETS), rng.choice((-1, 50, 1 << 30)), rng.random() < 0.5
        for band in (tl + ql, tl + ql + 7):
            want = et.extend_align_np(t, q, *params, band, zdrop, to_qend)
            assert at.extend_adaptive_align_np(t, q, *params, band, zdrop, to_qend) == want
            if tl * ql <= 4000:
                assert at.extend_adaptive_align(t, q, *params, band, zdrop, to_qend) == want
        if tl <= 64:
            band = rng.choice((0, 3, 30))
            assert at.extend_adaptive_align(t, q, *params, band, zdrop, to_qend) == et.extend_align(t, q, *params, band, zdrop, to_qend)


def test_a_shift_is_at_most_the_band_and_reaches_it_in_both_directions():
    """(the bound itself is an assertion inside the textbook: every call of this file exercises it)"""
    for band in (1, 8, 33, 40):
        pairs = ac.seam_shift_pairs(band)
        cs = [_both(t, q, GATK, band, -1)[1] for t, q in pairs]
        assert cs[0][:2] == [0, band] and cs[1][:2] == [0, -band]
        assert cs[2][:3] == [0, 0, band] and cs[3][:3] == [0, 0, -band]
        assert cs[4][:3] == [0, band, 0] and cs[5][:3] == [0, -band, 0]
        for (t, q), c in zip(pairs, cs):  # the band found the indel: nothing but it in the CIGAR
            ext, cigar = at.extend_adaptive_align_np(t, q, *GATK, band, -1)
            assert len(re.findall(r"[ID]", cigar)) == (2 if c[1] and not c[2] else 1) and ext.score > 200 * 250, (band, cigar)


def test_a_band_of_64_follows_ten_indels_of_20_bases():
    """the point of the feature: about 3 000 rows, identical except ten 20-base indels; the adaptive band of 64 returns what the fixed
    band that covers the matrix returns, the fixed band of 64 a smaller score"""
    pairs = ac.drift_pairs()
    assert sorted(pairs) == ["deletions", "insertions", "mixed"]
    for name, (t, q) in pairs.items():
        assert 2700 <= len(q) <= 3300 and len(t) == 3000
        centres = []
        got = at.extend_adaptive_align_np(t, q, *GATK, 64, -1, centres=centres)
        full = et.extend_align_np(t, q, *GATK, len(t) + len(q), -1)
        fixed = et.extend_align_np(t, q, *GATK, 64, -1)
        assert got == full, name
        assert fixed[0].score < full[0].score, name
        assert len(re.findall(r"20[ID]", got[1])) == 10 and got[0].t_end == 3000
        assert max(abs(c) for c in centres) >= 100 and {"deletions": min, "insertions": max, "mixed": min}[name](centres) == {"deletions": -200, "insertions": 200, "mixed": -100}[name]


def test_an_unrelated_query_pulls_the_band_to_column_0():
    rng = random.Random(23)
    t = bytes(rng.choice(b"ACGT") for _ in range(300))
    q = bytes(rng.choice(b"NM") for _ in range(300))
    (ext, cigar), centres = _both(t, q, GATK, 8, -1)
    assert centres == [0, -8, -16, -24, -32] and (ext.score, cigar) == (0, "")   # as fast as the bound allows; it never gets there
    (ext, cigar), centres = _both(t, q, GATK, 40, -1, True)
    assert centres[:3] == [0, -40, -80] and 65 + centres[1] - 40 <= 0 < 81 + centres[1] - 40   # (i, 0) is back in the band for rows 65 .. 80
    assert ext.cigar_from == 0 and ext.score_qend == et.NO_QEND
    trace = []
    et.extend_align(t[:70], q, *GATK, 40, -1, trace=trace)  # the static band holds the border column while i <= band, and not after
    assert trace[39][2] == 0 and trace[60][2] > 0


def test_a_band_that_walks_off_the_right_end():
    rng = random.Random(24)
    core = bytes(rng.choice(b"ACGT") for _ in range(70))
    t, q = core + bytes(rng.choice(b"ACGT") for _ in range(200)), b"N" * 60 + core
    for band in (20, 60):
        (off, _), centres = _both(t, q, GATK, band, -1, True)
        (on, _), _ = _both(t, q, GATK, band, 1 << 30, True)
        assert centres[1] >= 15 and off.dropped == 0 and off.rows_done == len(t)
        lo = centres[(on.rows_done) // 64] - band
        assert on.dropped == 1 and on.rows_done + 1 + lo > len(q) >= on.rows_done + lo   # the first row with i + d_b - band > ql drops
        assert (on.score, on.t_end, on.q_end, on.score_qend, on.t_end_qend) == (off.score, off.t_end, off.q_end, off.score_qend, off.t_end_qend)
        assert on.t_end_qend >= 1 and on.cigar_from == 1


def test_homopolymers_and_two_letter_sequences_ties_steer_the_band():
    ts = [b"A" * 300, b"A" * 300, b"AC" * 160, b"ACAC" * 80 + b"A" * 30, b"AC" * 80 + b"CA" * 80, b"AAC" * 100]
    qs = [b"A" * 300, b"A" * 197, b"CA" * 140, b"AC" * 170, b"AC" * 160, b"ACA" * 90]
    for params in (GATK, (1, -1, 1, 1), (3, -1, 4, 3), (1, 0, 1, 0)):
        for band in (0, 3, 9, 64):
            for zdrop in (-1, 2 * params[2]):
                for t, q in zip(ts, qs):
                    _both(t, q, params, band, zdrop, band & 1 == 1)
    # the smallest column among equal maxima: with free extension row 64 of A^200 x A^100 holds 64 in every column from 64 on
    assert _both(b"A" * 200, b"A" * 100, (1, 0, 1, 0), 10, -1)[1][1] == 0


def test_slot_formula_mirror_at_its_edges_and_monotone():
    src = open(os.path.join(ROOT, "mgl_amd", "csrc", "sw_extend.h")).read()
    assert "extend_pair_bytes(tl, ql, band, score_only) + (score_only ? 0 : extend_centre_bytes(tl))" in src
    assert "((int64_t)((tl + 63) / 64) * 4 + 255) / 256 * 256" in src and "EXTEND_RECENTRE_ROWS = 64" in src and at.R == 64
    for tl, extra in ((1, 256), (64, 256), (65, 256), (4096, 256), (4097, 512), (10000, 768)):
        assert at.extend_adaptive_pair_bytes(tl, 50, 9) == et.extend_pair_bytes(tl, 50, 9) + extra
        assert at.extend_adaptive_pair_bytes(tl, 50, 9, True) == et.extend_pair_bytes(tl, 50, 9, True)
    assert at.extend_adaptive_pair_bytes(10200, 10186, 512) == 81664 + 81664 + 160 * 1152 * 32 + 768 == 6062336
    assert at.extend_adaptive_pair_bytes(10200, 10186, 128) == 81664 + 81664 + 160 * 384 * 32 + 768 == 2130176
    assert at.extend_adaptive_slot_bytes(100, 50, 10 ** 9) == at.extend_adaptive_pair_bytes(100, 50, 150)
    for band in (0, 1, 31, 33, 200):
        for score_only in (False, True):
            for max_tl in (1, 63, 64, 65, 130):
                for max_ql in (1, 64, 65, 129, 140):
                    slot = at.extend_adaptive_slot_bytes(max_tl, max_ql, band, score_only)
                    clamped = min(band, max_tl + max_ql)
                    prev_row = None
                    for tl in range(1, max_tl + 1):
                        row = [at.extend_adaptive_pair_bytes(tl, ql, clamped, score_only) for ql in range(1, max_ql + 1)]
                        assert max(row) <= slot and row == sorted(row)
                        assert prev_row is None or all(x >= y for x, y in zip(row, prev_row))
                        prev_row = row
                    assert prev_row[-1] == slot
