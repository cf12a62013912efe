"""The banded textbook (tests/banded_textbook.py) against the committed golden records, without a GPU: a band that covers the matrix
gives the full-matrix result (R1), a band that holds the golden path gives the golden offset and CIGAR (R2), one cell narrower cuts the
path, band 0 on equal lengths is the pure diagonal, the plain and the row-wise forms agree, and the mirrored range guard and slot
formula stand where mgl_amd/csrc/sw_banded.h puts them."""
import os
import random
import re

import pytest

import banded_textbook as bt
import golden_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_CELLS = 12000


def _small(suite, every=1):
    return [g for k, g in enumerate(golden_io.load(suite)) if k % every == 0 and len(g.t) * len(g.q) <= MAX_CELLS]


RECORDS = _small("tiny", 7) + _small("ties") + _small("shapes") + _small("random") + _small("known")


def test_there_are_records_of_every_strategy():
    assert len(RECORDS) > 1000
    assert {g.strategy for g in RECORDS} == {bt.SOFTCLIP, bt.INDEL, bt.LEADING_INDEL, bt.IGNORE}


def test_r1_a_band_that_covers_the_matrix_is_the_full_matrix_function():
    for g in RECORDS:
        band = max(len(g.t), len(g.q))
        off, ez, cigar = bt.banded_align(g.t, g.q, *g.params, g.strategy, band)
        assert (off, ez, cigar) == (g.offset, g.score, g.cigar), (g, off, ez, cigar)


def test_r2_a_band_that_holds_the_path_keeps_offset_and_cigar_and_one_less_cuts_it():
    held = cut = same_text = 0
    for g in RECORDS:
        band = bt.path_band(g)
        if band is None:
            assert g.strategy == bt.IGNORE
            continue
        off, _, cigar = bt.banded_align(g.t, g.q, *g.params, g.strategy, band)
        assert (off, cigar) == (g.offset, g.cigar), (g, band, off, cigar)
        held += 1
        if band > 0:
            # (the path is what is cut: on a homopolymer the narrower band's path can spell the same CIGAR from another offset --
            # one `ties` record, 72 x 43, does -- so the pair is compared)
            off, _, narrower = bt.banded_align(g.t, g.q, *g.params, g.strategy, band - 1)
            assert (off, narrower) != (g.offset, g.cigar), (g, band)
            same_text += narrower == g.cigar
            cut += 1
    assert held > 800 and cut > 250 and same_text <= 1


def test_band_zero_on_equal_lengths_is_the_diagonal():
    rng = random.Random(5)
    for n in (1, 2, 17, 64, 65, 200):
        t = bytes(rng.choice(b"ACGT") for _ in range(n))
        q = bytes(rng.choice(b"ACGT") for _ in range(n))
        for params in ((200, -150, 260, 11), (1, -1, 1, 1), (3, -1, 4, 3)):
            m, x = params[0], -abs(params[1])
            total = sum(m if a == b else x for a, b in zip(t, q))
            for s in (bt.SOFTCLIP, bt.INDEL, bt.LEADING_INDEL, bt.IGNORE):
                for f in (bt.banded_align, bt.banded_align_np):
                    off, ez, cigar = f(t, q, *params, s, 0)
                    assert (off, cigar) == (0, f"{n}M")
                    assert ez == (total, n, total, n, n, 0)


def test_plain_and_row_wise_forms_agree():
    rng = random.Random(11)
    psets = [(200, -150, 260, 11), (25, -50, 110, 6), (3, -1, 4, 3), (1, -1, 1, 1), (1, -4, 6, 1), (5, -4, 2, 7), (2, -3, 0, 0)]
    for k in range(400):
        tl, ql = rng.randint(1, 90), rng.randint(1, 90)
        alpha = b"AC" if k % 5 == 0 else b"ACGT"
        t = bytes(rng.choice(alpha) for _ in range(tl))
        q = bytes(rng.choice(alpha) for _ in range(ql)) if k % 3 else (t[: ql // 2] + t[ql // 2 + 3:])[:ql] or b"A"
        band = rng.choice((0, 1, 2, 5, 17, 100))
        s = (bt.SOFTCLIP, bt.INDEL, bt.LEADING_INDEL, bt.IGNORE)[k % 4]
        p = psets[k % len(psets)]
        assert bt.banded_align(t, q, *p, s, band) == bt.banded_align_np(t, q, *p, s, band), (t, q, p, s, band)


def test_path_band_of_hand_made_records():
    G = golden_io.Golden
    g = G("x", b"A" * 10, b"A" * 10, (1, -1, 1, 1), bt.SOFTCLIP, 0, "10M", (0,) * 6, 0)
    assert bt.path_band(g) == 0
    g = g._replace(cigar="3M2I5M", q=b"A" * 10, t=b"A" * 8)  # ql - tl = 2: the band's own slant holds the run
    assert bt.path_band(g) == 0
    g = g._replace(cigar="3M2D3M2I2M", t=b"A" * 10, q=b"A" * 10)  # two rows below the diagonal
    assert bt.path_band(g) == 2
    g = g._replace(cigar="2S8M", offset=0, t=b"A" * 10, q=b"A" * 10)  # starts at (0, 2)
    assert bt.path_band(g) == 2
    assert bt.path_band(g._replace(strategy=bt.IGNORE)) is None


def test_range_guard_mirror_at_its_edges():
    ok = bt.banded_range_ok
    assert ok(1, 1, 200, -150, 260, 11) and ok(10000, 10000, 200, -150, 260, 11)
    assert not ok(0, 5, 1, -1, 1, 1) and not ok(5, 0, 1, -1, 1, 1)
    assert ok(1 << 28, 1, 0, 0, 0, 0) and not ok((1 << 28) + 1, 1, 0, 0, 0, 0)
    assert ok(5, 5, 1, -1, 1 << 24, 1 << 24) and not ok(5, 5, 1, -1, (1 << 24) + 1, 1) and not ok(5, 5, 1, -1, 1, (1 << 24) + 1)
    assert not ok(5, 5, -1, -1, 1, 1) and not ok(5, 5, 1, 1, 1, 1)  # not normalised
    # max(match, |mismatch|) min + 2 gopen + gext max <= 2^29, to the unit
    n = 1 << 20
    assert ok(n, n, 511, -3, 100, 1) == (511 * n + 200 + n <= 1 << 29)
    assert ok(n, n, 500, -3, 0, 12) and not ok(n, n, 500, -3, 1, 12)  # 500 n + 12 n = 2^29 exactly
    assert ok(n, 2 * n, 3, -488, 0, 12) and not ok(n, 2 * n, 3, -488, 1, 12)  # 488 n + 24 n
    src = open(os.path.join(ROOT, "mgl_amd", "csrc", "sw_banded.h")).read()
    assert re.search(r"BANDED_MAX_LEN = 1 << 28;", src) and re.search(r"BANDED_MAX_SCORE = 1 << 29;", src)
    assert "s * lo + 2 * (int64_t)gopen + (int64_t)gext * hi <= BANDED_MAX_SCORE" in src


def test_slot_formula_mirror():
    # 10 kb x 10 kb at band 512: 157 strips x (1 025 + 63 columns + 63 steps of skew) x 32 bytes, the carry row and the elements
    assert bt.banded_strip_steps(10000, 10000, 512) == 1152
    assert bt.banded_pair_bytes(10000, 10000, 512) == 80128 + 80128 + 157 * 1152 * 32
    assert bt.banded_pair_bytes(10000, 10000, 512, score_only=True) == 80128
    assert bt.banded_strip_steps(100, 30, 1000) == (30 + 63 + 7) & ~7  # never more than the query
    src = open(os.path.join(ROOT, "mgl_amd", "csrc", "sw_banded.h")).read()
    assert "banded_strip_steps(tl, ql, band) * 32" in src and "(tl + ql + 4) * 4" in src and "(ql + 1) * 8" in src


def test_slot_bound_mirror_covers_every_pair_within_the_bounds():
    """banded_slot_bound() is a case analysis: brute force over every (tl, ql) within small bounds says it is an upper bound of
    banded_pair_bytes, and a tight one (some pair needs all of its decisions part)."""
    for max_tl, max_ql in ((1, 1), (5, 200), (64, 64), (65, 300), (130, 129), (200, 50), (260, 260), (300, 70)):
        for band in (0, 1, 7, 33, 64, 100, 400):
            bound = bt.banded_slot_bound(max_tl, max_ql, band)
            need = max(bt.banded_pair_bytes(tl, ql, band) for tl in range(1, max_tl + 1) for ql in range(1, max_ql + 1))
            assert need <= bound, (max_tl, max_ql, band, need, bound)
            fixed = bt.banded_pair_bytes(max_tl, max_ql, band, score_only=True) + (max_tl + max_ql + 4) * 4 + 255
            assert bound - need <= fixed, (max_tl, max_ql, band, need, bound)  # (the carry row and the elements are sized by the maxima)
            assert bt.banded_slot_bound(max_tl, max_ql, band, score_only=True) == bt.banded_pair_bytes(1, max_ql, band, score_only=True)
    # the long-read case: slots are sized for the worst pair the bounds admit, not for the square one
    assert bt.banded_pair_bytes(10000, 10000, 512) < 6 << 20 < 26 << 20 < bt.banded_slot_bound(10000, 10000, 512) < 28 << 20
    src = open(os.path.join(ROOT, "mgl_amd", "csrc", "sw_banded.h")).read()
    assert "const int64_t peak = ((int64_t)t_max + 2 * (int64_t)band + 64 + 1) / 2;" in src
    assert "const int qs[4] = {max_ql, (int)(peak < max_ql ? peak : max_ql), (int)(peak + 1 < max_ql ? peak + 1 : max_ql), t_max < max_ql ? t_max : max_ql};" in src
