"""sw_dp16_lane_ck_kernel, the narrow CARRY rows: where 0 <= o - e <= 255 the *_fold kernels keep every kept row -- the row
entering each 32-row strip (row 32 k, the border row 0 included) as well as the row in a strip's middle -- as H of four columns and
a difference byte H - E per column, one format, column 0 not stored (WaveMem, sw_dp16_lane_ck.hip).  Pass 1 itself rebuilds E of
the row that enters a strip from the byte, so a wrong byte changes SCORES, not only CIGARs.  MGL_SW_DEBUG_CK_WIDE=1 keeps the wide
records (the *_fold_wide kernels).  Every launch here is a few hundred pairs on this kernel; every output is compared byte for byte
with the oracle, in both forms, and the two forms with each other.

The cells that decide: a carry row's byte is 0 where a vertical gap RUNS THROUGH row 32 k and o - e where it OPENS right below it,
so deletions are placed with their first missing target row at 32 k and at 32 k + 1, in runs of 3 and of 40 rows (across one seam
and across two), at tl = 65 and 97 (a partial last strip) -- and asserted to be there, from the oracle's own CIGARs.  Query lengths
run through every shape of the last group of four columns on both sides of the tail rule (3 ceil(ql / 4) <= ql: only ql = 1, 2
and 5 keep a wide tail) and zero, one and several checkpoints; o - e through 0, 249, 255 and 256 (the wide form without the switch).

Two mutants of the kernel, each built once and this file run once on it (not kept), fail it:
  * pass 1's reader sign-extends the carry byte (differences of 128 .. 255 come back negative);
  * a column's carry byte is taken from its neighbour in the group.
The first fails 20 of the 26 cases: test_vertical_gaps_across_a_seam for o - e = 249 and 255, test_query_lengths for every ql >= 3,
test_query_lengths_grouped, test_band_parities, test_column_0_of_a_carry_row and test_two_bit_scatter_and_a_second_launch; the
second the same but test_band_parities.  Both pass o - e = 0 (every byte 0), o - e = 256 and the set without a folded diagonal (the
wide kernels) and ql = 1 and 2 (a wide tail: no byte), as they must.  (docs/history.md C.000e has the runs.)"""
import re

import numpy as np
import pytest

import oracle_lib as ol
from mgl_amd import smithwaterman as sw

pytestmark = pytest.mark.gpu

LANE16_CK = 7
CK = 32  # LANE_CK_COLS
ACGT = np.frombuffer(b"ACGT", np.uint8)
GATK = (200, -150, 260, 11)  # o - e = 249, folds
# o - e = 0, 249, 255 (narrow), 256 (folds, but takes the wide kernels), and a set without a folded diagonal (wide)
PARAMS = ((200, -150, 11, 11), GATK, (200, -150, 266, 11), (200, -150, 267, 11), (25, -50, 110, 6))


def _diag_fold(match, mismatch, gext):
    """sw_device.h diag_fold(): does some K take two bytes to match + 2e and mismatch + 2e (mod 2^16)?"""
    a, x = (match + 2 * gext) & 0xFFFF, (mismatch + 2 * gext) & 0xFFFF
    if not (a or x):
        return True
    for k in range(1, 1 << 16):
        s = (k & -k).bit_length() - 1
        ok = True
        for v in (a, x):
            if v & ((1 << s) - 1):
                ok = False
                break
            b = ((v >> s) * pow(k >> s, -1, 1 << 16)) & ((0x10000 >> s) - 1)
            if b > 255:
                ok = False
                break
        if ok:
            return True
    return False


def _rand(rng, n):
    return ACGT[rng.integers(0, 4, n)]


def _gapped(rng, tl, ql, kind, at, g, cut):
    """One pair: the read is target[s:] with ONE gap at read position `cut` -- kind 'D': target rows at .. at + g - 1 (1-based) are
    missing from the read; 'I': g foreign bases, the first in column `at` -- or None where that does not fit the geometry with eight
    bases of the target on either side of the gap."""
    t = _rand(rng, tl)
    if kind == "D":
        s = at - 1 - cut
        if s < 0 or cut < 8 or ql - cut < 8 or s + ql + g > tl:
            return None
        q = np.concatenate([t[s:s + cut], t[s + cut + g:s + ql + g]])
    else:
        cut = at - 1
        s = int(rng.integers(0, max(1, tl - ql)))
        if cut < 8 or ql - cut - g < 8 or s + ql - g > tl:
            return None
        q = np.concatenate([t[s:s + cut], _rand(rng, g), t[s + cut:s + ql - g]])
    assert len(q) == ql
    return t.tobytes(), q.tobytes()


def _plain(rng, tl, ql, k):
    """a read cut from its target, every fourth one with a substitution"""
    t = _rand(rng, tl)
    s = int(rng.integers(0, tl - ql + 1)) if tl >= ql else 0
    q = np.concatenate([t[s:s + ql], _rand(rng, ql)])[:ql].copy()
    if k % 4 == 1 and ql > 2:
        j = int(rng.integers(0, ql))
        q[j] = ACGT[(int(np.searchsorted(ACGT, q[j])) + 1) % 4]
    return t.tobytes(), q.tobytes()


def _seam_pairs(tl, ql, n, seed, rows, glens=(3,), every=1, cols=()):
    """n pairs of tl x ql: in every `every`-th pair a deletion whose first missing row runs through `rows` (or an insertion whose first
    column runs through `cols`), its length through `glens`, at read positions that run through the read; the rest plain"""
    rng = np.random.default_rng(seed)
    places = [("D", r, g) for g in glens for r in rows] + [("I", c, 3) for c in cols]
    ts, qs = [], []
    for k in range(n):
        pair = None
        if places and k % every == 0:
            kind, at, g = places[(k // every) % len(places)]
            for attempt in range(max(1, ql - 15)):  # read positions from one that runs through the read, until the gap fits
                pair = _gapped(rng, tl, ql, kind, at, g, 8 + (13 * (k // every) + attempt) % max(1, ql - 15))
                if pair:
                    break
        t, q = pair or _plain(rng, tl, ql, k)
        ts.append(t)
        qs.append(q)
    return ts, qs


def _runs(offsets, cigars):
    """the gap runs of SOFTCLIP results, per pair: ('D', first row, column it stands in, length) / ('I', row, first column, length), 1-based"""
    out = []
    for off, cg in zip(offsets, cigars):
        i, j, mine = int(off), 0, []
        for n, op in re.findall(r"(\d+)([MIDS])", cg if isinstance(cg, str) else cg.decode()):
            n = int(n)
            if op == "M":
                i, j = i + n, j + n
            elif op == "S":
                j += n
            elif op == "D":
                mine.append(("D", i + 1, j, n))
                i += n
            else:
                mine.append(("I", i, j + 1, n))
                j += n
        out.append(mine)
    return out


@pytest.fixture()
def lane():
    a = sw.MicrosoftSmithWaterman(0)
    a.set_lane_kernel(2)
    yield a
    a.close()


_want = {}


def _oracle(key, ts, qs, params, strategy):
    """(one oracle run per batch, parameters and strategy, shared by the cases that align the same batch)"""
    k = (key, params, strategy)
    if k not in _want:
        _want[k] = ol.oracle_align_batch(ts, qs, params, strategy, nthreads=8)
    return _want[k]


def _same(res, want, what):
    off, sc, cg = want
    assert (np.asarray(res.offsets) == off).all(), what
    assert (np.asarray(res.scores) == sc).all(), what
    assert list(res.cigars) == list(cg), what


def _both_forms(a, monkeypatch, key, ts, qs, params, strategy, run=None, **kw):
    """the launch's own form (narrow where the parameters allow it) and, with the switch, the wide one: each against the oracle,
    and against each other"""
    want = _oracle(key, ts, qs, params, strategy)
    got = []
    for wide in ("0", "1"):
        monkeypatch.setenv("MGL_SW_DEBUG_CK_WIDE", wide)
        res = run(a) if run else a.align_batch(ts, qs, params, strategy, **kw)
        assert a.timing().fill_kernel == LANE16_CK, (key, params, strategy)
        _same(res, want, (key, params, strategy, "wide" if wide == "1" else "default"))
        got.append(res)
    monkeypatch.delenv("MGL_SW_DEBUG_CK_WIDE")
    assert (np.asarray(got[0].offsets) == np.asarray(got[1].offsets)).all() and (np.asarray(got[0].scores) == np.asarray(got[1].scores)).all()
    assert list(got[0].cigars) == list(got[1].cigars)


def test_parameter_sets():
    """the sets above are what the cases need: differences 0, 249, 255 and 256, folding and not"""
    assert [p[2] - p[3] for p in PARAMS] == [0, 249, 255, 256, 104]
    assert [_diag_fold(p[0], p[1], p[3]) for p in PARAMS] == [True, True, True, True, False]


# ---- vertical gaps across a strip seam.  tl = 65 (strips of 32, 32 and ONE row) and 97 (32, 32, 32 and one) reach this kernel only
# inside a grouped launch: whole waves of each geometry, 32-row strips whatever the target
SEAM_GEOMETRIES = ((65, 24, 257), (65, 40, 258), (97, 50, 385), (97, 32, 257))


def _seam_batch():
    ts, qs = [], []
    for tl, ql, n in SEAM_GEOMETRIES:
        # (tl = 65 has no room for 40 missing rows FROM row 32: there the long runs start at rows 9 .. 12 and cross the seam at 32)
        t1, q1 = _seam_pairs(tl, ql, n, 1000 * tl + ql, rows=(31, 32, 33, 34, 63, 64, 65, 66) + ((9, 10, 11, 12) if tl == 65 else ()), glens=(3, 40))
        ts += t1
        qs += q1
    order = np.random.default_rng(65).permutation(len(ts))
    return [ts[k] for k in order], [qs[k] for k in order]


@pytest.mark.parametrize("params", PARAMS)
def test_vertical_gaps_across_a_seam(monkeypatch, params):
    """Deletions whose first missing row is 32 k (the gap runs through the carry row: byte 0) and 32 k + 1 (it opens right below it:
    byte o - e), runs of 3 rows and of 40 (across one seam at tl = 65, across two at tl = 97).  The oracle's CIGARs say where the
    gaps really are."""
    monkeypatch.setenv("MGL_SW_DEBUG_LANE_GROUP_MIN", "128")
    ts, qs = _seam_batch()
    assert len(ts) >= 1024  # (the library sorts batches of 1 024 pairs and more)
    off, _, cg = _oracle("seam", ts, qs, GATK, ol.SOFTCLIP)
    dels = [(len(t), r, n) for t, runs in zip(ts, _runs(off, cg)) for k, r, _, n in runs if k == "D"]
    seen = {(tl, r % 32, n) for tl, r, n in dels}
    assert {(65, 0, 3), (65, 1, 3), (97, 0, 3), (97, 1, 3), (97, 0, 40), (97, 1, 40)} <= seen, sorted(seen)
    assert any(tl == 65 and n == 40 and r <= 32 < r + n for tl, r, n in dels), "a run of 40 rows across the seam at 32, tl = 65"
    assert any(tl == 97 and n == 40 and r <= 32 and r + n > 64 for tl, r, n in dels), "a run of 40 rows across the seams at 32 and 64"
    a = sw.MicrosoftSmithWaterman(0)
    a.set_small_kernel(1)
    try:
        for strategy in ol.STRATEGIES if params == GATK else (ol.SOFTCLIP, ol.INDEL):
            _both_forms(a, monkeypatch, "seam", ts, qs, params, strategy, cigar_stride=256)
    finally:
        a.close()


# every shape of the last group of four columns (one to four columns) on both sides of the tail rule (ql = 1, 2, 5: a wide tail), with
# zero, one (64: the checkpoint is the last column's), two (65) and four (150) checkpoints
QLS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 32, 33, 34, 35, 64, 65, 150)


@pytest.mark.parametrize("ql", QLS)
def test_query_lengths(lane, monkeypatch, ql):
    """tl = 64 (two strips: the carry row 32 is written by one strip and read by the next; 128 and 256 for the queries that leave no
    room for a deletion in 64 rows), 131 pairs, where the query is long enough with deletions on either side of a seam.  With the
    lane kernel forced the planner sends every ql >= 1 here."""
    tl = 64 if ql <= 35 else 128 if ql <= 65 else 256
    ts, qs = _seam_pairs(tl, ql, 131, 6400 + ql, rows=tuple(r for r in (31, 32, 33, 34, 63, 64, 65, 66, 95, 96, 97) if r < tl - 16), every=2)
    for strategy in (ol.SOFTCLIP, ol.INDEL):
        _both_forms(lane, monkeypatch, ("ql", ql), ts, qs, GATK, strategy)
    _both_forms(lane, monkeypatch, ("ql", ql), ts, qs, PARAMS[2], ol.LEAD_INDEL)


def test_query_lengths_grouped(monkeypatch):
    """The same shapes of the last group as waves of ONE launch (the tail's form is a property of the wave, not of the launch), with a
    partial last strip: tl = 97 with ql = 5 (a wide tail), 6, 7 and 9."""
    monkeypatch.setenv("MGL_SW_DEBUG_LANE_GROUP_MIN", "128")
    ts, qs = [], []
    for tl, ql, n in ((97, 5, 257), (97, 6, 258), (97, 7, 257), (97, 9, 259), (80, 2, 130)):
        t1, q1 = _seam_pairs(tl, ql, n, 100 * tl + ql, rows=())
        ts += t1
        qs += q1
    order = np.random.default_rng(97).permutation(len(ts))
    ts, qs = [ts[k] for k in order], [qs[k] for k in order]
    assert len(ts) >= 1024
    a = sw.MicrosoftSmithWaterman(0)
    a.set_small_kernel(1)
    try:
        for strategy in (ol.SOFTCLIP, ol.INDEL):
            _both_forms(a, monkeypatch, "ql grouped", ts, qs, GATK, strategy, cigar_stride=256)
    finally:
        a.close()


def test_band_parities(lane, monkeypatch):
    """160 x 100, 259 pairs (odd).  The two walks of a lane wait for blocks of different 16-row bands and different column blocks in
    the same round: pair A has its gap in the UPPER band of a strip (the band's kept row is a carry row) near column 20, pair B in
    the LOWER band of another strip (a middle row) near column 80 -- and in the second half of the batch the other way round."""
    tl, ql = 160, 100
    rng = np.random.default_rng(160100)
    upper, lower = ("D", 40, 3, 20), ("D", 120, 3, 80)  # (kind, first missing row, length, read position)
    ts, qs = [], []
    for k in range(259):
        kind, at, g, cut = (upper, lower)[(k + (k >= 130)) % 2]
        t, q = _gapped(rng, tl, ql, kind, at, g, cut)
        ts.append(t)
        qs.append(q)
    off, _, cg = _oracle("parity", ts, qs, GATK, ol.SOFTCLIP)
    runs = _runs(off, cg)
    band = [{((r - 1) >> 4) & 1 for k, r, _, n in mine if k == "D"} for mine in runs]
    block = [{c // CK for k, _, c, n in mine if k == "D"} for mine in runs]
    assert any(band[k] == {0} and band[k + 1] == {1} and block[k] != block[k + 1] for k in range(0, 128, 2)), "A upper, B lower"
    assert any(band[k] == {1} and band[k + 1] == {0} and block[k] != block[k + 1] for k in range(130, 258, 2)), "A lower, B upper"
    for strategy in ol.STRATEGIES:
        _both_forms(lane, monkeypatch, "parity", ts, qs, GATK, strategy)
    _both_forms(lane, monkeypatch, "parity", ts, qs, PARAMS[2], ol.SOFTCLIP)


def test_column_0_of_a_carry_row(lane, monkeypatch):
    """128 x 90.  Reads that start at target base 32 k: the walk's diagonal passes through the cells (32 k + 32 b, 32 b) -- a carry
    row at a block's left edge -- and ends in (32 k, 0), column 0 of a carry row, which no kept row stores: the border's formula
    stands in for it in pass 1 (the diagonal entering a strip's first column), in the stretch check and in a recomputed block's first
    column.  Small gaps right behind those cells have the blocks there recomputed.  INDEL and LEAD_INDEL give the border a slope."""
    tl, ql = 128, 90
    rng = np.random.default_rng(12890)
    ts, qs = [], []
    for s in (32, 0, 32, 64, 32):
        for p in (2, 3, 5, 34, 35, 66, 67):
            for g in (1, -1, 2, -2):
                t = _rand(rng, tl)
                src = t[s:]
                r = np.concatenate([src[:p], _rand(rng, g), src[p:]]) if g > 0 else np.concatenate([src[:p], src[p - g:]])
                ts.append(t.tobytes())
                qs.append(np.concatenate([r, _rand(rng, ql)])[:ql].tobytes())
    ts, qs = ts[:-1], qs[:-1]
    assert len(ts) % 2 == 1 and len(ts) > 128
    off, _, cg = _oracle("col0", ts, qs, GATK, ol.SOFTCLIP)
    first = [re.match(r"(\d+)([MIDS])", c if isinstance(c, str) else c.decode()) for c in cg]
    assert sum(int(o) == 32 and m.group(2) == "M" for o, m in zip(off, first)) >= 20, "walks that end in (32, 0)"
    assert sum(int(o) == 0 and m.group(2) == "M" and int(m.group(1)) >= 32 for o, m in zip(off, first)) >= 5, "walks through (32, 32)"
    for params in (GATK, PARAMS[2], PARAMS[0]):
        for strategy in ol.STRATEGIES if params == GATK else (ol.INDEL,):
            _both_forms(lane, monkeypatch, "col0", ts, qs, params, strategy)


def test_two_bit_scatter_and_a_second_launch(lane, monkeypatch):
    """128 x 120 with gaps around every seam and checkpoint: as 2-bit input (the walks read the staged codes), with a CIGAR stride that
    is no multiple of four (the scatter kernels) -- and launch after launch on ONE context, with another gap cost and another strategy
    in between: the border row is written once per launch, in the kept rows' format, and must be this launch's."""
    from mgl_amd import device_batch as db

    tl, ql = 128, 120
    ts, qs = _seam_pairs(tl, ql, 257, 2281, rows=(31, 32, 33, 34, 63, 64, 65, 66, 95, 96, 97), cols=(32, 33, 64, 65))
    tb, qb = db.pack2bit(b"".join(ts)), db.pack2bit(b"".join(qs))
    t_start, q_start = np.arange(len(ts), dtype=np.int64) * tl, np.arange(len(qs), dtype=np.int64) * ql
    for params in (GATK, PARAMS[0], PARAMS[4]):
        _both_forms(lane, monkeypatch, "forms", ts, qs, params, ol.INDEL,
                    run=lambda a: a.align_packed_2bit(tb, tl * len(ts), t_start, None, qb, ql * len(qs), q_start, None, tl, ql, params, ol.INDEL))
        _both_forms(lane, monkeypatch, "forms", ts, qs, params, ol.SOFTCLIP, cigar_stride=250)
    for params, strategy in ((GATK, ol.SOFTCLIP), (PARAMS[2], ol.INDEL), (GATK, ol.SOFTCLIP), (PARAMS[0], ol.LEAD_INDEL), (GATK, ol.INDEL)):
        res = lane.align_batch(ts, qs, params, strategy)
        assert lane.timing().fill_kernel == LANE16_CK
        _same(res, _oracle("forms", ts, qs, params, strategy), ("second launch", params, strategy))
