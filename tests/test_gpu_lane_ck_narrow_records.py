"""sw_dp16_lane_ck_kernel, pass 1's NARROW records: where 0 <= o - e <= 255 the *_fold kernels keep the middle rows and the column
checkpoints as H and a difference byte (H - E, H - the horizontal-gap value), 16 bytes a store, instead of two 16-bit values each
(WaveMem, sw_dp16_lane_ck.hip).  MGL_SW_DEBUG_CK_WIDE=1 keeps the wide records (the *_fold_wide kernels).  Every launch here is a few hundred pairs forced
onto this kernel; every output is compared byte for byte with the oracle, in both forms, and the two forms with each other.

The cells that decide: a record's byte is 0 where the gap RUNS THROUGH the kept cell and o - e where it OPENS right behind it, so
the gaps are placed on both sides of a middle row (row 32 k + 16) and of a checkpoint (column 32 b) -- and asserted to be there,
from the oracle's own CIGARs.  Query lengths run through every shape of the last group of four columns and zero, one and several
checkpoints; o - e through 0, 249, 255 and 256 (the wide form without the switch).

Two mutants of the kernel, each built once and this file run once on it (not kept), fail it -- both the same 15 cases:
  * the readers sign-extend the byte (differences of 128 .. 255 come back negative);
  * a column's difference bytes are taken from its neighbour in the pair.
test_gaps_around_the_kept_cells for o - e = 249 and 255, test_query_lengths for every ql >= 3, test_lane_halves_and_odd_count,
test_two_bit_and_scatter and test_grouped_partial_strip fail; the cases that run the wide records (o - e = 256, no folded diagonal,
ql = 1 and 2: a last group of one or two columns is wide) and o - e = 0 (every byte 0) pass, as they must.
(docs/history.md C.000d has the runs.)"""
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


def _pairs(tl, ql, n, seed, rows=(), cols=(), glen=3, every=1):
    """n pairs: a read cut from its target with a substitution or two and, in every `every`-th pair, ONE gap.  `rows`: deletions
    whose first missing target row (1-based) runs through these values (where the read reaches them); `cols`: insertions whose
    first foreign column (1-based) runs through these.  Without either: gaps at places that run through the whole read."""
    rng = np.random.default_rng(seed)
    ts, qs = [], []
    places = [("D", r) for r in rows] + [("I", c) for c in cols]
    for k in range(n):
        t = ACGT[rng.integers(0, 4, tl)].copy()
        s = int(rng.integers(0, max(1, tl - ql - glen + 1))) if tl >= ql + glen else 0
        src = np.concatenate([t[s:], ACGT[rng.integers(0, 4, ql + 2 * glen + 8)]])
        if k % every == 0 and ql > 8:
            g = glen + (k // max(1, len(places))) % 2 if places else 1 + k % 5
            kind, at = places[k % len(places)] if places else (("D", "I")[k % 2], 0)
            if not places:
                cut = 3 + (k * 7) % (ql - 6)
            elif kind == "D":  # target rows s + cut + 1 .. s + cut + g are missing from the read
                s = max(0, min(s, at - 4))
                src = np.concatenate([t[s:], ACGT[rng.integers(0, 4, ql + 2 * glen + 8)]])
                cut = at - 1 - s
            else:
                cut = at - 1
            if 3 <= cut <= ql - 3:
                if kind == "D":
                    src = np.concatenate([src[:cut], src[cut + g:]])
                else:
                    src = np.concatenate([src[:cut], ACGT[rng.integers(0, 4, g)], src[cut:]])
        q = src[:ql].copy()
        if k % 4 == 1 and ql > 2:
            j = int(rng.integers(0, ql))
            q[j] = ACGT[(int(np.searchsorted(ACGT, q[j])) + 1) % 4]
        ts.append(t.tobytes())
        qs.append(q.tobytes())
    return ts, qs


def _runs(offsets, cigars):
    """the gap runs of SOFTCLIP results: ('D', first row, column it stands in, length) / ('I', row, first column, length), 1-based"""
    out = []
    for off, cg in zip(offsets, cigars):
        i, j = int(off), 0
        for n, op in re.findall(r"(\d+)([MIDS])", cg if isinstance(cg, str) else cg.decode()):
            n = int(n)
            if op == "M":
                i, j = i + n, j + n
            elif op == "S":
                j += n
            elif op == "D":
                out.append(("D", i + 1, j, n))
                i += n
            else:
                out.append(("I", i, j + 1, n))
                j += n
    return out


@pytest.fixture()
def lane():
    a = sw.MicrosoftSmithWaterman(0)
    a.set_lane_kernel(2)
    yield a
    a.close()


_want = {}


def _oracle(key, ts, qs, params, strategy):
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


# o - e = 0, 249, 255 (narrow where the diagonal folds), 256 (wide, no switch needed); the last two sets have no folded diagonal
PARAMS = ((200, -150, 11, 11), GATK, (200, -150, 266, 11), (200, -150, 267, 11), (25, -50, 6, 6), (25, -50, 110, 6))


def test_parameter_sets():
    """the sets above are what the cases need: differences 0, 249, 255 and 256, folding and not"""
    assert [p[2] - p[3] for p in PARAMS] == [0, 249, 255, 256, 0, 104]
    assert [_diag_fold(p[0], p[1], p[3]) for p in PARAMS] == [True, True, True, True, False, False]


@pytest.mark.parametrize("params", PARAMS)
def test_gaps_around_the_kept_cells(lane, monkeypatch, params):
    """128 x 120, 257 pairs (odd).  Deletions whose first missing row is row 16 and row 17 of a strip (32 k + 16: the gap runs through
    the middle row, its byte is 0; 32 k + 17: it opens right below it, the byte is o - e) and rows next to them; insertions whose first
    column is 32 b (the gap runs through the checkpoint) and 32 b + 1 (it opens behind it).  The oracle's CIGARs say where the
    gaps really are."""
    tl, ql = 128, 120
    ts, qs = _pairs(tl, ql, 257, 1281, rows=(15, 16, 17, 18, 47, 48, 49, 80, 81), cols=(31, 32, 33, 34, 64, 65, 96, 97))
    off, _, cg = _oracle("kept", ts, qs, GATK, ol.SOFTCLIP)
    runs = _runs(off, cg)
    d_rows = {r % 32 for k, r, _, n in runs if k == "D" and n >= 2}
    i_cols = {(c % CK, c // CK) for k, _, c, n in runs if k == "I" and n >= 2 and c >= CK}
    assert {16, 17} <= d_rows, sorted(d_rows)
    assert {0, 1} <= {c for c, _ in i_cols} and {b for c, b in i_cols if c in (0, 1)} >= {1, 2, 3}, sorted(i_cols)
    for strategy in ol.STRATEGIES if params == GATK else (ol.SOFTCLIP, ol.INDEL):
        _both_forms(lane, monkeypatch, "kept", ts, qs, params, strategy)


# every shape of a strip's last group of columns (32: none; 33, 34: wide records; 35: a group of three) with zero, one (64: the
# checkpoint is the last column's), two (65) and four (150) checkpoints -- and the shortest queries there are: one group or less
QLS = (1, 2, 3, 5, 6, 32, 33, 34, 35, 64, 65, 150)


@pytest.mark.parametrize("ql", QLS)
def test_query_lengths(lane, monkeypatch, ql):
    """tl = 64 (two strips: every middle row and checkpoint has a strip behind it), 131 pairs.  With the lane kernel forced the
    planner sends every ql >= 1 here, so the shortest ones are cases too."""
    tl = 64
    ts, qs = _pairs(tl, ql, 131, 6400 + ql)
    for strategy in (ol.SOFTCLIP, ol.INDEL):
        _both_forms(lane, monkeypatch, ("ql", ql), ts, qs, GATK, strategy)
    _both_forms(lane, monkeypatch, ("ql", ql), ts, qs, PARAMS[2], ol.LEAD_INDEL)


def test_lane_halves_and_odd_count(lane, monkeypatch):
    """125 x 70 (a partial last strip), 259 pairs: a lane's pair A has a gap and its pair B has none, then the other way round
    -- the two halves of a record's dwords must not leak into each other.  All four strategies."""
    tl, ql = 125, 70
    ta, qa = _pairs(tl, ql, 130, 12570, rows=(16, 17, 48, 49), cols=(32, 33, 64, 65), every=2)
    tb, qb = _pairs(tl, ql, 129, 12571, rows=(16, 17, 48, 49), cols=(32, 33, 64, 65), every=2)
    ts, qs = ta + tb[1:] + tb[:1], qa + qb[1:] + qb[:1]  # (second part: the gaps in the odd pairs)
    assert len(ts) % 2 == 1
    off, _, cg = _oracle("halves", ts, qs, GATK, ol.SOFTCLIP)
    gapped = [bool(re.search(r"\d+[DI]", c if isinstance(c, str) else c.decode())) for c in cg]
    assert any(gapped[k] and not gapped[k + 1] for k in range(0, 128, 2)) and any(gapped[k + 1] and not gapped[k] for k in range(130, 258, 2))
    for strategy in ol.STRATEGIES:
        _both_forms(lane, monkeypatch, "halves", ts, qs, GATK, strategy)


def test_two_bit_and_scatter(lane, monkeypatch):
    """The same kind of pairs as 2-bit input (the walks read the staged codes) and with a CIGAR stride that is no multiple of four
    (the scatter kernels), with parameters that fold and parameters that do not."""
    from mgl_amd import device_batch as db

    tl, ql = 128, 120
    ts, qs = _pairs(tl, ql, 257, 2281, rows=(16, 17, 48, 49, 80, 81), cols=(32, 33, 64, 65, 96, 97))
    tb, qb = db.pack2bit(b"".join(ts)), db.pack2bit(b"".join(qs))
    t_start, q_start = np.arange(len(ts), dtype=np.int64) * tl, np.arange(len(qs), dtype=np.int64) * ql
    for params in (GATK, PARAMS[0], PARAMS[5]):
        _both_forms(lane, monkeypatch, "2bit", ts, qs, params, ol.INDEL,
                    run=lambda a: a.align_packed_2bit(tb, tl * len(ts), t_start, None, qb, ql * len(qs), q_start, None, tl, ql, params, ol.INDEL))
        _both_forms(lane, monkeypatch, "2bit", ts, qs, params, ol.SOFTCLIP, cigar_stride=250)


def test_grouped_partial_strip(monkeypatch):
    """A grouped launch -- whole waves of each geometry, 32-row strips whatever the target: targets of 80 and 97 rows (a partial last
    strip of 16 rows and of one row) with queries of 33, 35, 70 and 5 columns, so every wave has its own shape of groups and tails."""
    monkeypatch.setenv("MGL_SW_DEBUG_LANE_GROUP_MIN", "128")
    ts, qs = [], []
    for tl, ql, n in ((80, 33, 257), (97, 35, 258), (97, 70, 385), (80, 5, 130)):
        t1, q1 = _pairs(tl, ql, n, 100 * tl + ql, rows=(16, 17, 48, 49), cols=(32, 33, 64, 65))
        ts += t1
        qs += q1
    order = np.random.default_rng(9).permutation(len(ts))
    ts, qs = [ts[k] for k in order], [qs[k] for k in order]
    assert len(ts) >= 1024  # (the library sorts batches of 1 024 pairs and more)
    a = sw.MicrosoftSmithWaterman(0)
    a.set_small_kernel(1)
    try:
        for strategy in (ol.SOFTCLIP, ol.INDEL):
            _both_forms(a, monkeypatch, "grouped", ts, qs, GATK, strategy, cigar_stride=256)
    finally:
        a.close()
