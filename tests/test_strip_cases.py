"""tests/strip_cases.py on the CPU: the planner takes the strip height height_interval() says at both ends of every interval, and the
cases built for a height do what they were built for -- judged from the oracle's CIGARs and scores alone, no GPU."""
import pytest

import oracle_lib as ol
import strip_cases as sc
from mgl_amd import _lib

STRIP16 = 6
COMBOS = [(sr, w, 1) for w in (1, 2, 4) for sr in range(17, 33)] + [(sr, 4, 2) for sr in range(22, 33)] + [(22, 4, 3), (23, 4, 3)]


def test_intervals_tile_the_targets():
    """the intervals of one (waves, passes) follow each other without a gap, and the table the planner was measured with"""
    for w, p, floor in ((1, 1, 17), (2, 1, 17), (4, 1, 17), (4, 2, 22), (4, 3, 22)):
        for sr in range(floor, 32):
            assert sc.height_interval(sr, w, p)[1] + 1 == sc.height_interval(sr + 1, w, p)[0]
    assert sc.height_interval(17, 1, 1)[1] == 2176 and sc.height_interval(32, 1, 1) == (3969, 4096)
    assert sc.height_interval(17, 2, 1) == (4097, 4352) and sc.height_interval(32, 2, 1) == (7937, 8192)
    assert sc.height_interval(17, 4, 1) == (8193, 8704) and sc.height_interval(32, 4, 1) == (15873, 16384)
    assert sc.height_interval(22, 4, 2) == (16385, 22528) and sc.height_interval(32, 4, 2) == (31745, 32768)
    assert sc.height_interval(22, 4, 3) == (32769, 33792) and sc.height_interval(23, 4, 3)[0] == 33793
    assert sc.height_interval(21, 4, 1)[0] <= 10300 <= sc.height_interval(21, 4, 1)[1]
    with pytest.raises(ValueError):
        sc.height_interval(21, 4, 2)


@pytest.mark.parametrize("sr,waves,passes", COMBOS, ids=str)
def test_the_planner_takes_this_height(sr, waves, passes):
    lo, hi = sc.height_interval(sr, waves, passes)
    # the first target behind the interval: the next height, or the first height of twice the waves or of one pass more
    behind = (sr + 1, waves) if sr < 32 else (17, 2 * waves) if waves < 4 else (22, 4)
    for tl, want in ((lo, (sr, waves)), (hi, (sr, waves)), (hi + 1, behind)):
        p = _lib.explain(n=64, max_tl=tl, max_ql=tl, parameters=sc.GATK)
        assert p.fill_kernel == STRIP16, (tl, p.fill_kernel)
        assert (p.rows, p.waves_per_pair) == want, (tl, p.rows, p.waves_per_pair)
    if lo == sc.first_strip_target():
        assert _lib.explain(n=64, max_tl=lo - 1, max_ql=lo - 1, parameters=sc.GATK).fill_kernel != STRIP16


def test_seam_strips():
    assert sc.seam_strips(1) == [0, 1, 63, 64, 127]
    assert sc.seam_strips(2) == [0, 1, 63, 64, 127, 128, 191, 192, 255]
    assert sc.seam_strips(4) == [0, 1, 63, 64, 255, 256, 319, 320, 511]
    assert sc.seam_strips(4, 2) == [0, 1, 63, 64, 255, 256, 319, 320, 511, 512, 1023]
    assert sc.seam_strips(4, 3) == [0, 1, 63, 64, 255, 256, 319, 320, 511, 512, 1023, 1024, 1535]


def test_path_rows_ops():
    cross, runs = sc.path_rows_ops(3, "2S4M3I2D5M1S", 20, 15)
    assert cross == {3: ("M", 4), 4: ("M", 4), 5: ("M", 4), 6: ("M", 4), 7: ("D", 2), 8: ("D", 2), 9: ("M", 5), 10: ("M", 5), 11: ("M", 5),
                     12: ("M", 5), 13: ("M", 5)}
    assert runs == [(7, 7, 9)]


def _oracle(cs):
    """the oracle's (offset, CIGAR, score) of every case, a batch per strategy"""
    out = [None] * len(cs)
    for strategy, idx in sc.batches(cs).items():
        off, score, cg = ol.oracle_align_batch([cs[k].target for k in idx], [cs[k].query for k in idx], sc.GATK, strategy, nthreads=8)
        for n, k in enumerate(idx):
            out[k] = (int(off[n]), cg[n], tuple(int(x) for x in score[n]))
    return out


def _check_cases(cs, sr, waves, passes, full):
    lo, hi = sc.height_interval(sr, waves, passes)
    assert cs[0].intent.family == "anchor" and len(cs[0].target) == hi
    assert all(len(c.target) <= hi and 1 <= len(c.query) <= sc.MAX_QL for c in cs)
    for idx in sc.batches(cs).values():
        assert idx[0] == 0 and max(len(cs[k].target) for k in idx) == hi
    # (the pass seams lie beyond the reach of LEADING_INDEL's border: strip_cases.strategy_of)
    assert {c.strategy for c in cs} == (set(sc.STRATEGIES) if full else {sc.SOFTCLIP, sc.INDEL, sc.IGNORE})
    k_ = sc.bands_k(sr)
    for c in cs:
        it = c.intent
        if it.family == "insck":   # a checkpoint column of the band of row b + 1
            assert (it.col + sc.CPS * k_ * (it.row // (sr * k_))) % sc.CK_COLS == 0 and len(c.query) >= 140
        if it.family == "ins16":
            assert it.col % 16 == 0
    res = _oracle(cs)
    met = {}
    for c, (off, cg, score) in zip(cs, res):
        ok = sc.intent_met(c, off, cg, score, sr)
        if ok is not None:
            fam = "bytes" if c.intent.family.startswith("bytes") else c.intent.family
            met.setdefault(fam, []).append(bool(ok))
    assert set(met) == ({"row_tl", "col_tl", "diag", "del", "ins16", "insck", "bytes"} if full else {"row_tl", "diag", "del", "ins16", "insck"})
    for fam, oks in met.items():
        assert (len(oks) - sum(oks)) * 10 <= len(oks), (sr, waves, passes, fam, len(oks) - sum(oks), len(oks))
    return res


@pytest.mark.parametrize("sr,waves,passes", [(sr, w, 1) for sr in (17, 21, 22, 26, 27, 32) for w in (1, 2, 4)] + [(22, 4, 2), (32, 4, 2), (22, 4, 3)], ids=str)
def test_the_cases_mean_what_they_say(sr, waves, passes):
    cs = sc.cases(sr, waves, passes, sc.rng_for(sr, waves, passes))
    _check_cases(cs, sr, waves, passes, full=True)
    # coverage: row tl on every register row; its owners lane 0 and lane 63 of every wave, in either half; every seam a boundary
    rows = [c.intent for c in cs if c.intent.family in ("row_tl", "col_tl")]
    assert {(len(c.target) - 1) % sr for c in cs if c.intent.family == "row_tl"} == set(range(sr)), "the last row decides on every register row"
    assert {it.r for it in rows if it.family == "col_tl"} == set(range(1, sr, 2))
    assert all(it.strip == (it.row - 1) // sr and it.r == (it.row - 1) % sr for it in rows)
    owners = {sc.owner(it.strip, waves)[1:] for it in rows}
    assert {(h, w, l) for h in (0, 1) for w in range(waves) for l in (0, 63)} <= owners
    assert set(sc.seam_strips(waves, passes)) <= {it.strip for it in rows}
    bounds = {c.intent.row for c in cs if c.intent.family == "diag"}
    assert {sr * g for g in sc.seam_strips(waves, passes) if g} <= bounds
    assert any(b % (sr * sc.bands_k(sr)) == 0 for b in bounds)
    assert sorted(len(c.query) for c in cs if c.intent.family == "tiny") == sorted(sc.TINY_QL)
    fams = [c.intent.family for c in cs]
    assert fams.count("diag") == fams.count("del") == fams.count("ins16") == fams.count("insck") == len(bounds)


@pytest.mark.parametrize("sr,passes", [(22, 2), (32, 2), (22, 3)], ids=str)
def test_the_pass_seam_cases_mean_what_they_say(sr, passes):
    cs = sc.pass_cases(sr, passes, sc.rng_for(sr, 4, passes, pass_seams=True))
    _check_cases(cs, sr, 4, passes, full=False)
    assert {c.intent.row for c in cs if c.intent.family == "diag"} == {512 * sr * p for p in range(1, passes)}
    assert {c.intent.strip for c in cs if c.intent.family == "row_tl"} == {512, 1023}
