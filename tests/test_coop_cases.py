"""tests/coop_cases.py on the CPU: the restated geometry of the workgroup kernels at its edges, the planner's switch between the 16-bit
and the int32 form exactly where the restated coop16_worthwhile says, and the cases of every family doing what they were built for
-- judged from the oracle's CIGARs and scores alone, no GPU."""
import pytest

import coop_cases as cc
import oracle_lib as ol
from mgl_amd import _lib

COOP, COOP16 = 3, 5
COMBOS = [(form, W) for form in cc.FORMS for W in cc.WAVES]


def test_geometry():
    assert [cc.sps32(q) for q in (1, 32, 33, 64, 65)] == [96, 96, 128, 128, 160]
    assert [cc.sps16(q) for q in (1, 31, 32, 63, 64)] == [160, 160, 192, 192, 224]
    # S: a multiple of the ring that holds the steps of a stripe and 64 more
    for form in cc.FORMS:
        for ql in range(1, 700):
            s = cc.seq_numbers(form, ql)
            assert s % cc.RING_COLS == 0 and s - cc.RING_COLS < cc.sps(form, ql) + 64 <= s
    assert [cc.seq_numbers(32, q) for q in (128, 129, 384, 385)] == [256, 512, 512, 768]
    assert [cc.seq_numbers(16, q) for q in (63, 64, 319, 320, 575, 576)] == [256, 512, 512, 768, 768, 1024]
    assert [cc.main_hi(q) for q in (31, 32, 33, 159, 160)] == [0, 32, 32, 128, 160]
    assert [cc.wrap_tag(k, 4) for k in (0, 3, 4, 7, 8, 4 * 0x7fff, 4 * 0x8000)] == [1, 1, 2, 2, 3, 0x8000, 1]   # never 0
    assert cc.seam_rows(32, 2) == [64, 128, 256] and cc.seam_rows(32, 4) == [64, 128, 192, 256, 512]
    assert cc.seam_rows(16, 4) == [128, 256, 384, 512, 1024] and cc.hbm_rows(16, 16) == [2048, 4096]
    assert cc.seam_rows(16, 16)[-3:] == [1920, 2048, 4096] and len(cc.seam_rows(16, 16)) == 17
    assert cc.owner(32, 4, 256) == (0, 3) and cc.owner(32, 4, 257) == (1, 0) and cc.owner(16, 2, 513) == (2, 0)


@pytest.mark.parametrize("form,W", COMBOS, ids=str)
def test_lengths(form, W):
    r = cc.R[form]
    tls, qls = cc.tl_values(form, W), cc.ql_values(form)
    assert {cc.stripes(form, tl) for tl in tls} >= {1, W - 1, W, W + 1, 2 * W, 2 * W + 1, 2 * W + 2} - {0}
    for n in (1, W - 1, W, W + 1, 2 * W, 2 * W + 1):
        assert {r * n - 1, r * n, r * n + 1} <= set(tls)
    if form == 16:   # the owner of row tl: lane 0 low and high, lane 63 low and high
        assert {tl % 128 for tl in tls} == {1, 2, 127, 0}
    assert {1, 2, 3, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 159, 160, 161, 255, 256, 257, 511, 512, 513} <= set(qls)
    steps = [q for q in range(2, cc.MAX_QL + 1) if cc.seq_numbers(form, q) != cc.seq_numbers(form, q - 1)]
    assert len(steps) >= 2 and all({q - 1, q} <= set(qls) for q in steps)


def test_the_16_bit_form_s_guards_at_their_edges():
    """the largest match of (m, -150, 260, 11) that coop16_worthwhile / coop16_possible pass, and the planner's switch from
    sw_dp_coop16_kernel to sw_dp_coop_kernel exactly behind the first, on a shape that takes these kernels on a default context"""
    def last(pred):
        m = max(x for x in range(1, 4001) if pred(x, -150, 260, 11))
        assert all(pred(x, -150, 260, 11) for x in range(1, m + 1)) and not pred(m + 1, -150, 260, 11)
        return m

    worth, possible = last(cc.coop16_worthwhile), last(cc.coop16_possible)
    assert 200 < worth < possible < 4000
    # the two formulas, by hand, at the edge: margins, and 128 PEs of match + 2e each
    margin = lambda m: (34 * 249 + 2 * (m + 271) + 249 + 128 + 64) + (34 * (m + 271) + 260 + m + 22 + 64)
    assert margin(possible) <= 60000 < margin(possible + 1)
    assert 128 * (worth + 22) + 2 * 249 + margin(worth) <= 64000 < 128 * (worth + 1 + 22) + 2 * 249 + margin(worth + 1)
    for m, want in ((200, COOP16), (worth, COOP16), (worth + 1, COOP), (possible, COOP), (possible + 1, COOP)):
        p = _lib.explain(n=8, max_tl=31000, max_ql=70000, parameters=(m, -150, 260, 11))
        assert p.fill_kernel == want, (m, p.fill_kernel)
    # what else coop16_possible refuses: constants that do not pack, a gap that opens for less than it extends
    for params in ((0, -1, 1, 1), (5, 6, 1, 1), (5, -3, 2, 9), (5, -3, 1, -1), (4001, -3, 1, 1), (5, -4001, 1, 1), (5, -3, 4001, 1)):
        assert not cc.coop16_possible(*params), params
    assert cc.coop16_possible(4000, -4000, 1, 1) is False and cc.coop16_possible(5, -3, 4000, 4000) is False   # (the margins)
    assert all(cc.coop16_worthwhile(*p) for p in (cc.GATK,) + cc.TIE_PARAMS)


def test_path_rows_ops():
    rows, runs = cc.path_rows_ops(3, "2S4M3I2D5M1S", 15)
    assert rows == {4: ("M", 4), 5: ("M", 4), 6: ("M", 4), 7: ("M", 4), 8: ("D", 2), 9: ("D", 2), 10: ("M", 5), 11: ("M", 5), 12: ("M", 5),
                    13: ("M", 5), 14: ("M", 5)}
    assert runs == [(7, 7, 9)]


@pytest.mark.parametrize("form,W", COMBOS, ids=str)
def test_the_cases_mean_what_they_say(form, W):
    cs = cc.cases_for(form, W)
    r = cc.R[form]
    assert cs[0].intent.family == "anchor" and len(cs[0].target) >= r * W
    assert all(1 <= len(c.query) <= cc.MAX_QL or (c.intent.family in ("row_tl", "col_ql") and len(c.query) == 513) for c in cs)
    assert max(len(c.target) for c in cs) <= 2 * 16 * 128 + 129 + 330   # (a run of 129 rows behind the last seam, and a flank)
    for idx in cc.batches(cs).values():
        assert idx[0] == 0 and len(idx) >= 2
    # ---- every case does what it says: nothing is left to the builders' word
    met = {}
    for c in cs:
        ok = cc.intent_met(c, form, W)
        if ok is not None:
            met.setdefault(c.intent.family, []).append(ok)
            assert ok, (form, W, c.intent, c.params, c.strategy)
    # ---- and every seam has its cases
    seams = cc.seam_rows(form, W) if W <= 4 else cc.hbm_rows(form, W)
    by = lambda fam: [c for c in cs if c.intent.family == fam]
    assert {c.intent.row for c in by("diag")} == set(seams)
    for b in seams:
        dels = {(c.intent.first, c.intent.last - c.intent.first + 1) for c in by("del") if c.intent.row == b}
        assert dels == set(cc.del_placements(form, b))
        lengths = sorted(set(cc.DEL_RUNS) | {r + 1})
        if b >= r + 1 + cc.MIN_FLANK:    # (nearer to row 1 the longer runs have no room above the seam)
            assert {n for f, n in dels if f + n - 1 == b} == set(lengths), "ends exactly on b"
        assert {n for f, n in dels if f == b + 1} == set(lengths), "starts exactly on b + 1"
        assert {n for f, n in dels if f <= b < f + n - 1} >= set(lengths) - {1}, "straddles b"
        assert {(c.intent.first, c.intent.col) for c in by("ins") if c.intent.row == b} == {(b + 1, 96), (b + 1, 256), (b, 96), (b, 256)}
    assert {s for c in by("diag") + by("del") + by("ins") for s in [c.strategy]} == set(cc.STRATEGIES)
    # the HBM rows of both rounds: a deletion run whose E' travels through the hop, tags 2 and 3
    for k, b in enumerate(cc.hbm_rows(form, W)):
        assert cc.owner(form, W, b) == (k, W - 1) and cc.owner(form, W, b + 1) == (k + 1, 0) and cc.wrap_tag(b // r, W) == k + 2
        assert any(c.intent.first <= b < c.intent.last for c in by("del") if c.intent.row == b)
    # ---- lengths: every tl and every ql, both named corners, every strategy
    lens = by("row_tl") + by("col_ql")
    assert {len(c.target) for c in lens} >= set(cc.tl_values(form, W)) and {len(c.query) for c in lens} >= set(cc.ql_values(form))
    assert (1, 513) in {(len(c.target), len(c.query)) for c in lens}
    assert {(2 * W * r + 1, q) for q in (1, 2, 3)} <= {(len(c.target), len(c.query)) for c in lens}
    assert {c.strategy for c in lens} == set(cc.STRATEGIES)
    # ---- ties: both periodic patterns tie across waves and rounds under both strategies without a border
    ties = by("ties")
    assert all(cc.stripes(form, len(c.target)) == 2 * W + 1 for c in ties)
    assert {c.params for c in ties} == set(cc.TIE_PARAMS) and {c.strategy for c in ties} == set(cc.STRATEGIES)
    assert sum(c.intent.col == 1 for c in ties) == 8 and len(met["ties"]) >= 8
    if (form, W) in ((32, 2), (32, 4), (16, 2)):   # where 2 W + 1 stripes are shorter than the longest query: the last row decides
        assert sum(c.intent.col == 2 for c in ties) == 4
    # ---- the 16-bit field of the HBM row at its bounds
    if form == 32 and W <= 4:
        b = cc.hbm_rows(32, W)[0]
        assert {c.params for c in by("gap_field")} == set(cc.FIELD_PARAMS) and {c.params for c in by("gap_refused")} == set(cc.FIELD_REFUSED)
        assert all(c.intent.first <= b + 1 <= c.intent.last + 1 and len(c.target) + len(c.query) <= 2000 for c in by("gap_field") + by("gap_refused"))
        assert all(any(c.intent.first <= b < c.intent.last for c in by("gap_field") if c.params == p) for p in cc.FIELD_PARAMS)
        assert len(met["gap_field"]) == 9
    else:
        assert not by("gap_field")
    # ---- mixed: one batch per strategy, every stripe count, in an order that is not sorted
    for s in cc.STRATEGIES:
        idx = cc.batches(cs)[(cc.GATK, s, "mixed")]
        counts = [cc.stripes(form, len(cs[k].target)) for k in idx[1:]]
        assert set(counts) == {1, 2, W - 1, W, W + 1, 2 * W, 2 * W + 1} and counts != sorted(counts) and len(counts) == 14


def test_one_tie_is_decided_by_the_last_row():
    cs = [c for form, W in ((32, 2), (32, 4), (16, 2)) for c in cc.cases_for(form, W) if c.intent.family == "ties" and c.intent.col == 2]
    assert cs
    for c in cs:
        mqe, mqe_t, mx, max_t, max_q, seg = ol.oracle_align(c.target, c.query, c.params, c.strategy)["score"]
        assert max_t == len(c.target) and mx == mqe and mqe_t == len(c.target) and max_q == len(c.target) and seg == len(c.query) - max_q
