"""The workgroup kernels (sw_dp_coop.hip: sw_dp_coop_kernel and its 16-bit form sw_dp_coop16_kernel) at 2, 4 and 16 waves per pair
on the pairs of tests/coop_cases.py, whose paths, lengths and ties lie on the kernels' own seams -- the LDS ring from wave to wave,
the HBM row from the last wave back to wave 0 with its tags and its 16-bit H - E' field, the 32-step groups, the ring's lap, the
lane that owns row tl, waves left idle by a short pair -- bit for bit against the oracle: offset, CIGAR, all six score fields, and
the backtrack matrix cell for cell.  The waves per pair are forced, the anchor of every batch makes the planner keep them, and both
are asserted through mgl_sw_explain on the forced context and from the timing record after the run."""
import os

import numpy as np
import pytest

import coop_cases as cc
import oracle_lib as ol
from mgl_amd import _lib, smithwaterman as sw

pytestmark = pytest.mark.gpu

COOP, COOP16 = 3, 5
KERNEL = {32: COOP, 16: COOP16}
LAYOUT = {32: 0, 16: 3}
COMBOS = [(form, W) for form in cc.FORMS for W in cc.WAVES]
LATE = (300, -300, 310, 10)   # test_window_fails_late


def _forced(form, W, precision=None):
    a = sw.MicrosoftSmithWaterman(0)
    a.set_cooperative(W)
    a.set_precision(32 if form == 32 else 0 if precision is None else precision)
    return a


def _stride(ts, qs):
    return 4 * (max(map(len, ts)) + max(map(len, qs))) + 16


def _run(a, ts, qs, params, strategy, W, kernel):
    """one batch on the forced context: the planner keeps W waves and the kernel, before and after"""
    if kernel is not None:
        p = _lib.explain(n=len(ts), max_tl=max(map(len, ts)), max_ql=max(map(len, qs)), parameters=params, strategy=strategy, ctx=a.ctx)
        assert (p.fill_kernel, p.waves_per_pair) == (kernel, W), (params, strategy, p.fill_kernel, p.waves_per_pair)
    res = a.align_batch(ts, qs, params, strategy, cigar_stride=_stride(ts, qs))   # (raises on any status but 0)
    if kernel is not None:
        assert a.timing().fill_kernel == kernel, (params, strategy, a.timing().fill_kernel)
    return res


def _compare(res, want, where):
    off, score, cg = want
    for n in range(len(cg)):
        got = (int(res.offsets[n]), res.cigars[n], tuple(int(x) for x in res.scores[n]))
        assert got == (int(off[n]), cg[n], tuple(int(x) for x in score[n])), where(n)


def _batches(cs, families=None):
    """[(params, strategy, case indices)] of the cases, the anchor first in each"""
    return [(params, strategy, idx) for (params, strategy, _), idx in sorted(cc.batches(cs).items(), key=lambda kv: str(kv[0]))
            if families is None or cs[idx[1]].intent.family in families]


@pytest.mark.parametrize("form,W", COMBOS, ids=str)
def test_seams(form, W):
    cs = cc.cases_for(form, W)
    a = _forced(form, W)
    try:
        for params, strategy, idx in _batches(cs):
            if cs[idx[1]].intent.family == "gap_refused":
                continue   # test_gap_field_bound
            ts, qs = [cs[k].target for k in idx], [cs[k].query for k in idx]
            want = ol.oracle_align_batch(ts, qs, params, strategy, nthreads=16)
            res = _run(a, ts, qs, params, strategy, W, KERNEL[form])
            assert all(a.slot_layout(n) == LAYOUT[form] for n in range(len(idx))), (form, W, params, strategy)
            _compare(res, want, lambda n: (form, W, params, strategy, idx[n], cs[idx[n]].intent))
    finally:
        a.close()


def _cell_cases(form, W):
    """the del and ins cases on the first HBM row, row tl at R W - 1 and R W + 1, one tie"""
    cs = cc.cases_for(form, W)
    b = cc.hbm_rows(form, W)[0]
    dels = [k for k, c in enumerate(cs) if c.intent.family == "del" and c.intent.row == b]
    keep = [k for k in dels if cs[k].intent.last - cs[k].intent.first + 1 in (2, 65, cc.R[form] + 1) and cs[k].intent.first <= b + 1 <= cs[k].intent.last + 1][:6]
    keep += [k for k, c in enumerate(cs) if c.intent.family == "ins" and c.intent.row == b]
    for tl in (b - 1, b + 1):
        keep.append(next(k for k, c in enumerate(cs) if c.intent.family in ("row_tl", "col_ql") and len(c.target) == tl))
    keep.append(next(k for k, c in enumerate(cs) if c.intent.family == "ties" and c.intent.col == 1 and c.params == cc.TIE_PARAMS[1]))
    return cs, keep


@pytest.mark.parametrize("form,W", [(form, W) for form in cc.FORMS for W in (2, 4)], ids=str)
def test_backtrack_cell_for_cell(form, W):
    cs, keep = _cell_cases(form, W)
    assert 10 <= len(keep) <= 14
    by = {}
    for k in keep:
        by.setdefault((cs[k].params, cs[k].strategy), [0]).append(k)
    a = _forced(form, W)
    try:
        for (params, strategy), idx in sorted(by.items()):
            ts, qs = [cs[k].target for k in idx], [cs[k].query for k in idx]
            _run(a, ts, qs, params, strategy, W, KERNEL[form])
            for n, k in enumerate(idx):
                assert a.slot_layout(n) == LAYOUT[form]
                want = ol.oracle_align(ts[n], qs[n], params, strategy, want_btr=True)["btr"][1:, 1:]
                got = a.expand_slot(n, len(ts[n]), len(qs[n]))[1:, 1:]
                if not np.array_equal(got, want):
                    i, j = (int(x[0]) + 1 for x in np.nonzero(got != want))
                    raise AssertionError((form, W, cs[k].intent, params, strategy, "first differing (row, column)", (i, j), int(got[i - 1, j - 1]), int(want[i - 1, j - 1])))
    finally:
        a.close()


@pytest.mark.parametrize("W", [2, 4], ids=str)
def test_gap_field_bound(W):
    """o - e = 65535 fills the HBM row's 16-bit H - E' field to the last bit and o - e = 0 empties it: sw_dp_coop_kernel, equal to the
    oracle.  A gap open of 65536 or one below the gap extension is beyond the planner's guard: another kernel, equal to the oracle."""
    cs = cc.cases_for(32, W)
    a = _forced(32, W)
    seen = set()
    try:
        for params, strategy, idx in _batches(cs, ("gap_field", "gap_refused")):
            ts, qs = [cs[k].target for k in idx], [cs[k].query for k in idx]
            want = ol.oracle_align_batch(ts, qs, params, strategy, nthreads=16)
            if params in cc.FIELD_PARAMS:
                res = _run(a, ts, qs, params, strategy, W, COOP)
            else:
                p = _lib.explain(n=len(ts), max_tl=max(map(len, ts)), max_ql=max(map(len, qs)), parameters=params, strategy=strategy, ctx=a.ctx)
                assert p.fill_kernel not in (COOP, COOP16)
                res = _run(a, ts, qs, params, strategy, W, None)
                assert a.timing().fill_kernel not in (COOP, COOP16)
            seen.add(params)
            _compare(res, want, lambda n: (W, params, strategy, idx[n], cs[idx[n]].intent))
    finally:
        a.close()
    assert seen == set(cc.FIELD_PARAMS + cc.FIELD_REFUSED)


def _late_batch(W, rng):
    """P: the first 128 W target rows have nothing to do with the query -- a spread of H over a wave's 128 rows of under 25 000 -- and
    the rows behind them copy it: 127 matches on an anti-diagonal of 128 rows spread 127 (match + 2 e); P cut to its first 128 W
    rows; pairs whose queries of 60 bases cannot spread further than 60 (match + 2 e)"""
    q = cc._rand(rng, 300)
    t = np.concatenate([cc._unrelated(rng, 128 * W, q), q, cc._rand(rng, 20)])
    stay = []
    for lo in (40, 128 * W - 30, 128 * W + 50):
        t2 = cc._rand(rng, 128 * W + 200)
        stay.append((cc._b(t2), cc._b(cc._noisy(rng, t2[lo:lo + 60]))))
    pairs = [(cc._b(t), cc._b(q))] + stay + [(cc._b(t[:128 * W]), cc._b(q))]
    return [p[0] for p in pairs], [p[1] for p in pairs]


@pytest.mark.parametrize("W", [2, 4], ids=str)
def test_window_fails_late(W):
    """A window check of sw_dp_coop16_kernel that fails only in the second round, after the HBM row has been written and read in 16
    bits: the workgroup redoes the pair with the int32 body over the same LDS and the same HBM row, beside pairs of the same launch
    that stay in 16 bits.  Parameters (300, -300, 310, 10): coop16_possible (margins 33 858 of 65 535) and not coop16_worthwhile;
    precision 16 forces the attempt.  Observed on an MI355X, W = 2 and 4 alike: pair 0 (P) layout 0, pairs 1 .. 3 and pair 4 (P cut to
    its first 128 W rows) layout 3."""
    assert cc.coop16_possible(*LATE) and not cc.coop16_worthwhile(*LATE)
    ts, qs = _late_batch(W, np.random.default_rng(1600 + W))
    a = _forced(16, W, precision=16)
    try:
        for strategy in (cc.SOFTCLIP, cc.INDEL):
            want = ol.oracle_align_batch(ts, qs, LATE, strategy, nthreads=16)
            res = _run(a, ts, qs, LATE, strategy, W, COOP16)
            assert a.timing().dp_launches == 1   # both layouts come out of ONE launch
            layouts = [a.slot_layout(n) for n in range(len(ts))]
            print("test_window_fails_late", W, strategy, "layouts", layouts)
            assert layouts[-1] == 3, layouts     # P's first round alone fits
            assert layouts[0] == 0, layouts      # ... P does not
            assert layouts[1:-1] == [3] * (len(ts) - 2), layouts
            _compare(res, want, lambda n: (W, strategy, n, layouts))
    finally:
        a.close()


def test_one_pair_entry_on_the_seams():
    """mgl_sw_align, every call a direct call on the calling thread's context (four waves per pair): the HBM row of the 16-bit form +- 1
    against queries of 1 and 257 bases, and a tie across waves and rounds"""
    cs = cc.cases_for(16, 4)
    b = cc.hbm_rows(16, 4)[0]
    rng = np.random.default_rng(41)
    pairs = [cc.length_case(tl, ql, True, s, rng) for tl, ql, s in ((b - 1, 1, cc.SOFTCLIP), (b + 1, 1, cc.INDEL), (b, 257, cc.LEADING_INDEL),
                                                                    (b - 1, 257, cc.IGNORE), (b + 1, 257, cc.SOFTCLIP))]
    pairs.append(next(c for c in cs if c.intent.family == "ties" and c.intent.col == 1))
    pairs.append(next(c for c in cc.cases_for(32, 4) if c.intent.family == "ties" and c.intent.col == 2))
    sw.set_coalescing(0, 0)
    sw.set_service(0)
    try:
        for c in pairs:
            o = ol.oracle_align(c.target, c.query, c.params, c.strategy)
            cigar, off, ez = sw.align(c.target, c.query, c.params, c.strategy)
            assert (off, cigar, tuple(ez)) == (o["offset"], o["cigar"], tuple(o["score"])), (c.intent, c.params, c.strategy)
    finally:   # back to what the library starts with (sw_service.cpp: ServicePool(), sw_batcher.cpp: EnvInit)
        sw.set_service(int(os.environ.get("MGL_SW_SERVICE_SLOTS", 64)))
        us, batch = int(os.environ.get("MGL_SW_COALESCE_US", 50)), int(os.environ.get("MGL_SW_COALESCE_BATCH", 4096))
        if us >= 0 and batch > 0:
            sw.set_coalescing(batch, us)
