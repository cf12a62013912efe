"""Every strip height of the long-read strip kernel (sw_dp16_strip.hip: 17 .. 32 rows, three entry points and four bodies each) on
one, two and four waves and in two and three passes, on the pairs of tests/strip_cases.py whose paths cross the kernel's seams --
the register row of target row tl, lane 63 -> lane 0 of the next wave, the low halves -> the high halves, a pass -> the next, the
kept rows, the band-shifted checkpoint columns, the baseline's moves -- bit for bit against the oracle: offset, CIGAR and all six
score fields.  The height is the planner's own choice for the batch's longest target (the anchor of every batch), asserted through
mgl_sw_explain on the forced context."""
from collections import namedtuple

import pytest

import oracle_lib as ol
import strip_cases as sc
from mgl_amd import _lib, smithwaterman as sw

pytestmark = pytest.mark.gpu

STRIP16 = 6
KEPT_BODIES = ("fold", "codes", "bytes")   # layout 6: <SR, true, CMP_FOLD>, <SR, true, CMP_CODES>, <SR, true, CMP_BYTES>
BODIES = KEPT_BODIES + ("stored",)         # layout 4: <SR, false, CMP_BYTES>
ENV = {"codes": ("MGL_SW_DEBUG_DIAG_FOLD", "0"), "bytes": ("MGL_SW_DEBUG_STRIP_CODES", "0")}


@pytest.fixture(scope="module")
def forced():
    a = sw.MicrosoftSmithWaterman(0)
    a.set_small_kernel(1)
    a.set_strip_kernel(2)
    yield a
    a.close()


def _oracle(cs, params):
    """[(strategy, case indices, offsets, scores, CIGARs)]: the oracle on every batch of the cases, once"""
    out = []
    for strategy, idx in sorted(sc.batches(cs).items()):
        off, score, cg = ol.oracle_align_batch([cs[k].target for k in idx], [cs[k].query for k in idx], params, strategy, nthreads=16)
        out.append((strategy, idx, off, score, cg))
    return out


def _run(a, body, monkeypatch, ts, qs, params, strategy):
    """one batch through one body of the kernel"""
    if body in ENV:
        monkeypatch.setenv(*ENV[body])
    if body == "stored":
        a.set_lane_checkpoint(1)
    try:
        return a.align_batch(ts, qs, params, strategy)   # (raises on any status but 0)
    finally:
        if body in ENV:
            monkeypatch.delenv(ENV[body][0])
        if body == "stored":
            a.set_lane_checkpoint(0)


def _planned(a, ts, qs, params, strategy):
    return _lib.explain(n=len(ts), max_tl=max(map(len, ts)), max_ql=max(map(len, qs)), parameters=params, strategy=strategy, ctx=a.ctx)


def _compare(res, cs, idx, off, score, cg, where):
    for n, k in enumerate(idx):
        got = (int(res.offsets[n]), res.cigars[n], tuple(int(x) for x in res.scores[n]))
        want = (int(off[n]), cg[n], tuple(int(x) for x in score[n]))
        assert got == want, where + (k, cs[k].intent, cs[k].strategy)


def _check_bodies(a, monkeypatch, cs, oracle, params, bodies, sr, waves):
    for strategy, idx, off, score, cg in oracle:
        ts, qs = [cs[k].target for k in idx], [cs[k].query for k in idx]
        p = _planned(a, ts, qs, params, strategy)
        assert (p.fill_kernel, p.rows, p.waves_per_pair) == (STRIP16, sr, waves), (sr, waves, strategy, p.fill_kernel, p.rows, p.waves_per_pair)
        for body in bodies:
            res = _run(a, body, monkeypatch, ts, qs, params, strategy)
            assert a.timing().fill_kernel == STRIP16, (sr, waves, body, strategy)
            layout = 4 if body == "stored" else 6
            assert all(a.slot_layout(n) == layout for n in range(len(idx))), (sr, waves, body, strategy)
            _compare(res, cs, idx, off, score, cg, (sr, waves, body))


def _check_packed(a, cs, sr, waves):
    """the pairs that are all ACGT as 2-bit packed input at unaligned base offsets: byte for byte what the ASCII run gives"""
    import torch
    from test_gpu_parity import _packed_from_rows

    Row = namedtuple("Row", "t q")
    acgt = set(b"ACGT")
    rows = [Row(c.target, c.query) for c in cs if set(c.target) <= acgt and set(c.query) <= acgt]
    assert len(rows) >= len(cs) - 3 and rows[0].t == cs[0].target
    res = a.align_batch([r.t for r in rows], [r.q for r in rows], sc.GATK, sc.SOFTCLIP)
    assert a.timing().fill_kernel == STRIP16
    pb = _packed_from_rows(rows, torch.device("cuda", 0))
    pb.run(a, sc.GATK, sc.SOFTCLIP)
    torch.cuda.synchronize()
    assert a.timing().fill_kernel == STRIP16 and int((pb.status != 0).sum()) == 0
    off, score, cg = pb.offsets.cpu().numpy(), pb.scores.cpu().numpy(), pb.cigar_strings()
    assert (off == res.offsets).all() and (score == res.scores).all(), (sr, waves, "2-bit")
    assert list(cg) == [res.cigars[n] for n in range(len(rows))], (sr, waves, "2-bit")


@pytest.mark.parametrize("sr", range(17, 33), ids=str)
def test_height(forced, sr, monkeypatch):
    for waves in (1, 2, 4):
        cs = sc.cases(sr, waves, 1, sc.rng_for(sr, waves, 1))
        _check_bodies(forced, monkeypatch, cs, _oracle(cs, sc.GATK), sc.GATK, BODIES, sr, waves)
        _check_packed(forced, cs, sr, waves)
        if waves == 1:   # parameters that do not fold: the base-code body without the switch
            assert _planned(forced, [cs[0].target], [cs[0].query], sc.GATK, sc.SOFTCLIP).diag_fold != 0
            assert _planned(forced, [cs[0].target], [cs[0].query], sc.NOT_FOLDING, sc.SOFTCLIP).diag_fold == 0
            _check_bodies(forced, monkeypatch, cs, _oracle(cs, sc.NOT_FOLDING), sc.NOT_FOLDING, ("fold",), sr, waves)


@pytest.mark.parametrize("sr,passes", [(sr, 2) for sr in range(22, 33)] + [(22, 3)], ids=str)
def test_height_multi_pass(forced, sr, passes, monkeypatch):
    """rows 512 sr (and 1024 sr) enter the next pass through the row the pass before kept in HBM"""
    cs = sc.pass_cases(sr, passes, sc.rng_for(sr, 4, passes, pass_seams=True))
    oracle = _oracle(cs, sc.GATK)
    _check_bodies(forced, monkeypatch, cs, oracle, sc.GATK, KEPT_BODIES, sr, 4)
    if (sr, passes) == (22, 2):   # with every flag stored there is one pass only: such a batch leaves the strip kernel
        for strategy, idx, off, score, cg in oracle:
            res = _run(forced, "stored", monkeypatch, [cs[k].target for k in idx], [cs[k].query for k in idx], sc.GATK, strategy)
            assert forced.timing().fill_kernel != STRIP16
            _compare(res, cs, idx, off, score, cg, (sr, 4, "stored: another kernel"))
