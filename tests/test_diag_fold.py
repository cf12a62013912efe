"""The folded diagonal (sw_device.h: diag_fold) as the planner reports it (mgl_sw_explain, no GPU): for parameter sets where some K and two
bytes b_m, b_x in [0, 255] give b_m K == match + 2 gext and b_x K == mismatch + 2 gext (mod 2^16), the base-code forms of the checkpointed
lane kernel and of the long-read strip kernel form the diagonal in one multiply-add; mgl_sw_plan.diag_fold is that K, 0 for none."""
import numpy as np
import pytest

from mgl_amd import _lib

GATK = (200, -150, 260, 11)
LANE16_CK, STRIP16 = 7, 6
BENCH_WS = 208 << 30
FOLDS = [GATK, (3, -1, 4, 3), (1, -1, 1, 1), (2, -1, 2, 1), (1, -3, 5, 2)]
NO_FOLD = [(25, -50, 110, 6), (10, -15, 30, 5), (1, -4, 6, 1), (5, -4, 10, 1)]

_B = np.arange(256, dtype=np.int64)


def brute(match, mismatch, gext):
    """The smallest K in [1, 2^16) for which both constants are some byte times K (mod 2^16), or 0."""
    a, x = (match + 2 * gext) & 0xFFFF, (mismatch + 2 * gext) & 0xFFFF
    prod = (np.arange(1 << 16, dtype=np.int64)[:, None] * _B[None, :]) & 0xFFFF   # [K][byte]
    ok = (prod == a).any(axis=1) & (prod == x).any(axis=1)
    ok[0] = False
    return int(np.argmax(ok)) if ok.any() else 0


def bytes_for(k, match, mismatch, gext):
    prod = (k * _B) & 0xFFFF
    bm = np.flatnonzero(prod == (match + 2 * gext) & 0xFFFF)
    bx = np.flatnonzero(prod == (mismatch + 2 * gext) & 0xFFFF)
    return bm, bx


def lane_plan(params):
    return _lib.explain(n=10_000_000, max_tl=256, max_ql=150, parameters=params, flags=_lib.FLAG_UNIFORM_GEOMETRY, workspace=BENCH_WS)


def strip_plan(params):
    return _lib.explain(n=2304, max_tl=4608, max_ql=4608, parameters=params, workspace=BENCH_WS)


def random_sets(n, seed=20261016):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        gext = int(rng.integers(0, 20))
        out.append((int(rng.integers(1, 40)), -int(rng.integers(1, 60)), gext + int(rng.integers(0, 60)), gext))
    return out


def test_gatk_folds_on_the_headline_and_the_long_reads():
    p = lane_plan(GATK)
    assert p.fill_kernel == LANE16_CK and p.diag_fold == 20138
    bm, bx = bytes_for(20138, 200, -150, 11)
    assert 179 in bm and 192 in bx
    p = strip_plan(GATK)
    assert p.fill_kernel == STRIP16 and p.traceback == 1 and p.diag_fold == 20138


@pytest.mark.parametrize("params", FOLDS + NO_FOLD, ids=str)
def test_the_issue_table(params):
    p = lane_plan(params)
    assert p.fill_kernel == LANE16_CK
    assert (p.diag_fold != 0) == (params in FOLDS)
    assert p.diag_fold == brute(params[0], params[1], params[3])


def test_random_sets_agree_with_a_brute_force():
    n_lane = n_fold = 0
    for params in random_sets(300):
        p = lane_plan(params)
        want = brute(params[0], params[1], params[3])
        if p.fill_kernel != LANE16_CK:
            assert p.diag_fold == 0, params
            continue
        n_lane += 1
        assert p.diag_fold == want, params
        if want:
            n_fold += 1
            bm, bx = bytes_for(want, params[0], params[1], params[3])
            assert len(bm) and len(bx), params
    assert n_lane >= 250 and 0 < n_fold < n_lane


def test_other_kernels_report_none():
    assert _lib.explain(n=16, max_tl=256, max_ql=150, parameters=GATK).diag_fold == 0          # one wave per pair (sw_small_kernel)
    p = _lib.explain(n=2304, max_tl=4608, max_ql=4608, parameters=(25, -50, 110, 6), workspace=BENCH_WS)
    assert p.diag_fold == 0


def test_the_debug_switch_turns_it_off(monkeypatch):
    monkeypatch.setenv("MGL_SW_DEBUG_DIAG_FOLD", "0")
    assert lane_plan(GATK).diag_fold == 0 and strip_plan(GATK).diag_fold == 0
    monkeypatch.setenv("MGL_SW_DEBUG_DIAG_FOLD", "1")
    assert lane_plan(GATK).diag_fold == 20138
