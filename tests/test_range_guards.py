"""The 16-bit range guards of the DNA kernels, on the CPU: the mirrors of tests/range_guards.py pinned to the planner at each guard's
edge and one step past it (so a moved guard shows here before the GPU edge tests silently test inside it), a plain int64 reference
of the recurrence against the C restatement, and the strip kernel's static window evaluated on adversarial long inputs."""
import numpy as np
import pytest

import oracle_lib as ol
import range_guards as rg
from mgl_amd import _lib

GATK = (200, -150, 260, 11)
UNIFORM, SCORE_ONLY = _lib.FLAG_UNIFORM_GEOMETRY, _lib.FLAG_SCORE_ONLY
WS = 208 << 30
DP32, DP16, DP32_64, COOP, LANE16, COOP16, STRIP16, LANE16_CK, SMALL = range(9)

# (params, tl, largest admitted ql): the worked edges of the dp16 guard
DP16_EDGES = [(GATK, 300, 289), (GATK, 1200, 242)]
# strip16: `below` tight without a fold, `below` tight with a fold (K = 25378), `above` tight (K = 5)
STRIP_BELOW, STRIP_BELOW_FOLD, STRIP_ABOVE = (200, -867, 260, 11), (50, -3900, 260, 2), (44, -846, 423, 423)
STRIP_EDGES = [(STRIP_BELOW, 1, -1), (STRIP_BELOW_FOLD, 1, -1), (STRIP_ABOVE, 0, +1)]  # (set, the parameter one step moves, step)
SMALL_EDGE = (600, -400, 500, 10)  # span 65 000 at 100 x 100; gopen 501 is one past
STRIP_ROWS = 19                    # rows per strip the planner gives the 2.4 kb candidates


def _random_sets(seed, n):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        gext = int(rng.integers(0, 40))
        out.append((int(rng.integers(1, 400)), -int(rng.integers(1, 3000)), gext + int(rng.integers(0, 3000)), gext))
    return out


def random_edges(seed, n):
    """n random sets in the style of scripts/range_fuzz.py with a target length whose largest admitted query is 16 .. 300 long (the
    geometries every 16-bit short-read kernel takes): [(params, tl, ql)]"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        p = _random_sets(int(rng.integers(0, 1 << 30)), 1)[0]
        tl = int(rng.choice([64, 100, 150, 200, 256, 300]))
        ql = rg.dp16_largest_ql(tl, p)
        if 16 <= ql <= 300:
            out.append((p, tl, ql))
    return out


def test_worked_edges():
    for params, tl, ql in DP16_EDGES:
        assert rg.dp16_largest_ql(tl, params) == ql
        assert rg.dp16_range_ok(tl, ql, *params) and not rg.dp16_range_ok(tl, ql + 1, *params)
    assert rg.dp16_slack(300, 289, *GATK) == 40
    assert rg.strip16_window(*GATK) == (24567, 18051)           # 717 of slack below the 18 768 limit
    assert rg.param_edge(rg.strip16_range_ok, GATK, 1, -1, -4000) == STRIP_BELOW
    assert rg.param_edge(rg.strip16_range_ok, (44, -846, 423, 423), 0, +1, 4000) == STRIP_ABOVE
    assert rg.strip16_window(*STRIP_BELOW)[1] == rg.strip16_window(*STRIP_BELOW_FOLD)[1] == 32768 + rg.STRIP_LEVEL
    assert rg.strip16_window(*STRIP_ABOVE)[0] == 32767 - rg.STRIP_LEVEL
    for params, k, step in STRIP_EDGES:
        assert rg.strip16_range_ok(*params) and not rg.strip16_range_ok(*rg.past(params, k, step))
    assert rg.small_span(100, 100, *SMALL_EDGE) == 65000
    assert rg.small_fits_int16(100, 100, *SMALL_EDGE) and not rg.small_fits_int16(100, 100, *rg.past(SMALL_EDGE, 2, 1))


@pytest.mark.parametrize("params,tl,ql", DP16_EDGES + random_edges(5, 8), ids=str)
def test_dp16_mirror_pinned_to_the_planner(params, tl, ql):
    """At the largest admitted ql: the headline's lane kernel (checkpointed), the stored-flag lane kernel (score-only hint), the
    eight-pairs-per-wave kernel and the device sort of a mixed batch all run in 16 bits; one column more, every one of them is int32."""
    for q, fits in ((ql, rg.dp16_range_ok(tl, ql, *params)), (ql + 1, rg.dp16_range_ok(tl, ql + 1, *params))):
        shapes = [(10_000_000, UNIFORM, LANE16_CK), (10_000_000, UNIFORM | SCORE_ONLY, LANE16), (6000, UNIFORM, DP16)]
        for n, flags, kernel in shapes:
            p = _lib.explain(n=n, max_tl=tl, max_ql=q, parameters=params, flags=flags, workspace=WS)
            if fits:
                assert p.precision_bits == 16, (n, flags, q)
                if tl <= 300:   # (the worked 1200-row edge: its lane regions do not fit, the eight-pair kernel takes it)
                    assert p.fill_kernel == kernel, (n, flags, q, p.fill_kernel)
            else:
                assert p.precision_bits == 32 and p.fill_kernel not in (DP16, LANE16, LANE16_CK), (n, flags, q)
        if tl * q <= (1 << 20):
            p = _lib.explain(n=max(100_000, tl * q // 8 + 1), max_tl=tl, max_ql=q, parameters=params, workspace=WS)
            assert (p.sorted_by_library == 1 and p.precision_bits == 16) == fits, (q, p.sorted_by_library, p.precision_bits)


@pytest.mark.parametrize("params,k,step", STRIP_EDGES + [(GATK, 1, -1)], ids=str)
def test_strip16_mirror_pinned_to_the_planner(params, k, step):
    """Long reads take STRIP16 at the edge (one pass and several); one step past, the workgroup kernels -- COOP16 exactly where
    coop16_worthwhile says so, else COOP -- or the int32 wave-per-pair kernel where that fits."""
    edge = rg.param_edge(rg.strip16_range_ok, params, k, step, 4000 * step)
    if params != GATK:
        assert edge == params
    beyond = rg.past(edge, k, step)
    assert not rg.strip16_range_ok(*beyond)
    for n, tl, ql in ((8, 3000, 3000), (2, 20000, 3000)):
        p = _lib.explain(n=n, max_tl=tl, max_ql=ql, parameters=edge, workspace=WS)
        assert p.fill_kernel == STRIP16 and p.precision_bits == 16, (tl, p.fill_kernel)
        q = _lib.explain(n=n, max_tl=tl, max_ql=ql, parameters=beyond, workspace=WS)
        assert q.fill_kernel != STRIP16
    q = _lib.explain(n=4, max_tl=12000, max_ql=12000, parameters=beyond, workspace=WS)
    assert q.fill_kernel == (COOP16 if rg.coop16_worthwhile(*beyond) else COOP), (beyond, q.fill_kernel)
    assert rg.coop16_possible(*beyond)


def test_strip16_mirror_on_random_sets():
    rng = np.random.default_rng(17)
    seen = {True: 0, False: 0}
    for _ in range(40):
        gext = int(rng.integers(0, 40))
        p = (int(rng.integers(1, 400)), -int(rng.integers(0, 1500)), gext + int(rng.integers(0, 600)), gext)
        ok = rg.strip16_range_ok(*p)
        seen[ok] += 1
        assert (_lib.explain(n=8, max_tl=3000, max_ql=3000, parameters=p, workspace=WS).fill_kernel == STRIP16) == ok, p
    assert min(seen.values()) >= 3, seen


def test_coop16_mirrors_pinned_to_the_planner():
    """Sets past the strip guard, long queries: COOP16 where coop16_worthwhile holds, COOP where it does not; both edges of
    coop16_worthwhile's inequality (match walked up) and coop16_possible's (gopen walked up)."""
    base = (40, -3000, 600, 5)
    assert not rg.strip16_range_ok(*base) and rg.coop16_worthwhile(*base)
    edge_w = rg.param_edge(rg.coop16_worthwhile, base, 0, +1, 4000)
    edge_p = rg.param_edge(rg.coop16_possible, (40, -3000, 600, 600), 2, +1, 4000)
    assert rg.coop16_possible(*rg.past(edge_w, 0, 1)) and not rg.coop16_possible(*rg.past(edge_p, 2, 1))
    for p in (edge_w, rg.past(edge_w, 0, 1), edge_p, rg.past(edge_p, 2, 1)):
        q = _lib.explain(n=4, max_tl=12000, max_ql=12000, parameters=p, workspace=WS)
        assert q.fill_kernel == (COOP16 if rg.coop16_worthwhile(*p) else COOP), (p, q.fill_kernel)


def test_small_kernel_at_its_span():
    """Both sides of small_fits_int16's span take sw_small_kernel (narrow or wide is not visible from outside)."""
    for p in (SMALL_EDGE, rg.past(SMALL_EDGE, 2, 1)):
        assert _lib.explain(n=8, max_tl=100, max_ql=100, parameters=p).fill_kernel == SMALL


# ---- the reference recurrence

@pytest.mark.parametrize("strategy", ol.STRATEGIES)
def test_reference_dp_against_the_restatement(strategy):
    rng = np.random.default_rng(strategy)
    alpha = np.frombuffer(b"ACGT", np.uint8)
    cases = [(b"A" * 40, b"A" * 33), (b"A" * 30, b"C" * 50), (b"ACGT" * 20, b"AC" * 17), (b"G", b"G"), (b"G", b"T")]
    cases += [(alpha[rng.integers(0, 4, int(rng.integers(1, 90)))].tobytes(), alpha[rng.integers(0, 4, int(rng.integers(1, 90)))].tobytes()) for _ in range(12)]
    for params in (GATK, STRIP_BELOW, STRIP_ABOVE, (1, -4, 6, 1), (5, 0, 3, 3)):
        for t, q in cases:
            H, E, F = rg.dp_full(t, q, params, strategy)
            o = ol.oracle_align(t, q, params, strategy)
            assert int(H[-1, -1]) == o["h_end"] and rg.score_max(H) == o["score"], (params, t, q)
            # E and F are what they claim: H never falls below either, and each is one of its two sources
            assert (H[1:, 1:] >= E[1:, 1:]).all() and (H[1:, 1:] >= F[1:, 1:]).all()
            assert (E[2:, 1:] == np.maximum(H[1:-1, 1:] - params[2], E[1:-1, 1:] - params[3])).all()
            assert (F[1:, 2:] == np.maximum(H[1:, 1:-1] - params[2], F[1:, 1:-1] - params[3])).all()


# ---- the strip kernel's static window, evaluated

STRIP_SETS = [GATK, STRIP_BELOW, STRIP_BELOW_FOLD, STRIP_ABOVE]


@pytest.mark.parametrize("params", STRIP_SETS, ids=str)
def test_strip_window_holds_on_adversarial_inputs(params):
    """Every candidate, SOFTCLIP and INDEL borders: the rise and the fall in the strips of the planner's row count stay inside
    what strip16_range_ok grants (and so inside 16 bits at STRIP_LEVEL)."""
    assert _lib.explain(n=8, max_tl=2400, max_ql=2400, parameters=params, workspace=WS).rows == STRIP_ROWS
    above, below = rg.strip16_window(*params)
    worst = [0.0, 0.0]
    for name, (t, q) in rg.strip_candidates().items():
        for strategy in (ol.SOFTCLIP, ol.INDEL):
            H, E, F = rg.dp_full(t, q, params, strategy)
            fa, fb, a, b = rg.strip_fraction(H, E, F, params, STRIP_ROWS)
            assert a <= above and b <= below, (name, strategy, a, b)
            assert rg.STRIP_LEVEL + a <= 32767 and rg.STRIP_LEVEL - b >= -32768
            worst = [max(worst[0], fa), max(worst[1], fb)]
    print(f"{params}: largest fraction of the window reached: above {worst[0]:.3f}, below {worst[1]:.3f}")


# (set, side) -> (the candidate the GPU test runs, the least fraction of that side it must reach).  Measured in strips of 19 rows: a
# 40-base insertion into an otherwise identical target reaches 0.182 of `above` under the `below` edge without a fold, 0.079 with
# one and 0.362 under the `above` edge; unrelated sequences 0.050 / 0.095 of `below`, identical ones 0.033 with the fold.
STRIP_PICKS = {
    (STRIP_BELOW, "above"): ("insertion40", 0.18), (STRIP_BELOW, "below"): ("unrelated", 0.049),
    (STRIP_BELOW_FOLD, "above"): ("insertion40", 0.078), (STRIP_BELOW_FOLD, "below"): ("identical", 0.033),
    (STRIP_ABOVE, "above"): ("insertion40", 0.36), (STRIP_ABOVE, "below"): ("unrelated", 0.094),
}


@pytest.mark.parametrize("params", [STRIP_BELOW, STRIP_BELOW_FOLD, STRIP_ABOVE], ids=str)
def test_strip_inputs_picked_by_measured_spread(params):
    """The GPU test's strip inputs reach the most of each side of the window that any candidate reaches, and at least the pinned
    fraction: they cannot drift into easy cases."""
    (na, fa), (nb, fb) = rg.pick_strip_inputs(params, ol.SOFTCLIP, STRIP_ROWS)
    pool = rg.strip_candidates()
    for side, best in ((0, fa), (1, fb)):
        name, least = STRIP_PICKS[(params, ("above", "below")[side])]
        got = rg.strip_fraction(*rg.dp_full(*pool[name], params, ol.SOFTCLIP), params, STRIP_ROWS)[side]
        print(f"{params} {('above', 'below')[side]}: {name} reaches {got:.3f} of the window (best candidate {best:.3f})")
        assert got >= least and got >= best - 1e-9, (name, side, got, na, nb)
