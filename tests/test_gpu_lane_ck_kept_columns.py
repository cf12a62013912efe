"""sw_dp16_lane_ck_kernel, pass 2: a walk whose diagonal stretch to the next kept row does not add up first checks the stretch
to the left edge of its block against the column checkpoints (PathWalk::edge_len / edge_apply) and only then has a block
recomputed.  The shapes here are the smallest at which that can go wrong: one indel at every read position, with the alignment's
diagonal shifted so that the edge cell falls on every row of a strip, ties, gaps at and across the edges themselves, every staging
path, geometries that change from wave to wave, and regions reused by launches with other borders.  Everything is compared with
the oracle: offsets, all six score fields, CIGAR strings.

What these tests can and cannot see.  A stretch taken where it must not be, or a border row left over from another launch, changes
a CIGAR or a score and fails here.  An edge check that never fires does NOT: with a wrong checkpoint index or a wrong base window
the sum would not fit, the walk would have its block recomputed as before, and the output would be the same.  That the path is
live shows only in the measurement build's counters (-DMGL_CK_PHASES, scripts/ck_phases.py: edge stretches taken and tried, block
rounds per wave; docs/history.md C.000a has the figures), which nothing asserts here.  That the sweeps exercise both branches
(stretches that add up and stretches that do not) rests on a CPU model of the walk, not on a count taken from the kernel."""
import numpy as np
import pytest

import oracle_lib as ol
from mgl_amd import smithwaterman as sw

pytestmark = pytest.mark.gpu

GATK = (200, -150, 260, 11)
OTHER = (25, -50, 110, 6)
LANE16_CK = 7
SHIFTS = tuple(range(0, 32, 3))


def _rand(rng, alpha, n):
    return alpha[rng.integers(0, len(alpha), n)]


def _read(rng, alpha, t, s, p, g, ql):
    """target[s:] with one indel at read position p -- g > 0: g extra bases in the read, g < 0: -g bases of the target missing --
    cut or padded to ql"""
    src = t[s:]
    r = np.concatenate([src[:p], _rand(rng, alpha, g), src[p:]]) if g > 0 else np.concatenate([src[:p], src[p - g:]])
    return np.concatenate([r, _rand(rng, alpha, ql)])[:ql]


def _sweep(tl, ql, seed, alphabet=b"ACGT", gaps=(1, -1, 3, -3), positions=None, shifts=SHIFTS):
    """One indel of every length in `gaps` at every read position, at every shift of the diagonal; an ODD number of pairs, so that
    a lane's two pairs stand in different places and the last lane holds one pair."""
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(alphabet, np.uint8)
    ts, qs = [], []
    for s in shifts:
        for p in (positions if positions is not None else range(2, ql - 1)):
            for g in gaps:
                t = _rand(rng, alpha, tl)
                ts.append(t.tobytes())
                qs.append(_read(rng, alpha, t, s, p, g, ql).tobytes())
    if len(ts) % 2 == 0:
        ts.pop()
        qs.pop()
    return ts, qs


@pytest.fixture()
def lane():
    a = sw.MicrosoftSmithWaterman(0)
    a.set_lane_kernel(2)
    yield a
    a.close()


_want = {}


def _oracle(key, ts, qs, params, strategy):
    """(one oracle run per batch, parameters and strategy, shared by the tests that align the same batch)"""
    k = (key, params, strategy)
    if k not in _want:
        _want[k] = ol.oracle_align_batch(ts, qs, params, strategy, nthreads=8)
    return _want[k]


def _check(res, want, what):
    off, sc, cg = want
    assert (np.asarray(res.offsets) == off).all(), what
    assert (np.asarray(res.scores) == sc).all(), what
    assert list(res.cigars) == list(cg), what


def _run(lane, key, ts, qs, params, strategy):
    res = lane.align_batch(ts, qs, params, strategy)
    assert lane.timing().fill_kernel == LANE16_CK, (key, params, strategy)
    _check(res, _oracle(key, ts, qs, params, strategy), (key, params, strategy))


@pytest.mark.parametrize("tl,ql", [(96, 70), (64, 33), (120, 97)])
def test_single_indel_sweep(lane, tl, ql):
    """Checkpoints at columns 32 / 64 / 96, a last block of one column at ql = 33, a partial last strip at tl = 120."""
    ts, qs = _sweep(tl, ql, seed=tl * 1000 + ql)
    assert len(ts) % 2 == 1 and len(ts) > 128
    for strategy in ol.STRATEGIES:
        _run(lane, ("sweep", tl, ql), ts, qs, GATK, strategy)
    _run(lane, ("sweep", tl, ql), ts, qs, OTHER, ol.SOFTCLIP)


def _run_sorted(a, key, ts, qs, params, strategy):
    """a batch of several geometries through a default context: the library sorts it and hands the geometries that fill whole waves
    to the checkpointed lane kernel, one geometry per wave"""
    res = a.align_batch(ts, qs, params, strategy, cigar_stride=256)
    assert a.timing().fill_kernel == LANE16_CK, "the geometries that fill whole waves should take the lane kernel"
    _check(res, _oracle(key, ts, qs, params, strategy), (key, params, strategy))


def test_single_indel_sweep_100x97(monkeypatch):
    """The sweep at 100 x 97: the last strip holds four rows.  A batch of this geometry alone gets 16-row strips (112 rows instead
    of 128) and with them the lane kernel that stores its flags, whatever set_lane_kernel says; as the bulk of a batch of TWO
    geometries it runs on the checkpointed kernel, whole waves of 100 x 97.  Only whole waves of 128 pairs go there: the last 39 of
    the 4 135 pairs run on the other kernels, and no lane of this kernel holds a single pair here (the odd count matters in the
    uniform sweeps above, at 120 x 97 among them, not in this one)."""
    monkeypatch.setenv("MGL_SW_DEBUG_LANE_GROUP_MIN", "128")
    ts, qs = _sweep(100, 97, seed=100 * 1000 + 97)
    t2, q2 = _sweep(100, 40, seed=1, positions=(5, 20), shifts=(0,))
    ts, qs = ts + t2[:-1], qs + q2[:-1]
    assert len(t2) < 8
    a = sw.MicrosoftSmithWaterman(0)
    try:
        for strategy in ol.STRATEGIES:
            _run_sorted(a, "100x97", ts, qs, GATK, strategy)
        _run_sorted(a, "100x97", ts, qs, OTHER, ol.SOFTCLIP)
    finally:
        a.close()


def _homopolymers(tl, ql, seed):
    """runs of 6 .. 12 equal bases laid across columns 32 and 64, the read's run one or two bases longer or shorter than the
    target's: the gap can sit anywhere in the run at the same score"""
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(b"AC", np.uint8)
    ts, qs = [], []
    for edge in (32, 64):
        for run in range(6, 13):
            for lead in range(0, run + 1, 2):  # bases of the read's run in front of the edge
                for d in (-2, -1, 1, 2):
                    for s in (0, 7, 16, 25):
                        a = edge - lead  # read position where the run starts
                        t = _rand(rng, alpha, tl)
                        base = alpha[int(rng.integers(0, 2))]
                        t[s + a: s + a + run] = base
                        src = t[s:]
                        r = np.concatenate([src[:a], np.full(run + d, base, np.uint8), src[a + run:], _rand(rng, alpha, ql)])[:ql]
                        ts.append(t.tobytes())
                        qs.append(r.tobytes())
    return ts, qs


@pytest.mark.parametrize("params", [(1, -1, 1, 1), (5, -4, 10, 1)], ids=str)
def test_ties(lane, params):
    """Two-letter sequences and cheap gaps: many cells where a gap ties with the diagonal.  A stretch that adds up may be taken
    only when the diagonal wins in every cell of it -- the sum fits exactly then, and the diagonal wins ties."""
    ts, qs = _sweep(96, 70, seed=77, alphabet=b"AC")
    ht, hq = _homopolymers(96, 70, seed=78)
    ts, qs = ts + ht, qs + hq
    if len(ts) % 2 == 0:
        ts, qs = ts[:-1], qs[:-1]
    for strategy in ol.STRATEGIES:
        _run(lane, "ties", ts, qs, params, strategy)


def test_gaps_at_the_edge(lane):
    """The gap cell in column 32 b - 1, 32 b or 32 b + 1, and horizontal runs of 2 .. 5 that span the edge, at every shift of the
    diagonal: every row of a strip as the edge cell's row."""
    near = [p for e in (32, 64) for p in range(e - 6, e + 3)]
    ts, qs = _sweep(96, 70, seed=5, gaps=(1, 2, 3, 4, 5, -1, -2, -5), positions=near, shifts=tuple(range(26)))
    for params in (GATK, OTHER, (5, -4, 10, 1)):
        for strategy in (ol.SOFTCLIP, ol.INDEL):
            _run(lane, "edge", ts, qs, params, strategy)


def test_other_staging_paths(lane):
    """The same sweep as 2-bit packed input, and as ASCII with an N in one target of every wave (that wave stages raw bytes)."""
    from mgl_amd import device_batch as db

    ts, qs = _sweep(96, 70, seed=96 * 1000 + 70)
    tb, qb = db.pack2bit(b"".join(ts)), db.pack2bit(b"".join(qs))
    t_start = np.arange(len(ts), dtype=np.int64) * 96
    q_start = np.arange(len(qs), dtype=np.int64) * 70
    res = lane.align_packed_2bit(tb, 96 * len(ts), t_start, None, qb, 70 * len(qs), q_start, None, 96, 70, GATK, ol.SOFTCLIP)
    assert lane.timing().fill_kernel == LANE16_CK
    _check(res, _oracle(("sweep", 96, 70), ts, qs, GATK, ol.SOFTCLIP), "2-bit")
    rng = np.random.default_rng(3)
    tn = list(ts)
    for k in range(5, len(tn), 128):
        t = bytearray(tn[k])
        t[int(rng.integers(0, 96))] = ord("N")
        tn[k] = bytes(t)
    _run(lane, "with N", tn, qs, GATK, ol.SOFTCLIP)


def test_grouped_geometry(monkeypatch):
    """One launch whose geometry -- and with it the number of blocks per row -- changes from wave to wave."""
    monkeypatch.setenv("MGL_SW_DEBUG_LANE_GROUP_MIN", "128")
    ts, qs = [], []
    for ql in (33, 64, 65, 97):
        t1, q1 = _sweep(100, ql, seed=ql, gaps=(1, -1, 3, -3), positions=range(2, ql - 1, 3))
        ts += t1
        qs += q1
    order = np.random.default_rng(11).permutation(len(ts))
    ts, qs = [ts[k] for k in order], [qs[k] for k in order]
    assert min(sum(len(q) == ql for q in qs) for ql in (33, 64, 65, 97)) >= 128
    a = sw.MicrosoftSmithWaterman(0)
    try:
        for strategy in (ol.SOFTCLIP, ol.INDEL):
            _run_sorted(a, "grouped", ts, qs, GATK, strategy)
    finally:
        a.close()


def test_regions_reused_by_launches_with_other_borders(lane, monkeypatch):
    """Two wave slots, so that every wave takes many tiles in its region, and three launches in a row on one context whose border
    rows differ: another geometry and gap cost, then another strategy."""
    monkeypatch.setenv("MGL_SW_DEBUG_LANE_SLOTS", "2")
    big, small = _sweep(96, 70, seed=96 * 1000 + 70), _sweep(64, 33, seed=64 * 1000 + 33)
    assert len(big[0]) >= 6 * 128 and len(small[0]) >= 6 * 128
    for _ in range(2):
        _run(lane, ("sweep", 96, 70), *big, GATK, ol.SOFTCLIP)
        _run(lane, ("sweep", 64, 33), *small, OTHER, ol.SOFTCLIP)
        _run(lane, ("sweep", 96, 70), *big, GATK, ol.INDEL)
