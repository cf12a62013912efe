"""The 16-bit DNA kernels at the edges of their range guards (tests/range_guards.py mirrors them; tests/test_range_guards.py pins the
mirrors to the planner): every output bit-exact against the CPU restatement under every strategy, and the kernel that ran asserted --
at the largest geometry / parameter set a guard admits, with the sequences that drive the scores to the window's ends, and one step
past it, where the batch must leave the 16-bit kernel and stay exact."""
import numpy as np
import pytest

import oracle_lib as ol
import range_guards as rg
from mgl_amd import smithwaterman as sw

pytestmark = pytest.mark.gpu

GATK = (200, -150, 260, 11)
DP32, DP16, DP32_64, COOP, LANE16, COOP16, STRIP16, LANE16_CK, SMALL = range(9)
STRIP_BELOW, STRIP_BELOW_FOLD, STRIP_ABOVE = (200, -867, 260, 11), (50, -3900, 260, 2), (44, -846, 423, 423)
SMALL_EDGE = (600, -400, 500, 10)


def _check(res, ts, qs, params, strategy, what=""):
    off, sc, cg = ol.oracle_align_batch(ts, qs, params, strategy, nthreads=16)
    bad = [k for k in range(len(ts)) if int(res.offsets[k]) != off[k] or tuple(res.scores[k]) != tuple(sc[k]) or res.cigars[k] != cg[k]]
    assert not bad, (what, params, strategy, len(bad), bad[:8])


def _lane_pairs(tl, ql, seed, n=256):
    """Pairs 2k and 2k + 1 share a lane (sw_dp16_lane_ck.hip: slotA = 2 ls, slotB = 2 ls + 1): every lane holds an extreme-high pair
    (all-match homopolymer: exactly the top of the window) in its low half and an extreme-low one (all mismatch) in its high half,
    then periodic, random and gap-heavy pairs in the same alternation."""
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(b"ACGT", np.uint8)
    hi = [(b"A" * tl, b"A" * ql), (b"C" * tl, b"C" * ql), ((b"AC" * tl)[:tl], (b"AC" * ql)[:ql])]
    lo = [(b"A" * tl, b"C" * ql), (b"G" * tl, b"T" * ql), ((b"AC" * tl)[:tl], (b"GT" * ql)[:ql])]
    ts, qs = [], []
    for k in range(n // 2):
        if k < 64:
            a, b = hi[k % 3], lo[k % 3]
        else:
            t = alpha[rng.integers(0, 4, tl)].tobytes()
            src, out, i = np.frombuffer(t, np.uint8), [], 0
            while len(out) < ql:   # gap-heavy read out of t: the walk both verifies stretches and recomputes blocks
                r = rng.random()
                if r < 0.04:
                    i += int(rng.integers(1, 10))
                elif r < 0.08:
                    out.extend(alpha[rng.integers(0, 4, int(rng.integers(1, 10)))])
                else:
                    out.append(src[i % tl])
                    i += 1
            a = (t, bytes(np.array(out[:ql], np.uint8)))
            b = (t, alpha[rng.integers(0, 4, ql)].tobytes()) if k % 2 else (b"T" * tl, b"A" * ql)
        ts += [a[0], b[0]]
        qs += [a[1], b[1]]
    return ts, qs


def _edge_geometries():
    rng = np.random.default_rng(23)
    out = [(GATK, 300, 289), (GATK, 200, rg.dp16_largest_ql(200, GATK))]
    while len(out) < 5:
        gext = int(rng.integers(0, 40))
        p = (int(rng.integers(1, 400)), -int(rng.integers(1, 3000)), gext + int(rng.integers(0, 3000)), gext)
        tl = int(rng.choice([100, 150, 256, 300]))
        ql = rg.dp16_largest_ql(tl, p)
        if 32 <= ql <= 300:
            out.append((p, tl, ql))
    return out


EDGES = _edge_geometries()


@pytest.fixture(scope="module")
def lane():
    a = sw.MicrosoftSmithWaterman(0)
    a.set_small_kernel(1)
    a.set_lane_kernel(2)
    yield a
    a.close()


@pytest.mark.parametrize("params,tl,ql", EDGES, ids=str)
def test_lane_kernels_at_the_dp16_edge(lane, params, tl, ql, monkeypatch):
    """LANE16_CK folded and unfolded, LANE16 (flags stored), at the largest admitted ql and one past it (int32, still exact)."""
    assert rg.dp16_range_ok(tl, ql, *params) and not rg.dp16_range_ok(tl, ql + 1, *params)
    ts, qs = _lane_pairs(tl, ql, seed=tl + ql)
    for strategy in ol.STRATEGIES:
        res = lane.align_batch(ts, qs, params, strategy)
        assert lane.timing().fill_kernel == LANE16_CK and lane.timing().packed16 == 1
        _check(res, ts, qs, params, strategy, "lane_ck")
        monkeypatch.setenv("MGL_SW_DEBUG_DIAG_FOLD", "0")
        res = lane.align_batch(ts, qs, params, strategy)
        monkeypatch.delenv("MGL_SW_DEBUG_DIAG_FOLD")
        assert lane.timing().fill_kernel == LANE16_CK
        _check(res, ts, qs, params, strategy, "lane_ck unfolded")
    stored = sw.MicrosoftSmithWaterman(0)
    stored.set_small_kernel(1)
    stored.set_lane_kernel(2)
    stored.set_lane_checkpoint(1)
    for strategy in (ol.SOFTCLIP, ol.INDEL):
        res = stored.align_batch(ts, qs, params, strategy)
        assert stored.timing().fill_kernel == LANE16
        _check(res, ts, qs, params, strategy, "lane stored")
        assert stored.slot_layout(0) == stored.slot_layout(1)
    stored.close()
    ts1, qs1 = _lane_pairs(tl, ql + 1, seed=tl + ql + 1, n=128)
    for strategy in (ol.SOFTCLIP, ol.INDEL):
        res = lane.align_batch(ts1, qs1, params, strategy)
        assert lane.timing().packed16 == 0 and lane.timing().fill_kernel not in (DP16, LANE16, LANE16_CK)
        _check(res, ts1, qs1, params, strategy, "one past")


@pytest.mark.parametrize("params,tl,ql", EDGES[:3], ids=str)
def test_lane_kernel_2bit_inputs_at_the_dp16_edge(lane, params, tl, ql):
    """The same lanes from 2-bit packed inputs (one geometry promised: the checkpointed kernel stages base codes)."""
    from mgl_amd import device_batch as db

    ts, qs = _lane_pairs(tl, ql, seed=tl * 3 + ql)
    tb, qb = db.pack2bit(b"".join(ts)), db.pack2bit(b"".join(qs))
    t_start = np.arange(len(ts), dtype=np.int64) * tl
    q_start = np.arange(len(qs), dtype=np.int64) * ql
    for strategy in ol.STRATEGIES:
        res = lane.align_packed_2bit(tb, tl * len(ts), t_start, None, qb, ql * len(qs), q_start, None, tl, ql, params, strategy)
        assert lane.timing().fill_kernel == LANE16_CK
        off, sc, cg = ol.oracle_align_batch(ts, qs, params, strategy, nthreads=16)
        assert (res.offsets == off).all() and (res.scores == sc).all() and list(res.cigars) == cg, (params, strategy)


def test_sorted_mixed_batch_whose_largest_geometry_is_the_edge():
    """A device-resident batch of mixed geometries, sorted on the device (regroup), the largest at 300 x 289: whole waves through the
    checkpointed lane kernel, full blocks of eight through the packed kernel, the rest in int32."""
    import torch
    from mgl_amd import device_batch

    rng = np.random.default_rng(31)
    n = 12288   # (the device sort needs n * 8 >= max_tl * max_ql)
    geoms = [(300, 289), (300, 250), (256, 150), (120, 77)]
    ts, qs = [], []
    for k in range(n):
        tl, ql = geoms[(k // 128) % 4] if k < 9216 else (int(rng.integers(40, 301)), int(rng.integers(20, 290)))
        if k % 4 == 0:
            t, q = b"A" * tl, b"A" * ql
        elif k % 4 == 1:
            t, q = b"A" * tl, b"C" * ql
        else:
            t = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, tl)].tobytes()
            q = t[:ql] if k % 4 == 2 else np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, ql)].tobytes()
        ts.append(t)
        qs.append(q)
    assert max(len(t) for t in ts) == 300 and max(len(q) for q in qs) == 289
    td, toff = sw.concat(ts)
    qd, qoff = sw.concat(qs)
    b = device_batch.from_host(td, toff, qd, qoff, "cuda:0", cigar_stride=700)
    with sw.MicrosoftSmithWaterman(0) as a:
        for strategy in ol.STRATEGIES:
            b.run(a, GATK, strategy)
            torch.cuda.synchronize()
            assert a.timing().packed16 == 1 and int((b.status != 0).sum()) == 0
            off, sc, cg = ol.oracle_align_batch(ts, qs, GATK, strategy, nthreads=16)
            assert (b.offsets.cpu().numpy() == off).all() and (b.scores.cpu().numpy() == sc).all(), strategy
            assert b.cigar_strings() == cg, strategy


# ---- the long-read strip kernel at both edges of strip16_range_ok

# the inputs tests/test_range_guards.py picks by measured spread (STRIP_PICKS): the most of each side of the window any candidate reaches
STRIP_INPUTS = {STRIP_BELOW: ("insertion40", "unrelated"), STRIP_BELOW_FOLD: ("insertion40", "identical"), STRIP_ABOVE: ("insertion40", "unrelated")}
STRIP_PAST = {STRIP_BELOW: (1, -1), STRIP_BELOW_FOLD: (1, -1), STRIP_ABOVE: (0, +1)}


def _strip_pairs(params):
    pool = rg.strip_candidates()
    names = list(STRIP_INPUTS[params]) + ["homopolymer", "disjoint", "mismatch_blocks"]
    return [pool[x][0] for x in names], [pool[x][1] for x in names]


def _check_each(res, ts, qs, params, strategy, what):
    for k, (t, q) in enumerate(zip(ts, qs)):
        o = ol.oracle_align(t, q, params, strategy)
        assert (int(res.offsets[k]), res.cigars[k], tuple(int(x) for x in res.scores[k])) == (o["offset"], o["cigar"], o["score"]), (what, params, strategy, k)


@pytest.mark.parametrize("params", [STRIP_BELOW, STRIP_BELOW_FOLD, STRIP_ABOVE], ids=str)
def test_strip_kernel_at_the_strip16_edges(params, monkeypatch):
    assert rg.strip16_range_ok(*params)
    ts, qs = _strip_pairs(params)
    a = sw.MicrosoftSmithWaterman(0)
    a.set_strip_kernel(2)
    forms = [("ck", {}), ("ck unfolded", {"MGL_SW_DEBUG_DIAG_FOLD": "0"}), ("ck bytes", {"MGL_SW_DEBUG_STRIP_CODES": "0"})]
    for strategy in ol.STRATEGIES:
        for what, env in forms:
            if strategy not in (ol.SOFTCLIP, ol.INDEL) and env:
                continue
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            res = a.align_batch(ts, qs, params, strategy, cigar_stride=8192)
            for k in env:
                monkeypatch.delenv(k)
            assert a.timing().fill_kernel == STRIP16 and a.slot_layout(0) == 6, what
            _check_each(res, ts, qs, params, strategy, what)
    a.set_lane_checkpoint(1)   # flags stored (layout 4)
    for strategy in (ol.SOFTCLIP, ol.INDEL):
        res = a.align_batch(ts, qs, params, strategy, cigar_stride=8192)
        assert a.timing().fill_kernel == STRIP16 and a.slot_layout(0) == 4
        _check_each(res, ts, qs, params, strategy, "stored")
    a.set_lane_checkpoint(0)
    # one step past the edge: the batch leaves the strip kernel and stays exact
    beyond = rg.past(params, *STRIP_PAST[params])
    assert not rg.strip16_range_ok(*beyond)
    for strategy in (ol.SOFTCLIP, ol.INDEL):
        res = a.align_batch(ts, qs, beyond, strategy, cigar_stride=8192)
        assert a.timing().fill_kernel != STRIP16
        _check_each(res, ts, qs, beyond, strategy, "one past")
    a.close()


def test_strip_kernel_multi_pass_at_the_below_edge():
    """A target beyond 16 384 rows (two passes over the strips) under the `below` edge set, and one step past it."""
    rng = np.random.default_rng(41)
    alpha = np.frombuffer(b"ACGT", np.uint8)
    g = alpha[rng.integers(0, 4, 17000)].tobytes()
    ts, qs = [g, g, b"A" * 16500], [g[8000:9500], alpha[rng.integers(0, 4, 1500)].tobytes(), b"A" * 1200]
    a = sw.MicrosoftSmithWaterman(0)
    a.set_strip_kernel(2)
    for params, kernel_ok in ((STRIP_BELOW, True), (rg.past(STRIP_BELOW, 1, -1), False)):
        for strategy in (ol.SOFTCLIP, ol.INDEL):
            res = a.align_batch(ts, qs, params, strategy, cigar_stride=40000)
            assert (a.timing().fill_kernel == STRIP16) == kernel_ok, params
            _check_each(res, ts, qs, params, strategy, "multi-pass")
    a.close()


# ---- the small kernel and the one-pair service at small_fits_int16's span

@pytest.mark.parametrize("params", [SMALL_EDGE, rg.past(SMALL_EDGE, 2, 1)], ids=str)
def test_small_kernel_at_its_span(params):
    assert rg.small_fits_int16(100, 100, *params) == (params == SMALL_EDGE)
    ts = [b"A" * 100, b"A" * 100, (b"AC" * 50), b"G" * 100, b"A" * 100]
    qs = [b"A" * 100, b"C" * 100, (b"CA" * 50), b"T" * 100, b"A" * 57]
    a = sw.MicrosoftSmithWaterman(0)
    a.set_small_kernel(2)
    for strategy in ol.STRATEGIES:
        res = a.align_batch(ts, qs, params, strategy)
        assert a.timing().fill_kernel == SMALL
        _check(res, ts, qs, params, strategy, "small")
        for t, q in zip(ts[:2], qs[:2]):
            o = ol.oracle_align(t, q, params, strategy)
            assert sw.align(t, q, params, strategy)[:2] == (o["cigar"], o["offset"]), (params, strategy)
    a.close()


# ---- the cooperative 16-bit kernel at coop16_possible's edge

def test_coop16_at_its_possible_edge():
    """gopen walked up to the last set coop16_possible admits, precision 16 forced: whatever the kernel decides per pair (16 bits or
    its int32 body), the results are the oracle's; one step past, the int32 workgroup kernel."""
    edge = rg.param_edge(rg.coop16_possible, (40, -3000, 600, 600), 2, +1, 4000)
    beyond = rg.past(edge, 2, 1)
    pool = rg.strip_candidates(n=1500)
    ts, qs = [pool[x][0] for x in ("identical", "insertion40", "unrelated", "disjoint")], [pool[x][1] for x in ("identical", "insertion40", "unrelated", "disjoint")]
    a = sw.MicrosoftSmithWaterman(0)
    a.set_cooperative(7)
    a.set_precision(16)
    for params, kernel in ((edge, COOP16), (beyond, COOP)):
        for strategy in (ol.SOFTCLIP, ol.INDEL):
            res = a.align_batch(ts, qs, params, strategy, cigar_stride=8192)
            assert a.timing().fill_kernel == kernel, (params, a.timing().fill_kernel)
            _check_each(res, ts, qs, params, strategy, "coop")
    a.close()
