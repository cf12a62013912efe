"""The folded diagonal on the GPU (sw_device.h: diag_fold; sw_lane_cell.h: CMP_FOLD): the checkpointed lane kernel and the long-read strip
kernel bit-exact against the CPU restatement and the goldens, for parameter sets that fold and sets that do not, and the folded kernels
identical byte for byte to the unfolded ones (MGL_SW_DEBUG_DIAG_FOLD=0) on a million pairs of the headline workload."""
import numpy as np
import pytest

import golden_io
import oracle_lib as ol
from mgl_amd import _lib, smithwaterman as sw

pytestmark = pytest.mark.gpu

GATK = (200, -150, 260, 11)
FOLDING = [GATK, (3, -1, 4, 3), (1, -3, 5, 2)]
NOT_FOLDING = [(25, -50, 110, 6), (1, -4, 6, 1)]
LANE16_CK, STRIP16 = 7, 6


def _fold_of(params, strip=False):
    """K as the planner reports it for the headline's shape (lane kernel) or a long-read batch (strip kernel)"""
    if strip:
        return _lib.explain(n=2304, max_tl=4608, max_ql=4608, parameters=params, workspace=208 << 30).diag_fold
    return _lib.explain(n=10_000_000, max_tl=256, max_ql=150, parameters=params, flags=_lib.FLAG_UNIFORM_GEOMETRY, workspace=208 << 30).diag_fold


@pytest.fixture(scope="module")
def lane():
    a = sw.MicrosoftSmithWaterman(0)
    a.set_small_kernel(1)
    a.set_lane_kernel(2)
    yield a
    a.close()


@pytest.fixture(scope="module")
def strip():
    a = sw.MicrosoftSmithWaterman(0)
    a.set_small_kernel(1)
    a.set_strip_kernel(2)
    yield a
    a.close()


def _mutate(rng, t, ql, gap_heavy):
    """A read of ql bases out of t with substitutions and (gap_heavy) indels of up to 12 bases."""
    alpha = np.frombuffer(b"ACGT", np.uint8)
    src = np.frombuffer(t, np.uint8)
    out, i = [], int(rng.integers(0, max(1, len(src) - ql)))
    while len(out) < ql:
        r = rng.random()
        if gap_heavy and r < 0.03:
            i += int(rng.integers(1, 13))                                 # deletion
        elif gap_heavy and r < 0.06:
            out.extend(alpha[rng.integers(0, 4, int(rng.integers(1, 13)))])  # insertion
        else:
            out.append(src[i % len(src)] if rng.random() > 0.02 else alpha[rng.integers(0, 4)])
            i += 1
    return bytes(np.array(out[:ql], np.uint8))


def _lane_batch(tl, ql, seed):
    """Three waves of 128 pairs: gap-heavy reads whose queries hold N and lower-case letters (base codes: the query may hold anything);
    a wave with an N in one target (that whole wave takes the byte compare); unrelated pairs."""
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(b"ACGT", np.uint8)
    ts, qs = [], []
    for k in range(384):
        t = alpha[rng.integers(0, 4, tl)].tobytes()
        if k >= 256:
            q = alpha[rng.integers(0, 4, ql)].tobytes()
        else:
            q = bytearray(_mutate(rng, t, ql, gap_heavy=True))
            if k % 3 == 0:
                q[int(rng.integers(0, ql))] = ord("N")
            if k % 5 == 0:
                x = int(rng.integers(0, ql - 4))
                q[x:x + 4] = bytes(q[x:x + 4]).lower()
            q = bytes(q)
        if k == 200:
            t = t[:17] + b"N" + t[18:]
        ts.append(t)
        qs.append(q)
    return ts, qs


def _check(res, ts, qs, params, strategy):
    off, sc, cg = ol.oracle_align_batch(ts, qs, params, strategy, nthreads=4)
    assert (res.offsets == off).all(), (params, strategy)
    assert (res.scores == sc).all(), (params, strategy)
    assert res.cigars == cg, (params, strategy)


@pytest.mark.parametrize("params", FOLDING + NOT_FOLDING, ids=str)
@pytest.mark.parametrize("tl,ql", [(256, 150), (300, 200)])
def test_lane_kernel_against_the_oracle(lane, params, tl, ql, monkeypatch):
    assert (_fold_of(params) != 0) == (params in FOLDING)
    ts, qs = _lane_batch(tl, ql, seed=tl * 31 + ql + params[0])
    for strategy in ol.STRATEGIES:
        res = lane.align_batch(ts, qs, params, strategy)
        assert lane.timing().fill_kernel == LANE16_CK
        _check(res, ts, qs, params, strategy)
        monkeypatch.setenv("MGL_SW_DEBUG_DIAG_FOLD", "0")
        un = lane.align_batch(ts, qs, params, strategy)
        monkeypatch.delenv("MGL_SW_DEBUG_DIAG_FOLD")
        assert (un.offsets == res.offsets).all() and (un.scores == res.scores).all() and un.cigars == res.cigars


@pytest.mark.parametrize("params", FOLDING + NOT_FOLDING, ids=str)
def test_lane_kernel_2bit_input(lane, params):
    from mgl_amd import device_batch as db

    ts, qs = _lane_batch(256, 150, seed=params[0] + 5)
    keep = [k for k in range(len(ts)) if b"N" not in ts[k] and b"N" not in qs[k] and qs[k].upper() == qs[k]]
    ts, qs = [ts[k] for k in keep], [qs[k] for k in keep]
    tb, qb = db.pack2bit(b"".join(ts)), db.pack2bit(b"".join(qs))
    t_start = np.arange(len(ts), dtype=np.int64) * 256
    q_start = np.arange(len(qs), dtype=np.int64) * 150
    for strategy in (ol.SOFTCLIP, ol.INDEL):
        res = lane.align_packed_2bit(tb, 256 * len(ts), t_start, None, qb, 150 * len(qs), q_start, None, 256, 150, params, strategy)
        assert lane.timing().fill_kernel == LANE16_CK
        off, sc, cg = ol.oracle_align_batch(ts, qs, params, strategy, nthreads=4)
        assert (res.offsets == off).all() and (res.scores == sc).all() and list(res.cigars) == cg, (params, strategy)


def test_lane_kernel_goldens(lane):
    rows = [g for g in golden_io.load("config1") if g.params == GATK]
    assert rows and _fold_of(GATK) == 20138
    by = {}
    for g in rows:
        by.setdefault(g.strategy, []).append(g)
    for strategy, gs in by.items():
        res = lane.align_batch([g.t for g in gs], [g.q for g in gs], GATK, strategy)
        for k, g in enumerate(gs):
            assert int(res.offsets[k]) == g.offset and tuple(int(x) for x in res.scores[k]) == g.score
            if not g.cigar.startswith("sha1:"):
                assert res.cigars[k] == g.cigar


@pytest.mark.parametrize("params", FOLDING + NOT_FOLDING, ids=str)
def test_strip_kernel_long_pairs(strip, params, monkeypatch):
    from mgl_amd import synth

    rng = synth.rng_for(params[0] * 13 + 1)
    pairs = [tuple(x.tobytes() for x in synth.ont_pair(rng, n)) for n in (2000, 3100, 4097, 5000)]
    g = bytearray(synth.random_genome(rng, 3000).tobytes())
    qn = bytearray(g[100:2600])
    for x in (5, 700, 701, 2499):
        qn[x] = ord("N")
    tn = bytearray(g)
    tn[800] = ord("N")
    pairs += [(bytes(g), bytes(qn)), (bytes(tn), bytes(g[100:2600])), (bytes(g), bytes(g[50:2000]).lower()),
              (bytes(g[:1200]) + bytes(g[1700:]), bytes(g[100:2900]))]
    ts, qs = [p[0] for p in pairs], [p[1] for p in pairs]
    folds = _fold_of(params, strip=True) != 0
    assert folds == (params in FOLDING)
    for strategy in (ol.SOFTCLIP, ol.INDEL, ol.IGNORE):
        res = strip.align_batch(ts, qs, params, strategy, cigar_stride=16384)
        assert strip.timing().fill_kernel == STRIP16, params
        for k, (t, q) in enumerate(pairs):
            o = ol.oracle_align(t, q, params, strategy)
            assert (int(res.offsets[k]), res.cigars[k], tuple(int(x) for x in res.scores[k])) == (o["offset"], o["cigar"], o["score"]), (params, strategy, k)
        if folds:
            monkeypatch.setenv("MGL_SW_DEBUG_DIAG_FOLD", "0")
            un = strip.align_batch(ts, qs, params, strategy, cigar_stride=16384)
            monkeypatch.delenv("MGL_SW_DEBUG_DIAG_FOLD")
            assert (un.offsets == res.offsets).all() and (un.scores == res.scores).all() and un.cigars == res.cigars


def test_strip_kernel_long_goldens(strip):
    gs = [g for g in golden_io.load("long") + golden_io.load("long2") if g.params == GATK]
    assert gs
    by = {}
    for g in gs:
        by.setdefault(g.strategy, []).append(g)
    for strategy, rows in by.items():
        res = strip.align_batch([g.t for g in rows], [g.q for g in rows], GATK, strategy, cigar_stride=2 * max(len(g.t) + len(g.q) for g in rows) + 16)
        assert strip.timing().fill_kernel == STRIP16
        for k, g in enumerate(rows):
            assert int(res.offsets[k]) == g.offset and tuple(int(x) for x in res.scores[k]) == g.score
            if g.cigar.startswith("sha1:"):
                import hashlib
                assert "sha1:" + hashlib.sha1(res.cigars[k].encode()).hexdigest() == g.cigar
            else:
                assert res.cigars[k] == g.cigar


def test_headline_folded_equals_unfolded_on_a_million_pairs(monkeypatch):
    import torch

    from mgl_amd import device_batch

    n = 1 << 20
    assert _fold_of(GATK) == 20138
    dev = torch.device("cuda", 0)
    b = device_batch.window_batch(42, n, dev)
    out = []
    with sw.MicrosoftSmithWaterman(0) as a:
        for off in (None, "0"):
            if off:
                monkeypatch.setenv("MGL_SW_DEBUG_DIAG_FOLD", off)
            b.run(a)
            torch.cuda.synchronize()
            assert a.timing().fill_kernel == LANE16_CK
            out.append([x.clone() for x in (b.offsets, b.scores, b.cigars, b.cigar_len, b.status)])
    for x, y in zip(*out):
        assert torch.equal(x, y)
    assert int((out[0][4] != 0).sum()) == 0
