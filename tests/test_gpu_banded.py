"""mgl_sw_align_batch_device_banded on the GPU, bit-exact against the textbook (tests/banded_textbook.py) on every output -- offset, the
six score fields, CIGAR bytes, length, status -- and against the golden records through the two relations that tie the band to the
full-matrix function: R1 (a band that covers the matrix) and R2 (a band that holds the path)."""
import hashlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import banded_textbook as bt  # noqa: E402
import golden_io  # noqa: E402

pytestmark = pytest.mark.gpu

GATK = (200, -150, 260, 11)
PARAM_SETS = [GATK, (25, -50, 110, 6), (10, -15, 30, 5), (3, -1, 4, 3), (1, -1, 1, 1), (1, -4, 6, 1), (5, -4, 10, 1)]  # tests/golden/make_golden.py
STRATEGIES = (bt.SOFTCLIP, bt.INDEL, bt.LEADING_INDEL, bt.IGNORE)
BANDS = (0, 1, 2, 7, 31, 32, 33, 63, 64, 65, 200)
DIFFS = (-130, -64, -1, 0, 1, 63, 64, 65, 300)
SEAMS = (63, 64, 65, 127, 128, 129, 1000)


@pytest.fixture(scope="module")
def aligner():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mgl_amd import smithwaterman as sw

    a = sw.MicrosoftSmithWaterman(0)
    assert a.load()
    yield a
    a.close()


def _run(aligner, ts, qs, band, params, strategy, **kw):
    from mgl_amd import _lib

    res, st = aligner.align_banded(ts, qs, band, params, strategy, return_status=True, **kw)
    assert _lib.FILL_KERNEL_NAMES[aligner.timing().fill_kernel] == "sw_banded_kernel"
    return res, st


def _textbook(t, q, params, strategy, band):
    f = bt.banded_align if len(t) * min(len(q), 2 * band + abs(len(t) - len(q)) + 1) <= 4000 else bt.banded_align_np
    return f(t, q, *params, strategy, band)


def _check(aligner, ts, qs, band, params, strategy, want=None):
    """every output of a batch against the textbook (or against `want`: (offset, score or None, cigar) per pair)"""
    res, st = _run(aligner, ts, qs, band, params, strategy)
    for k, (t, q) in enumerate(zip(ts, qs)):
        off, ez, cigar = want[k] if want is not None else _textbook(t, q, params, strategy, band)
        got = (int(st[k]), int(res.offsets[k]), res.cigars[k], int(res.cigar_len[k]))
        assert got == (0, off, cigar, len(cigar)), (k, t, q, params, strategy, band, got, off, cigar)
        if ez is not None:
            assert tuple(int(x) for x in res.scores[k]) == tuple(ez), (k, t, q, params, strategy, band, res.scores[k], ez)
    return res


def _groups(records, key):
    out = {}
    for g in records:
        out.setdefault(key(g), []).append(g)
    return out


@pytest.mark.parametrize("suite", ["random", "ties", "shapes", "known"])
def test_r1_a_band_that_covers_the_matrix_gives_the_golden_records(aligner, suite):
    recs = golden_io.load(suite)
    assert {g.strategy for g in recs} >= set(STRATEGIES) or suite == "known"
    for (params, strategy), gs in _groups(recs, lambda g: (g.params, g.strategy)).items():
        band = max(max(len(g.t), len(g.q)) for g in gs)  # pairs of different geometry in one call
        _check(aligner, [g.t for g in gs], [g.q for g in gs], band, params, strategy, want=[(g.offset, g.score, g.cigar) for g in gs])


@pytest.mark.parametrize("suite", ["random", "ties", "shapes", "known"])
def test_r2_a_band_that_holds_the_golden_path_keeps_it_and_one_less_cuts_it(aligner, suite):
    recs = [g for g in golden_io.load(suite) if g.strategy != bt.IGNORE]
    held = cut = 0
    for (params, strategy, band), gs in _groups(recs, lambda g: (g.params, g.strategy, bt.path_band(g))).items():
        ts, qs = [g.t for g in gs], [g.q for g in gs]
        _check(aligner, ts, qs, band, params, strategy, want=[(g.offset, None, g.cigar) for g in gs])
        held += len(gs)
        if band > 0:
            res = _check(aligner, ts, qs, band - 1, params, strategy)
            for k, g in enumerate(gs):
                assert (int(res.offsets[k]), res.cigars[k]) != (g.offset, g.cigar), (g, band)
            cut += len(gs)
    assert held > 0 and (cut > 0 or suite == "known")


def _pair(rng, tl, ql, alphabet=b"ACGT"):
    """a target and a noisy copy of it cut or padded to ql"""
    a = np.frombuffer(alphabet, np.uint8)
    t = a[rng.integers(len(a), size=tl)]
    q = []
    for ch in t:
        r = rng.random()
        if r < 0.04:
            continue
        if r < 0.08:
            q.append(a[rng.integers(len(a))])
        q.append(a[rng.integers(len(a))] if rng.random() < 0.06 else ch)
    q = np.array(q[:ql] + list(a[rng.integers(len(a), size=max(0, ql - len(q)))]), np.uint8)
    return t.tobytes(), q.tobytes()


@pytest.mark.parametrize("pk", range(len(PARAM_SETS)))
def test_band_sweep_over_seams_and_length_differences(aligner, pk):
    """the band's edges crossing lane 0, lane 63 and the carry row at every offset"""
    rng = np.random.default_rng(100 + pk)
    params = PARAM_SETS[pk]
    ts, qs = [], []
    for tl in SEAMS:
        for d in DIFFS:
            if tl - d >= 1:
                t, q = _pair(rng, tl, tl - d, b"AC" if (tl + d) % 3 == 0 else b"ACGT")
                ts.append(t)
                qs.append(q)
    assert len(ts) == 51  # 7 x 9 less the twelve geometries without a query: d = 300 at tl <= 129, d >= tl at 63, 64, 65
    for band in BANDS:
        _check(aligner, ts, qs, band, params, STRATEGIES[(pk + band) % 4])


def test_adversarial_paths(aligner):
    rng = np.random.default_rng(7)
    a = np.frombuffer(b"ACGT", np.uint8)
    rnd = lambda n: a[rng.integers(4, size=n)].tobytes()  # noqa: E731
    ts, qs, bands = [], [], []
    for k in (1, 5, 40, 70):
        core, ins, gone = rnd(300), rnd(k), rnd(k)
        # k query bases inserted early and k target bases skipped late: the path runs along the upper edge of band k; and mirrored
        ts += [core[:20] + core[20:200] + gone + core[200:], core[:20] + gone + core[20:200] + core[200:]]
        qs += [core[:20] + ins + core[20:200] + core[200:], core[:20] + core[20:200] + ins + core[200:]]
        bands += [k, k]
        # a vertical run across the seam between rows 64 and 65 that ends on the band's edge
        ts.append(core[:64 - k // 2] + gone + core[64 - k // 2:])
        qs.append(core)
        bands.append(k)
    ts += [b"A" * 150, b"A" * 150, b"AC" * 80, b"ACAC" * 40 + b"A" * 30, rnd(200), rnd(200), rnd(50)]
    qs += [b"A" * 150, b"A" * 97, b"CA" * 70, b"AC" * 70, rnd(50), rnd(50), rnd(200)]  # homopolymer, two-letter ties, a band beyond the matrix's corner
    bands += [3, 9, 4, 6, 49, 51, 151]
    for strategy in STRATEGIES:
        for params in (GATK, (1, -1, 1, 1), (3, -1, 4, 3)):
            for band in sorted(set(bands)):
                pick = [k for k, b in enumerate(bands) if b == band]
                for delta in (0, -1, 1):
                    if band + delta >= 0:
                        _check(aligner, [ts[k] for k in pick], [qs[k] for k in pick], band + delta, params, strategy)


def test_long_pairs_at_band_512_and_at_the_band_of_their_path(aligner):
    recs = golden_io.load("long")
    assert any(g.cigar.startswith("sha1:") and len(g.t) >= 9000 and len(g.q) >= 9000 for g in recs)  # the 10 kb pair, its CIGAR pinned by SHA-1
    for g in recs:
        _check(aligner, [g.t], [g.q], 512, g.params, g.strategy, want=[bt.banded_align_np(g.t, g.q, *g.params, g.strategy, 512)])
        if g.strategy == bt.IGNORE:
            continue
        # R2: the full-matrix path (the textbook with a band that covers the matrix gives the golden record) and the band that holds it
        sha = lambda c: "sha1:" + hashlib.sha1(c.encode()).hexdigest() if g.cigar.startswith("sha1:") else c  # noqa: E731
        off, ez, cigar = bt.banded_align_np(g.t, g.q, *g.params, g.strategy, max(len(g.t), len(g.q)))
        assert (off, ez, sha(cigar)) == (g.offset, g.score, g.cigar)
        band = bt.path_band(g._replace(cigar=cigar))
        res, st = _run(aligner, [g.t], [g.q], band, g.params, g.strategy)
        assert (int(st[0]), int(res.offsets[0]), sha(res.cigars[0])) == (0, g.offset, g.cigar), band


def test_statuses_canaries_chunks_score_only_and_binary(aligner):
    from mgl_amd import _lib

    rng = np.random.default_rng(3)
    dev = torch.device("cuda", 0)
    pairs = [_pair(rng, int(rng.integers(1, 300)), int(rng.integers(1, 300))) for _ in range(90)]
    ts, qs = [p[0] for p in pairs], [p[1] for p in pairs]
    ts[5], qs[5] = _pair(rng, 2000, 1000)   # fits no slot of the small workspace below
    band, stride, n = 20, 48, len(ts)
    want = [_textbook(t, q, GATK, bt.SOFTCLIP, band) for t, q in zip(ts, qs)]
    g = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    tl, ql = np.array([len(t) for t in ts], np.int32), np.array([len(q) for q in qs], np.int32)
    toff, qoff = np.concatenate([[0], np.cumsum(tl)[:-1]]).astype(np.int64), np.concatenate([[0], np.cumsum(ql)[:-1]]).astype(np.int64)
    tl_bad, ql_bad = tl.copy(), ql.copy()
    tl_bad[7], ql_bad[9], tl_bad[11] = 0, 0, 301   # a length of 0 either side, a pair above max_tl
    td, qd = g(np.frombuffer(b"".join(ts) + b"\0" * 400, np.uint8).copy()), g(np.frombuffer(b"".join(qs) + b"\0" * 8, np.uint8).copy())

    def call(al, tlen, flags_binary=False, score_only=False, stride=stride, max_tl=300):
        out = (torch.full((n + 1,), -77, dtype=torch.int32, device=dev), torch.full((n + 1, 6), -77, dtype=torch.int32, device=dev),
               torch.full(((n + 1) * stride,), 0xEE, dtype=torch.uint8, device=dev), torch.full((n + 1,), -77, dtype=torch.int32, device=dev),
               torch.full((n + 1,), -77, dtype=torch.int32, device=dev))
        al.align_banded_device(td, g(toff), g(tlen), qd, g(qoff), g(ql_bad), max_tl, 2000, band, GATK, bt.SOFTCLIP, stride, flags_binary,
                                    score_only, out=out)
        torch.cuda.synchronize()
        return [x.cpu().numpy() for x in out]

    # a context of its own with the smallest workspace there is: one slot, a grid smaller than the batch, and the 2 000 x 1 000 pair
    # (1.09 MB of decisions) does not fit it
    from mgl_amd import smithwaterman as sw

    small_ws = sw.MicrosoftSmithWaterman(0)
    tl_small = tl_bad.copy()
    tl_small[11] = tl[11]  # (max_tl = 2000 admits pair 5; pair 11 keeps its own length here and is an ordinary pair)
    try:
        small_ws.set_workspace(1 << 20)
        off, sc, cg, ln, st = call(small_ws, tl_small, max_tl=2000)
    finally:
        small_ws.close()
    off2, sc2, cg2, ln2, st2 = call(aligner, tl_bad)  # the default workspace; max_tl = 300: pairs 5 and 11 are above it
    cg, cg2 = cg.reshape(n + 1, stride), cg2.reshape(n + 1, stride)
    for o_, s_, c_, l_, t_, small in ((off, sc, cg, ln, st, True), (off2, sc2, cg2, ln2, st2, False)):
        assert o_[n] == -77 and l_[n] == -77 and t_[n] == -77 and (s_[n] == -77).all() and (c_[n] == 0xEE).all()  # nothing behind the arrays
        for k in range(n):
            w_off, w_ez, w_cigar = want[k]
            if k in (5, 7, 9) or (k == 11 and not small):
                assert t_[k] == (_lib.ERR_UNSUPPORTED if (k == 5 and small) else _lib.ERR_BAD_ARG), (k, t_[k])
                assert o_[k] == 0 and l_[k] == 0 and (s_[k] == 0).all() and (c_[k] == 0xEE).all(), k
            elif len(w_cigar) > stride:
                assert (t_[k], o_[k], l_[k]) == (_lib.ERR_CIGAR_OVERFLOW, 0, len(w_cigar)) and tuple(s_[k]) == w_ez and (c_[k] == 0xEE).all(), k
            else:
                assert (t_[k], o_[k], l_[k]) == (0, w_off, len(w_cigar)) and tuple(s_[k]) == w_ez, (k, t_[k], o_[k], l_[k], want[k])
                assert c_[k, :l_[k]].tobytes().decode() == w_cigar and (c_[k, l_[k]:] == 0xEE).all(), k  # the canary behind every row
    assert any(len(w[2]) > stride for k, w in enumerate(want) if k not in (5, 7, 9, 11))  # (an overflow was among them)
    # score-only: the six fields of the full call, nothing else touched
    off3, sc3, cg3, ln3, st3 = call(aligner, tl_bad, score_only=True)
    ok = st2[:n] != _lib.ERR_BAD_ARG
    assert (sc3[:n][ok] == sc2[:n][ok]).all() and (cg3 == 0xEE).all() and (st3[:n][ok] == 0).all()
    # binary CIGAR: the text's elements
    off4, sc4, cg4, ln4, st4 = call(aligner, tl_bad, flags_binary=True, stride=4 * stride)
    cg4 = cg4.reshape(n + 1, 4 * stride)
    for k in range(n):
        if st4[k] == 0:
            assert bt.cigar_binary_to_text(cg4[k, :ln4[k]].view("<u4")) == want[k][2] and off4[k] == want[k][0], k
            assert (cg4[k, ln4[k]:] == 0xEE).all()
    assert (st4[:n] == 0).sum() > 60
