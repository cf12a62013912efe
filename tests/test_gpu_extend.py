"""mgl_sw_extend_batch_device on the GPU, bit-exact against the textbook (tests/extend_textbook.py) on every output -- the eight fields of
the record, CIGAR bytes, length, status -- with the band's edges, the strip seams, the Z-drop rule and both start cells placed where
the kernel has a decision to make."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import extend_textbook as et  # noqa: E402
import golden_io  # noqa: E402

pytestmark = pytest.mark.gpu

GATK = (200, -150, 260, 11)
PARAM_SETS = [GATK, (25, -50, 110, 6), (10, -15, 30, 5), (3, -1, 4, 3), (1, -1, 1, 1), (1, -4, 6, 1), (5, -4, 10, 1)]  # tests/test_gpu_banded.py's
KERNEL_EXTEND = 13
LENGTHS = (1, 63, 64, 65, 127, 128, 129, 1000)
DIFFS = (-130, -64, -1, 0, 1, 63, 64, 65, 300)


@pytest.fixture(scope="module")
def aligner():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mgl_amd import smithwaterman as sw

    a = sw.MicrosoftSmithWaterman(0)
    assert a.load()
    yield a
    a.close()


def _textbook(t, q, params, band, zdrop, to_qend):
    f = et.extend_align if len(t) * min(len(q), 2 * band + 1) <= 4000 else et.extend_align_np
    return f(t, q, *params, band, zdrop, to_qend)


def _check(aligner, ts, qs, band, zdrop, params=GATK, to_qend=False):
    """every output of a batch against the textbook; -> the textbook's results"""
    from mgl_amd import _lib

    res, st = aligner.extend(ts, qs, band, zdrop, params, to_qend, return_status=True)
    assert aligner.timing().fill_kernel == KERNEL_EXTEND == _lib.KERNEL_EXTEND
    want = [_textbook(t, q, params, band, zdrop, to_qend) for t, q in zip(ts, qs)]
    for k, (ext, cigar) in enumerate(want):
        got = et.Ext(*(int(res[c][k]) for c in range(8)))
        assert (int(st[k]), got, res.cigars[k], int(res.cigar_len[k])) == (0, ext, cigar, len(cigar)), (k, ts[k], qs[k], params, band, zdrop, to_qend)
    return want


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
def test_lengths_differences_and_bands(aligner, pk):
    """the band's edges crossing lane 0, lane 63, the carry row and the matrix's corner at every offset; Z-drop off, tight and loose"""
    rng = np.random.default_rng(200 + pk)
    params = PARAM_SETS[pk]
    ts, qs = [], []
    for tl in LENGTHS:
        for d in DIFFS:
            if tl - d >= 1:
                t, q = _pair(rng, tl, tl - d, b"AC" if (tl + d) % 3 == 0 else b"ACGT")
                ts.append(t)
                qs.append(q)
    assert len(ts) == 55
    o = abs(params[2])
    dropped = 0
    for n, band in enumerate((0, 1, 2, 31, 63, 64, 65, 200, 1300, 5000)):
        zdrop = (-1, 2 * o, 40 * o)[(n + pk) % 3]
        want = _check(aligner, ts, qs, band, zdrop, params, to_qend=bool((n + pk) & 1))
        dropped += sum(w[0].dropped for w in want)
    assert dropped > 20


def test_drops_in_the_first_strip_at_the_seam_in_the_last_row_and_never(aligner):
    """band 0: the path is the diagonal, a mismatch costs 150, and with zdrop 260 the second mismatched row drops"""
    rng = np.random.default_rng(5)
    a = np.frombuffer(b"ACGT", np.uint8)
    core = a[rng.integers(4, size=400)].tobytes()
    ts, qs, rows_done = [], [], []
    for p, tail in ((10, 200), (61, 200), (62, 200), (63, 200), (64, 200), (126, 100), (127, 100), (190, 2), (190, 3), (300, 0)):
        ts.append(core[:p] + b"A" * tail)
        qs.append(core[:p] + b"C" * tail)
        rows_done.append(p + 1 if tail >= 2 else p + tail)
    for to_qend in (False, True):
        want = _check(aligner, ts, qs, 0, 260, GATK, to_qend)
        assert [w[0].rows_done for w in want] == rows_done == [11, 62, 63, 64, 65, 127, 128, 191, 191, 300]
        assert [w[0].dropped for w in want] == [1] * 9 + [0]
        assert all(w[0].cigar_from == 0 for w in want[:9])  # column ql lies past rows_done: the request falls back to the best cell
        assert want[9][0].cigar_from == int(to_qend)
    # the same with room around the diagonal, and a drop that the band's edge brings about
    for band in (1, 10, 70):
        _check(aligner, ts, qs, band, 260)
        _check(aligner, ts, qs, band, 3000, to_qend=True)


def test_best_cell_in_strip_0_and_the_drop_two_strips_later(aligner):
    rng = np.random.default_rng(6)
    a = np.frombuffer(b"ACGT", np.uint8)
    core = a[rng.integers(4, size=30)].tobytes()
    t, q = core + b"A" * 300, core + b"C" * 300
    (ext, cigar), = _check(aligner, [t], [q], 0, 150 * 130)
    assert (ext.score, ext.t_end, ext.q_end, ext.rows_done, ext.dropped, cigar) == (6000, 30, 30, 160, 1, "30M")
    for band in (3, 64):
        (ext, _), = _check(aligner, [t], [q], band, 150 * 130)
        assert (ext.t_end, ext.q_end) == (30, 30) and ext.rows_done > 158
    # a long deletion the gap term keeps alive across two seams, then the match resumes
    tail = a[rng.integers(4, size=100)].tobytes()
    (ext, cigar), = _check(aligner, [core + b"N" * 150 + tail], [core + tail], 160, 260)
    assert (ext.dropped, cigar) == (0, "30M150D100M")


def test_best_cell_on_the_border_is_the_empty_extension(aligner):
    for to_qend in (False, True):
        want = _check(aligner, [b"AAAA", b"A" * 100, b"G"], [b"CCCC", b"C" * 70, b"T"], 8, -1, GATK, to_qend)
        assert all((w[0].score, w[0].t_end, w[0].q_end) == (0, 0, 0) for w in want)
        assert all((w[1] == "") != to_qend for w in want)


def test_homopolymers_and_two_letter_ties(aligner):
    ts = [b"A" * 150, b"A" * 150, b"AC" * 80, b"ACAC" * 40 + b"A" * 30, b"ACA", b"AC" * 40 + b"CA" * 40, b"A" * 64 + b"C" + b"A" * 64]
    qs = [b"A" * 150, b"A" * 97, b"CA" * 70, b"AC" * 70, b"AGA", b"AC" * 80, b"A" * 64 + b"G" + b"A" * 64]
    for params in (GATK, (1, -1, 1, 1), (3, -1, 4, 3)):
        for band in (0, 3, 9, 64, 200):
            for zdrop in (-1, 0, 2 * params[2]):
                for to_qend in (False, True):
                    want = _check(aligner, ts, qs, band, zdrop, params, to_qend)
        # the earliest of equal bests: rows 1 and 3 of ACA / AGA both reach `match` under (1, -1, 1, 1)
        if params == (1, -1, 1, 1):
            assert (want[4][0].score, want[4][0].t_end, want[4][0].q_end) == (1, 1, 1)


def test_to_query_end_with_the_last_column_out_of_band_or_past_rows_done(aligner):
    rng = np.random.default_rng(8)
    t, q = _pair(rng, 100, 160)
    for band, zdrop, cigar_from in ((10, -1, 0), (59, -1, 0), (60, -1, 1), (200, -1, 1)):  # (i, 160) is in the band from band = 60 on
        (ext, _), = _check(aligner, [t], [q], band, zdrop, GATK, True)
        assert ext.cigar_from == cigar_from and (ext.t_end_qend >= 1) == bool(cigar_from)
    t2, q2 = t + b"A" * 100, t + b"C" * 100
    (ext, _), = _check(aligner, [t2], [q2], 30, 500, GATK, True)
    assert ext.dropped == 1 and (ext.score_qend, ext.t_end_qend, ext.cigar_from) == (et.NO_QEND, -1, 0)


def test_statuses_canaries_chunks_score_only_and_binary(aligner):
    from mgl_amd import _lib
    from mgl_amd import smithwaterman as sw

    rng = np.random.default_rng(3)
    dev = torch.device("cuda", 0)
    pairs = [_pair(rng, int(rng.integers(1, 300)), int(rng.integers(1, 300))) for _ in range(90)]
    ts, qs = [p[0] for p in pairs], [p[1] for p in pairs]
    ts[5], qs[5] = _pair(rng, 14000, 6000)   # fits no slot of the small workspace below
    band, zdrop, stride, n = 20, 2000, 48, len(ts)
    want = [_textbook(t, q, GATK, band, zdrop, True) for t, q in zip(ts, qs)]
    g = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    tl, ql = np.array([len(t) for t in ts], np.int32), np.array([len(q) for q in qs], np.int32)
    toff, qoff = np.concatenate([[0], np.cumsum(tl)[:-1]]).astype(np.int64), np.concatenate([[0], np.cumsum(ql)[:-1]]).astype(np.int64)
    tl_bad, ql_bad = tl.copy(), ql.copy()
    tl_bad[7], ql_bad[9], tl_bad[11] = 0, 0, 301   # a length of 0 either side, a pair above max_tl
    td, qd = g(np.frombuffer(b"".join(ts) + b"\0" * 400, np.uint8).copy()), g(np.frombuffer(b"".join(qs) + b"\0" * 8, np.uint8).copy())

    def call(al, tlen, binary=False, score_only=False, stride=stride, max_tl=300, params=GATK):
        out = (torch.full((n + 1, 8), -77, dtype=torch.int32, device=dev), torch.full(((n + 1) * stride,), 0xEE, dtype=torch.uint8, device=dev),
               torch.full((n + 1,), -77, dtype=torch.int32, device=dev), torch.full((n + 1,), -77, dtype=torch.int32, device=dev))
        al.extend_device(td, g(toff), g(tlen), qd, g(qoff), g(ql_bad), max_tl, 6000, band, zdrop, params, True, stride, binary, score_only,
                         out=(out[0][:n], out[1], out[2], out[3]))
        torch.cuda.synchronize()
        assert al.timing().fill_kernel == KERNEL_EXTEND
        return [x.cpu().numpy() for x in out]

    # a context of its own with the smallest workspace there is, 1 MiB: one slot, so a grid smaller than the batch, and the
    # 14 000 x 6 000 pair (1.2 MB of decisions) does not fit it
    assert et.extend_pair_bytes(14000, 6000, band) > 1 << 20 > et.extend_pair_bytes(300, 300, band)
    small_ws = sw.MicrosoftSmithWaterman(0)
    tl_small = tl_bad.copy()
    tl_small[11] = tl[11]  # (max_tl = 14 000 admits pair 5; pair 11 keeps its own length here and is an ordinary pair)
    try:
        small_ws.set_workspace(1 << 20)
        ex, cg, ln, st = call(small_ws, tl_small, max_tl=14000)
    finally:
        small_ws.close()
    ex2, cg2, ln2, st2 = call(aligner, tl_bad)  # the default workspace; max_tl = 300: pairs 5 and 11 are above it
    overflows = 0
    for e_, c_, l_, t_, mode in ((ex, cg, ln, st, "small"), (ex2, cg2, ln2, st2, "default")):
        c_ = c_.reshape(n + 1, stride)
        assert l_[n] == -77 and t_[n] == -77 and (e_[n] == -77).all() and (c_[n] == 0xEE).all()  # nothing behind the arrays
        for k in range(n):
            w_ext, w_cigar = want[k]
            if k in (5, 7, 9) or (k == 11 and mode == "default"):
                assert t_[k] == (_lib.ERR_UNSUPPORTED if (k == 5 and mode == "small") else _lib.ERR_BAD_ARG), (k, mode, t_[k])
                assert l_[k] == 0 and (e_[k] == 0).all() and (c_[k] == 0xEE).all(), k
            elif len(w_cigar) > stride:
                assert (t_[k], l_[k]) == (_lib.ERR_CIGAR_OVERFLOW, 0) and (e_[k] == 0).all() and (c_[k] == 0xEE).all(), k
                overflows += 1
            else:
                assert (t_[k], l_[k]) == (0, len(w_cigar)) and tuple(e_[k]) == tuple(w_ext), (k, mode, t_[k], e_[k], want[k])
                assert c_[k, :l_[k]].tobytes().decode() == w_cigar and (c_[k, l_[k]:] == 0xEE).all(), k  # the canary behind every row
    assert overflows >= 3 and (st2[:n] == 0).sum() > 40
    # score-only: the eight fields of the full call (an overflow cannot happen), nothing else touched
    ex3, cg3, ln3, st3 = call(aligner, tl_bad, score_only=True)
    for k in range(n):
        if st2[k] in (0, _lib.ERR_CIGAR_OVERFLOW):
            assert st3[k] == 0 and tuple(ex3[k]) == tuple(want[k][0]), k
        else:
            assert st3[k] == st2[k] and (ex3[k] == 0).all()
    assert (cg3 == 0xEE).all() and (ln3[:n] == 0).all() and ln3[n] == -77
    # binary CIGAR: the text's elements
    ex4, cg4, ln4, st4 = call(aligner, tl_bad, binary=True, stride=4 * stride)
    cg4 = cg4.reshape(n + 1, 4 * stride)
    for k in range(n):
        if st4[k] == 0:
            assert et.cigar_binary_to_text(cg4[k, :ln4[k]].view("<u4")) == want[k][1] and tuple(ex4[k]) == tuple(want[k][0]), k
            assert (cg4[k, ln4[k]:] == 0xEE).all()
    assert (st4[:n] == 0).sum() > 60
    # outside the range guard (gopen above 2^24): every well-formed pair is unsupported
    ex5, cg5, ln5, st5 = call(aligner, tl_bad, params=(200, -150, (1 << 24) + 1, 11))
    assert all(st5[k] == (_lib.ERR_BAD_ARG if k in (5, 7, 9, 11) else _lib.ERR_UNSUPPORTED) for k in range(n)) and (ex5[:n] == 0).all() and (cg5 == 0xEE).all()


def test_a_10_kb_pair_at_band_512_with_and_without_a_junk_tail(aligner):
    recs = [g for g in golden_io.load("long") if len(g.t) >= 9000 and len(g.q) >= 9000]
    assert recs
    g = recs[0]
    rng = np.random.default_rng(12)
    for to_qend in (False, True):
        (ext, cigar), = _check(aligner, [g.t], [g.q], 512, 400 * 11, g.params, to_qend)
        assert ext.dropped == 0 and ext.t_end > 9000
    t = g.t + np.frombuffer(b"AC", np.uint8)[rng.integers(2, size=3000)].tobytes()
    q = g.q + np.frombuffer(b"GT", np.uint8)[rng.integers(2, size=3000)].tobytes()
    (ext, cigar), = _check(aligner, [t], [q], 512, 400 * 11, g.params)
    assert ext.dropped == 1 and len(g.t) - 64 <= ext.rows_done < len(t) - 2000 and ext.t_end <= len(g.t)
    _check(aligner, [t], [q], 512, -1, g.params, True)
