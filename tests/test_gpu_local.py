"""mgl_sw_local_batch_device_matrix on the GPU, bit-exact against the textbook DP (tests/local_textbook.py) on all five hit fields and
the CIGAR: kernel B (any pairs, full output), kernel A (score pass over shared-target tiles), the planner between them, a DNA case and
LocalSearch's top-k."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import local_textbook as lt  # noqa: E402

pytestmark = pytest.mark.gpu

PROT = b"ARNDCQEGHILKMFPSTWYV"
PROTA = np.frombuffer(PROT, np.uint8)


@pytest.fixture(scope="module")
def aligner():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mgl_amd import smithwaterman as sw

    a = sw.MicrosoftSmithWaterman(0)
    assert a.load()
    yield a
    a.close()


def _mutate(rng, s, rate=0.15, indel=0.05):
    out = bytearray()
    for ch in s:
        r = rng.random()
        if r < indel:
            continue
        if r < 2 * indel:
            out += bytes([PROT[rng.integers(len(PROT))]])
        out.append(PROT[rng.integers(len(PROT))] if rng.random() < rate else ch)
    return bytes(out)


def _batch(ts, qs, cigar_stride=512, max_tl=None, max_ql=None):
    from mgl_amd import protein

    dev = torch.device("cuda", 0)
    tb = b"".join(ts) + b"\0" * 8
    qb = b"".join(qs) + b"\0" * 8
    toff = np.concatenate([[0], np.cumsum([len(t) for t in ts])])[:-1].astype(np.int64)
    qoff = np.concatenate([[0], np.cumsum([len(q) for q in qs])])[:-1].astype(np.int64)
    g = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    return protein.LocalBatch(g(np.frombuffer(tb, np.uint8).copy()), g(toff), g(np.array([len(t) for t in ts], np.int32)),
                              g(np.frombuffer(qb, np.uint8).copy()), g(qoff), g(np.array([len(q) for q in qs], np.int32)),
                              max_tl if max_tl is not None else max(len(t) for t in ts), max_ql if max_ql is not None else max(len(q) for q in qs),
                              cigar_stride)


def _kernel(aligner):
    from mgl_amd import _lib

    return _lib.FILL_KERNEL_NAMES[aligner.timing().fill_kernel]


def _check_full(b, ts, qs, code, mat, o, e, binary=False):
    torch.cuda.synchronize()
    hits, st = b.hits.cpu().numpy(), b.status.cpu().numpy()
    cig = b.cigar_strings(binary=binary)
    for k, (t, q) in enumerate(zip(ts, qs)):
        want = lt.local_align_np(t, q, code, mat, o, e)
        got_c = lt.cigar_binary_to_text(cig[k]) if binary else cig[k]
        assert st[k] == 0, (k, st[k])
        assert tuple(int(x) for x in hits[k]) == want[:5] and got_c == want[5], (k, t, q, o, e, hits[k], got_c, want)


def _ragged(rng, n):
    ts, qs = [], []
    for k in range(n):
        tl = int(rng.integers(0, 300)) if k % 11 else 0
        t = bytes(PROTA[rng.integers(len(PROT), size=tl)]) if tl else b""
        kind = k % 5
        if kind == 0 and tl > 20:
            q = _mutate(rng, t[int(rng.integers(0, tl // 3)):])
        elif kind == 1:
            q = bytes(PROTA[rng.integers(len(PROT), size=int(rng.integers(1, 250)))]).lower()  # lower case
        elif kind == 2:
            q = bytes(rng.integers(0, 256, size=int(rng.integers(1, 120)), dtype=np.uint8))  # junk bytes -> 'X'
        elif kind == 3:
            q = b"BZX*" * int(rng.integers(1, 20)) + (t[:40] if t else b"")  # ambiguity codes
        else:
            q = bytes(PROTA[rng.integers(len(PROT), size=int(rng.integers(0, 200)))])
        if k % 13 == 5:
            q = b""  # a hole
        ts.append(t)
        qs.append(q)
    return ts, qs


def test_kernel_b_ragged_protein(aligner):
    from mgl_amd import protein

    rng = np.random.default_rng(11)
    code, mat = protein.blosum62()
    ts, qs = _ragged(rng, 300)
    b = _batch(ts, qs)
    protein.run_local(b, aligner, code, mat, 11, 1)
    _check_full(b, ts, qs, code, mat, 11, 1)
    assert _kernel(aligner) == "sw_local_pair_kernel"


@pytest.mark.parametrize("o,e", [(11, 1), (10, 2), (5, 5), (9, 0), (0, 0)])
def test_kernel_b_asymmetric_matrix_and_gap_models(aligner, o, e):
    from mgl_amd import protein

    rng = np.random.default_rng(o * 31 + e)
    mat = rng.integers(-6, 8, size=(32, 32)).astype(np.int8)  # asymmetric, every code used
    code = (np.arange(256) % 32).astype(np.uint8)
    ts, qs = [], []
    for k in range(120):
        t = bytes(rng.integers(0, 256, size=int(rng.integers(1, 200)), dtype=np.uint8))
        q = t[int(rng.integers(0, max(1, len(t) // 2))):][::-1] if k % 3 == 0 else bytes(rng.integers(0, 256, size=int(rng.integers(1, 200)), dtype=np.uint8))
        ts.append(t)
        qs.append(q or b"A")
    b = _batch(ts, qs)
    protein.run_local(b, aligner, code, mat, o, e)
    _check_full(b, ts, qs, code, mat, o, e)


def test_kernel_b_binary_cigar_and_overflow(aligner):
    from mgl_amd import _lib, protein

    rng = np.random.default_rng(5)
    code, mat = protein.blosum62()
    ts = [bytes(PROTA[rng.integers(len(PROT), size=200)]) for _ in range(40)]
    qs = [_mutate(rng, t, 0.2, 0.08) for t in ts]
    b = _batch(ts, qs, cigar_stride=1024)
    protein.run_local(b, aligner, code, mat, 11, 1, binary_cigar=True)
    _check_full(b, ts, qs, code, mat, 11, 1, binary=True)
    # a stride too small for most of them: the status says so, cigar_len holds the size needed, the hit is complete
    b = _batch(ts, qs, cigar_stride=8)
    protein.run_local(b, aligner, code, mat, 11, 1)
    torch.cuda.synchronize()
    st, ln, hits = b.status.cpu().numpy(), b.cigar_len.cpu().numpy(), b.hits.cpu().numpy()
    n_over = 0
    for k, (t, q) in enumerate(zip(ts, qs)):
        want = lt.local_align_np(t, q, code, mat, 11, 1)
        assert tuple(int(x) for x in hits[k]) == want[:5]
        if len(want[5]) > 8:
            n_over += 1
            assert st[k] == _lib.ERR_CIGAR_OVERFLOW and ln[k] == len(want[5])
        else:
            assert st[k] == 0 and b.cigar_strings([k])[0] == want[5]
    assert n_over > 20


def _tiles(rng, n_tiles, last_short=0, tl_choices=(1, 7, 31, 32, 33, 63, 64, 65, 150, 257), ql_max=300, holes=True):
    """n_tiles tiles of 128 pairs (the last one `last_short` pairs when given) sharing their target, query lengths mixed in a tile."""
    ts_, qs = [], []
    targets = []
    for k in range(n_tiles):
        t = bytes(PROTA[rng.integers(len(PROT), size=int(tl_choices[k % len(tl_choices)]))])
        targets.append(t)
        cnt = last_short if (k == n_tiles - 1 and last_short) else 128
        for p in range(cnt):
            r = rng.random()
            if holes and r < 0.05:
                q = b""
            elif r < 0.4 and len(t) > 4:
                q = _mutate(rng, t[int(rng.integers(0, len(t) // 2)):])[: ql_max]
            else:
                q = bytes(PROTA[rng.integers(len(PROT), size=int(rng.integers(1, ql_max)))])
            ts_.append(k)
            qs.append(q)
    return targets, ts_, qs


def _tile_batch(targets, tix, qs, max_ql=None):
    from mgl_amd import protein

    dev = torch.device("cuda", 0)
    tb = b"".join(targets) + b"\0" * 8
    starts = np.concatenate([[0], np.cumsum([len(t) for t in targets])])[:-1].astype(np.int64)
    qb = b"".join(qs) + b"\0" * 8
    qoff = np.concatenate([[0], np.cumsum([len(q) for q in qs])])[:-1].astype(np.int64)
    g = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    tix = np.asarray(tix)
    return protein.LocalBatch(g(np.frombuffer(tb, np.uint8).copy()), g(starts[tix]), g(np.array([len(targets[k]) for k in tix], np.int32)),
                              g(np.frombuffer(qb, np.uint8).copy()), g(qoff), g(np.array([len(q) for q in qs], np.int32)),
                              max(len(t) for t in targets), max_ql or max(1, max(len(q) for q in qs)), 0)


def _check_scores(b, targets, tix, qs, code, mat, o, e):
    torch.cuda.synchronize()
    hits, st = b.hits.cpu().numpy(), b.status.cpu().numpy()
    for k, q in enumerate(qs):
        want = lt.local_align_np(targets[tix[k]], q, code, mat, o, e)[0]
        assert st[k] == 0 and hits[k, 0] == want and (hits[k, 1:] == 0).all(), (k, hits[k], want)


def test_kernel_a_mixed_lengths_holes_short_last_tile(aligner):
    from mgl_amd import protein

    rng = np.random.default_rng(21)
    code, mat = protein.blosum62()
    targets, tix, qs = _tiles(rng, 10, last_short=37)
    b = _tile_batch(targets, tix, qs)
    protein.run_local(b, aligner, code, mat, 11, 1, score_only=True, shared_target=True)
    torch.cuda.synchronize()
    assert _kernel(aligner) == "sw_local_lane_kernel"
    _check_scores(b, targets, tix, qs, code, mat, 11, 1)
    # the same pairs through kernel B (no shared-target promise): the same scores
    b2 = _tile_batch(targets, tix, qs)
    protein.run_local(b2, aligner, code, mat, 11, 1, score_only=True)
    torch.cuda.synchronize()
    assert _kernel(aligner) == "sw_local_pair_kernel"
    assert torch.equal(b.hits, b2.hits)


def test_kernel_a_asymmetric_matrix_and_gaps(aligner):
    from mgl_amd import protein

    rng = np.random.default_rng(22)
    mat = rng.integers(-5, 9, size=(32, 32)).astype(np.int8)
    code = (np.arange(256) % 32).astype(np.uint8)
    for o, e in [(10, 2), (5, 5), (9, 0), (0, 0)]:
        targets, tix, qs = _tiles(rng, 3, last_short=70, ql_max=120)
        targets = [bytes(rng.integers(0, 256, size=len(t), dtype=np.uint8)) for t in targets]
        b = _tile_batch(targets, tix, qs)
        protein.run_local(b, aligner, code, mat, o, e, score_only=True, shared_target=True)
        torch.cuda.synchronize()
        assert _kernel(aligner) == "sw_local_lane_kernel"
        _check_scores(b, targets, tix, qs, code, mat, o, e)


def test_kernel_a_few_wave_slots_twice(aligner, monkeypatch):
    """A grid of 3 wave slots over 9 tiles draws from the counter; a second launch on the same context finds it back at zero."""
    from mgl_amd import protein

    monkeypatch.setenv("MGL_SW_DEBUG_LANE_SLOTS", "3")
    rng = np.random.default_rng(23)
    code, mat = protein.blosum62()
    targets, tix, qs = _tiles(rng, 9, ql_max=90)
    for _ in range(2):
        b = _tile_batch(targets, tix, qs)
        protein.run_local(b, aligner, code, mat, 11, 1, score_only=True, shared_target=True)
        torch.cuda.synchronize()
        assert _kernel(aligner) == "sw_local_lane_kernel"
        _check_scores(b, targets, tix, qs, code, mat, 11, 1)
    aligner.check()  # the counter stood in range and is back at zero


def test_kernel_a_broken_promise(aligner):
    """A tile whose pairs do not share one target start, or one target length, gets BAD_ARG and nothing else; the other tiles are right."""
    from mgl_amd import _lib, protein

    rng = np.random.default_rng(24)
    code, mat = protein.blosum62()
    targets, tix, qs = _tiles(rng, 4, ql_max=100)
    b = _tile_batch(targets, tix, qs)
    t_off, t_len = b.t_off.clone(), b.t_len.clone()
    b.t_off[128 + 5] = t_off[128 + 5] + 1          # tile 1: another start
    b.t_len[256 + 77] = t_len[256 + 77] - 1        # tile 2: another length
    b.hits.fill_(-7)
    protein.run_local(b, aligner, code, mat, 11, 1, score_only=True, shared_target=True)
    torch.cuda.synchronize()
    assert _kernel(aligner) == "sw_local_lane_kernel"
    st, hits = b.status.cpu().numpy(), b.hits.cpu().numpy()
    assert (st[128:384] == _lib.ERR_BAD_ARG).all() and (hits[128:384] == -7).all()
    for k in list(range(0, 128)) + list(range(384, 512)):
        want = lt.local_align_np(targets[tix[k]], qs[k], code, mat, 11, 1)[0]
        assert st[k] == 0 and hits[k, 0] == want


def test_range_guard_picks_the_kernel(aligner):
    """Both sides of local_lane_ok()'s 16-bit edge: max(S) * min(tl, ql) + 255 <= 65535.  Targets and queries of 520 residues with
    max(S) = 120 run kernel A (62 655), with max(S) = 127 kernel B (66 295) -- the same scores either way."""
    from mgl_amd import protein

    rng = np.random.default_rng(25)
    code = (np.arange(256) % 32).astype(np.uint8)
    targets = [bytes(rng.integers(0, 256, size=520, dtype=np.uint8))]
    tix = [0] * 128
    qs = [targets[0][: 520 - 3 * k] if k % 4 == 0 else bytes(rng.integers(0, 256, size=int(rng.integers(400, 521)), dtype=np.uint8)) for k in range(128)]
    qs[1] = targets[0]
    for smax, kernel in [(120, "sw_local_lane_kernel"), (127, "sw_local_pair_kernel")]:
        mat = rng.integers(-8, 9, size=(32, 32)).astype(np.int8)
        mat[np.arange(32), np.arange(32)] = smax  # identity scores high: the full-length pair reaches 520 * smax
        assert lt.local_lane_ok(int(mat.min()), smax, 11, 1, 520, 520) == (kernel == "sw_local_lane_kernel")
        b = _tile_batch(targets, tix, qs, max_ql=520)
        protein.run_local(b, aligner, code, mat, 11, 1, score_only=True, shared_target=True)
        torch.cuda.synchronize()
        assert _kernel(aligner) == kernel
        _check_scores(b, targets, tix, qs, code, mat, 11, 1)
        assert int(b.hits[1, 0]) == 520 * smax


def test_dna_pm_matrix(aligner):
    from mgl_amd import protein

    rng = np.random.default_rng(26)
    code, mat = protein.dna_matrix(2, -3)
    ref = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 2000)])
    ts, qs = [], []
    for k in range(100):
        s = int(rng.integers(0, 1800))
        ts.append(ref[s:s + 200])
        r = bytearray(ref[s + 20:s + 170])
        for _ in range(5):
            r[int(rng.integers(0, len(r)))] = ord("ACGTN"[rng.integers(0, 5)])
        qs.append(bytes(r).lower() if k % 2 else bytes(r))
    b = _batch(ts, qs)
    protein.run_local(b, aligner, code, mat, 5, 2)
    _check_full(b, ts, qs, code, mat, 5, 2)


def test_local_search_top_k(aligner):
    from mgl_amd import protein

    rng = np.random.default_rng(27)
    code, mat = protein.blosum62()
    D = 60
    lens = rng.integers(20, 260, D)
    seqs = [bytes(PROTA[rng.integers(len(PROT), size=int(L))]) for L in lens]
    seqs[7] = seqs[3]  # a tie: same score, the smaller database index first
    lens = np.array([len(x) for x in seqs])
    queries = [_mutate(rng, seqs[int(rng.integers(D))][10:150]) for _ in range(150)] + [b"", b"W"]
    db = np.frombuffer(b"".join(seqs), np.uint8).copy()
    db_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    s = protein.LocalSearch(db, db_off, queries, torch.device("cuda", 0))
    res = s.run(aligner, code, mat, 11, 1, top_k=5)
    want_scores = np.array([[lt.local_align_np(t, q, code, mat, 11, 1)[0] for q in queries] for t in seqs])
    assert (res["scores"].cpu().numpy() == want_scores).all()
    want_idx = lt.top_k(want_scores.T, 5)
    assert (res["index"] == want_idx).all()
    for q in range(len(queries)):
        for r in range(5):
            want = lt.local_align_np(seqs[want_idx[q, r]], queries[q], code, mat, 11, 1)
            assert res["score"][q, r] == want[0] and tuple(res["hits"][q, r]) == want[:5] and res["cigars"][q][r] == want[5]
