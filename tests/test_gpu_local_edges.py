"""mgl_sw_local_batch_device_matrix at its edges, seams and ties, bit-exact against the textbook DP (tests/local_textbook.py): kernel A
(sw_local_lane.hip) at the last length its 16-bit guard admits, on full-range / all-non-negative / all-non-positive matrices, with gap
constants at 16 bits, negative and o < e penalties, targets as long as its LDS carve, vertical gaps across its 32-row seams and every
shape of a tile's longest query; kernel B (sw_local.hip) on tied end cells and tied walks, gaps across its 64-row carry, pairs of
thousands of residues, a workspace small enough to cut the batch into many launches, per-pair error statuses, the exact CIGAR stride and
canaries around every output; LocalSearch at its degenerate shapes.  The inputs come from tests/local_cases.py, whose claims
tests/test_local_cases.py checks without a GPU.  Every comparison is exact; values are compared before the kernel's name, so that a
failure shows the values.

The CPU reference is what takes the time here.  Measured on the development machine: local_align_np on one 3 000 x 3 000 pair
0.6 s; local_scores_np on one tile of 128 queries of at most 100 residues against 63 200 residues 19 s."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import local_cases as lc  # noqa: E402
import local_textbook as lt  # noqa: E402

pytestmark = pytest.mark.gpu

PROT = b"ARNDCQEGHILKMFPSTWYV"
PROTA = np.frombuffer(PROT, np.uint8)
A, B = "sw_local_lane_kernel", "sw_local_pair_kernel"
SMALL_WORKSPACE = 1 << 20  # the smallest mgl_sw_ctx_set_workspace takes


def _aligner():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mgl_amd import smithwaterman as sw

    a = sw.MicrosoftSmithWaterman(0)
    assert a.load()
    return a


@pytest.fixture(scope="module")
def aligner():
    a = _aligner()
    yield a
    a.close()


@pytest.fixture(scope="module")
def small_aligner():
    """A second aligner whose workspace limit is 1 MiB."""
    a = _aligner()
    a.set_workspace(SMALL_WORKSPACE)
    yield a
    a.close()


def _prot(rng, n):
    return PROTA[rng.integers(len(PROT), size=int(n))].tobytes()


def _raw(rng, n, hi=256):
    return rng.integers(0, hi, size=int(n), dtype=np.uint8).tobytes()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _offsets(seqs):
    return np.concatenate([[0], np.cumsum([len(s) for s in seqs])])[:-1].astype(np.int64)


def _batch(ts, qs, cigar_stride=512, max_tl=None, max_ql=None, t_len=None, q_len=None):
    """One target per pair.  t_len / q_len: the lengths to DECLARE (default: the real ones)."""
    from mgl_amd import protein

    tb, qb = b"".join(ts) + b"\0" * 8, b"".join(qs) + b"\0" * 8
    tl = np.array([len(t) for t in ts] if t_len is None else t_len, np.int32)
    ql = np.array([len(q) for q in qs] if q_len is None else q_len, np.int32)
    return protein.LocalBatch(_dev(np.frombuffer(tb, np.uint8).copy()), _dev(_offsets(ts)), _dev(tl),
                              _dev(np.frombuffer(qb, np.uint8).copy()), _dev(_offsets(qs)), _dev(ql),
                              max(1, max(len(t) for t in ts)) if max_tl is None else max_tl,
                              max(1, max(len(q) for q in qs)) if max_ql is None else max_ql, cigar_stride)


def _tile_batch(targets, tix, qs, max_tl=None, max_ql=None):
    """Pair k: targets[tix[k]] against qs[k]; blocks of 128 pairs share their target."""
    from mgl_amd import protein

    tb, qb = b"".join(targets) + b"\0" * 8, b"".join(qs) + b"\0" * 8
    tix = np.asarray(tix)
    return protein.LocalBatch(_dev(np.frombuffer(tb, np.uint8).copy()), _dev(_offsets(targets)[tix]),
                              _dev(np.array([len(targets[k]) for k in tix], np.int32)), _dev(np.frombuffer(qb, np.uint8).copy()),
                              _dev(_offsets(qs)), _dev(np.array([len(q) for q in qs], np.int32)),
                              max(len(t) for t in targets) if max_tl is None else max_tl,
                              max(1, max(len(q) for q in qs)) if max_ql is None else max_ql, 0)


def _kernel(aligner):
    from mgl_amd import _lib

    return _lib.FILL_KERNEL_NAMES[aligner.timing().fill_kernel]


def _run_tiles(aligner, targets, tix, qs, code, mat, o, e, kernel, max_tl=None, max_ql=None, shared=True, want=None):
    """A score pass over shared-target tiles: every score equals the textbook's, every other field is 0, every status 0; then the
    kernel's name (kernel None: the caller checks it).  Returns the scores."""
    from mgl_amd import protein

    b = _tile_batch(targets, tix, qs, max_tl, max_ql)
    b.hits.fill_(-7)
    b.status.fill_(-7)
    protein.run_local(b, aligner, code, mat, o, e, score_only=True, shared_target=shared)
    torch.cuda.synchronize()
    ran = _kernel(aligner)
    hits, st = b.hits.cpu().numpy(), b.status.cpu().numpy()
    if want is None:
        want = np.zeros(len(qs), np.int64)
        tix = np.asarray(tix)
        for k in sorted(set(tix.tolist())):
            sel = np.nonzero(tix == k)[0]
            want[sel] = lt.local_scores_np(targets[k], [qs[p] for p in sel], code, mat, o, e)
    bad = np.nonzero(hits[:, 0] != want)[0]
    assert len(bad) == 0, (ran, (o, e), len(bad), [(int(k), int(hits[k, 0]), int(want[k]), len(qs[k])) for k in bad[:8]])
    assert (st == 0).all() and (hits[:, 1:] == 0).all(), (st[st != 0][:8], hits[(hits[:, 1:] != 0).any(axis=1)][:4])
    assert kernel is None or ran == kernel
    return hits[:, 0].copy()


def _run_full(aligner, pairs, code, mat, o, e, binary=False, cigar_stride=512, expect=None):
    """Kernel B with full output over [(t, q)]: all five hit fields and the CIGAR equal the textbook's, status 0, and nothing is written
    outside a pair's own outputs (the CIGAR rows are pre-filled with 0xA5).  Returns the LocalBatch."""
    from mgl_amd import protein

    ts, qs = [p[0] for p in pairs], [p[1] for p in pairs]
    b = _batch(ts, qs, cigar_stride)
    b.cigars.fill_(0xA5)
    b.hits.fill_(-7)
    protein.run_local(b, aligner, code, mat, o, e, binary_cigar=binary)
    torch.cuda.synchronize()
    ran = _kernel(aligner)
    hits, st, ln, raw = b.hits.cpu().numpy(), b.status.cpu().numpy(), b.cigar_len.cpu().numpy(), b.cigars.cpu().numpy()
    cig = b.cigar_strings(binary=binary)
    for k, (t, q) in enumerate(zip(ts, qs)):
        want = expect[k] if expect is not None else lt.local_align_np(t, q, code, mat, o, e)
        got_c = lt.cigar_binary_to_text(cig[k]) if binary else cig[k]
        assert st[k] == 0 and tuple(int(x) for x in hits[k]) == want[:5] and got_c == want[5], (k, t, q, (o, e), st[k], hits[k], got_c, want)
        assert (raw[k, ln[k]:] == 0xA5).all(), (k, ln[k])
    assert ran == B
    return b


def _groups(pairs):
    """[(t, q, key, o, e, ...)] -> {(key, o, e): [(t, q)]}, in order."""
    out = {}
    for p in pairs:
        out.setdefault((p[2], p[3], p[4]), []).append((p[0], p[1]))
    return out


# ---- kernel A --------------------------------------------------------------------------------------------------------------------------
def test_kernel_a_at_the_last_length_of_its_guard(aligner):
    """guard_edge_tiles(): at L (smax L + 255 = 65 533 and 65 535) kernel A runs, at L + 1 and L + 3 kernel B; all 128 scores equal the
    textbook's and the identical pair -- in a lane's low half, its high half and both -- scores smax times its length.  The values of
    all six tiles are compared before any kernel's name: a guard that lets L + 3 through shows as wrapped scores."""
    ran = []
    for smin, smax, L, length, code, mat, t, qs in lc.guard_edge_tiles():
        got = _run_tiles(aligner, [t], [0] * 128, qs, code, mat, 11, 1, None, max_tl=length, max_ql=length)
        ran.append((smax, length, _kernel(aligner), A if length == L else B))
        for slot in (lc.SLOT_LOW, lc.SLOT_HIGH, lc.SLOT_BOTH, lc.SLOT_BOTH + 1):
            assert got[slot] == smax * length, (smax, length, slot, got[slot])
        assert got[lc.SLOT_LOW + 1] == 0 and got[lc.SLOT_HIGH - 1] == 0
    assert all(got == want for _, _, got, want in ran), ran


def _mixed_tiles(rng, n_tiles, tl_choices, ql_max, maker, last_short=0):
    targets, tix, qs = [], [], []
    for k in range(n_tiles):
        t = maker(rng, tl_choices[k % len(tl_choices)])
        targets.append(t)
        for p in range(last_short if (last_short and k == n_tiles - 1) else 128):
            r = rng.random()
            if r < 0.06:
                q = b""
            elif r < 0.4 and len(t) > 4:
                q = t[int(rng.integers(0, len(t) // 2)):][:ql_max]
            else:
                q = maker(rng, rng.integers(1, ql_max + 1))
            tix.append(k)
            qs.append(q)
    return targets, tix, qs


def test_kernel_a_full_range_matrix(aligner):
    """min(S) = -128, max(S) = 127: profile bytes 0 .. 255, K = 128.  Asymmetric, all 32 codes in use."""
    rng = np.random.default_rng(201)
    mat = rng.integers(-128, 128, size=(32, 32)).astype(np.int8)
    mat[5, 9], mat[9, 5], mat[0, 0], mat[31, 31] = -128, 127, 127, -128
    code = (np.arange(256) % 32).astype(np.uint8)
    assert not (mat == mat.T).all() and lt.local_lane_ok(-128, 127, 11, 1, 400, 200)
    targets, tix, qs = _mixed_tiles(rng, 6, (1, 31, 32, 33, 200, 400), 200, _raw, last_short=51)
    _run_tiles(aligner, targets, tix, qs, code, mat, 11, 1, A, max_ql=200)
    _run_tiles(aligner, targets, tix, qs, code, mat, 40, 3, A, max_ql=200)


def test_kernel_a_matrix_without_a_negative_entry(aligner):
    """K = 0: ghost columns and the rows below the target score exactly 0, as real cells may.  Mixed query lengths and holes in a tile."""
    rng = np.random.default_rng(202)
    mat = rng.integers(0, 10, size=(32, 32)).astype(np.int8)
    mat[rng.random((32, 32)) < 0.3] = 0
    code = (np.arange(256) % 32).astype(np.uint8)
    assert mat.min() == 0 and lt.local_lane_bias(int(mat.min())) == 0
    targets, tix, qs = _mixed_tiles(rng, 6, (1, 30, 33, 64, 95, 130), 120, _raw, last_short=77)
    assert any(q == b"" for q in qs[:128]) and len({len(q) for q in qs[:128]}) > 20
    for o, e in [(11, 1), (3, 0), (0, 0)]:
        _run_tiles(aligner, targets, tix, qs, code, mat, o, e, A)


def test_kernel_a_matrix_without_a_positive_entry(aligner):
    rng = np.random.default_rng(203)
    code = (np.arange(256) % 32).astype(np.uint8)
    targets, tix, qs = _mixed_tiles(rng, 3, (20, 64, 100), 80, _raw)
    for mat in (rng.integers(-9, 1, size=(32, 32)).astype(np.int8), np.zeros((32, 32), np.int8), np.full((32, 32), -128, np.int8)):
        got = _run_tiles(aligner, targets, tix, qs, code, mat, 11, 1, A, want=np.zeros(len(qs), np.int64))
        assert (got == 0).all()


def test_gap_constants_at_16_bits(aligner):
    """gopen / gext = 65 535 are kernel A's last, 65 536 goes to kernel B: the textbook's scores either way (no gap ever pays)."""
    from mgl_amd import protein

    rng = np.random.default_rng(204)
    code, mat = protein.blosum62()
    targets, tix, qs = _mixed_tiles(rng, 2, (150, 90), 140, _prot, last_short=60)
    for o, e, kernel in [(65535, 65535, A), (65535, 1, A), (3, 65535, A), (65536, 65536, B), (65536, 1, B), (3, 65536, B)]:
        assert lt.local_lane_ok(-4, 11, o, e, 150, 140) == (kernel == A)
        _run_tiles(aligner, targets, tix, qs, code, mat, o, e, kernel)


def test_negative_penalties_are_their_absolute_values(aligner):
    from mgl_amd import protein

    rng = np.random.default_rng(205)
    code, mat = protein.blosum62()
    targets, tix, qs = _mixed_tiles(rng, 2, (120, 64), 100, _prot, last_short=40)
    pos = _run_tiles(aligner, targets, tix, qs, code, mat, 11, 1, A)
    neg = _run_tiles(aligner, targets, tix, qs, code, mat, -11, -1, A)
    assert (pos == neg).all()
    pairs = [(targets[tix[k]], qs[k]) for k in range(0, len(qs), 3)]
    b1 = _run_full(aligner, pairs, code, mat, 11, 1)
    b2 = _run_full(aligner, pairs, code, mat, -11, -1)
    assert torch.equal(b1.hits, b2.hits) and torch.equal(b1.cigar_len, b2.cigar_len) and b1.cigar_strings() == b2.cigar_strings()


@pytest.mark.parametrize("o,e", [(1, 4), (0, 3)])
def test_open_cheaper_than_extend(aligner, o, e):
    """o < e: an H that F made opens a better gap than its source (the textbook needs its cell-by-cell branch).  Kernel A's scores and
    kernel B's full output."""
    from mgl_amd import protein

    rng = np.random.default_rng(206 + o)
    code, mat = protein.blosum62()
    targets, tix, qs = _mixed_tiles(rng, 2, (70, 33), 60, _prot, last_short=30)
    _run_tiles(aligner, targets, tix, qs, code, mat, o, e, A)
    dcode, dmat = lt.dna_matrix(2, -3)
    pairs = [(targets[tix[k]], qs[k]) for k in range(0, len(qs), 4)]
    _run_full(aligner, pairs, code, mat, o, e)
    _run_full(aligner, [(p[0], p[1]) for p in lc.walk_tie_pairs()[:40]], dcode, dmat, o, e, binary=True)


def _long_tile(rng, tl, deep_from):
    """One target of tl residues and 128 queries of 1 .. 100: a third cut from the target beyond row deep_from (with a substitution and
    a short deletion), the others random, two holes."""
    t = _prot(rng, tl)
    qs = []
    for k in range(128):
        n = int(rng.integers(1, 101))
        if k % 3 == 0 and tl > n + 8:
            s = int(rng.integers(min(deep_from, tl - n - 8), tl - n - 4))
            q = bytearray(t[s:s + n + 4])
            if n > 20:
                del q[n // 2:n // 2 + 4]
                q[3] = PROT[int(rng.integers(20))]
            q = bytes(q[:n])
        else:
            q = _prot(rng, n)
        qs.append(q)
    qs[17] = qs[90] = b""
    qs[127] = t[tl - 100:]  # ends in the target's last row
    return t, qs


def test_kernel_a_targets_as_long_as_its_lds_carve(aligner):
    """max_tl = 63 200: 1 975 strips, 64 KiB of dynamic LDS, the best cells beyond strip 1 000.  The same tile with max_tl = 63 201
    declared is outside the guard and runs kernel B: equal scores.  And a tile of 33-residue targets with max_tl = 63 200 declared."""
    from mgl_amd import protein

    rng = np.random.default_rng(207)
    code, mat = protein.blosum62()
    limit = 63200
    assert lt.local_lane_ok(-4, 11, 11, 1, limit, 100) and not lt.local_lane_ok(-4, 11, 11, 1, limit + 1, 100)
    assert lt.local_lane_lds_bytes(limit) == 64 * 1024
    t, qs = _long_tile(rng, limit, 32 * 1000)
    want = lt.local_scores_np(t, qs, code, mat, 11, 1)
    assert want[127] >= 400 and (want[::3] > 40).sum() > 15  # the cut queries are found, the last in the target's last row
    a = _run_tiles(aligner, [t], [0] * 128, qs, code, mat, 11, 1, A, max_tl=limit, max_ql=100, want=want)
    b = _run_tiles(aligner, [t], [0] * 128, qs, code, mat, 11, 1, B, max_tl=limit + 1, max_ql=100, want=want)
    assert (a == b).all()
    t2, qs2 = _long_tile(rng, 20000, 16000)
    _run_tiles(aligner, [t2], [0] * 128, qs2, code, mat, 11, 1, A, max_tl=limit, max_ql=100)
    shorts = [_prot(rng, 33) for _ in range(3)]
    tix = [0] * 128 + [1] * 128 + [2] * 19
    qs3 = [shorts[k][int(rng.integers(0, 10)):] if p % 2 else _prot(rng, rng.integers(1, 101)) for p, k in enumerate(tix)]
    _run_tiles(aligner, shorts, tix, qs3, code, mat, 11, 1, A, max_tl=limit, max_ql=100)


def test_kernel_a_vertical_gaps_across_its_strip_seams(aligner):
    """seam_gap_pairs(32): E leaves a strip through the carry row and enters the next.  One tile per gap model, its queries repeated
    to 128 pairs (so each sits in low and high halves of several lanes)."""
    for (key, o, e), pairs in _groups(lc.seam_gap_pairs(32)).items():
        code, mat = lc.scoring(key)
        t = pairs[0][0]
        assert all(p[0] == t for p in pairs)
        uniq = [p[1] for p in pairs]
        want_u = lt.local_scores_np(t, uniq, code, mat, o, e)
        idx = [(k * 5) % len(uniq) if k % 2 else k % len(uniq) for k in range(128)]
        _run_tiles(aligner, [t], [0] * 128, [uniq[k] for k in idx], code, mat, o, e, A, want=want_u[idx])


def test_kernel_a_longest_query_of_a_tile_and_declared_bound(aligner):
    """A tile's longest query at every residue mod 4 (the column loop leaves its group of four early) and max_ql at, just above and far
    above it; and a tile whose queries are all holes."""
    from mgl_amd import protein

    rng = np.random.default_rng(208)
    code, mat = protein.blosum62()
    t = _prot(rng, 45)
    for qmax in range(1, 10):
        qs = [t[s:s + n] if k % 2 else _prot(rng, n) for k in range(128) for n, s in [(int(rng.integers(0, qmax + 1)), int(rng.integers(0, 30)))]]
        qs[2 * int(rng.integers(0, 64)) + qmax % 2] = t[7:7 + qmax]
        want = lt.local_scores_np(t, qs, code, mat, 11, 1)
        assert max(len(q) for q in qs) == qmax
        for max_ql in (qmax, qmax + 1, qmax + 3, 300):
            _run_tiles(aligner, [t], [0] * 128, qs, code, mat, 11, 1, A, max_ql=max_ql, want=want)
    for max_ql in (1, 5):
        _run_tiles(aligner, [t, t[:9]], [0] * 128 + [1] * 5, [b""] * 133, code, mat, 11, 1, A, max_ql=max_ql, want=np.zeros(133, np.int64))


# ---- kernel B --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binary", [False, True])
def test_kernel_b_tied_end_cells(aligner, binary):
    """tied_pairs(): the maximum in many cells -- across the columns of a row, across lanes, across strips, and where row-first and
    column-first orders disagree.  The end is the smallest (i, j), row first."""
    for (key, o, e), pairs in _groups(lc.tied_pairs()).items():
        code, mat = lc.scoring(key)
        _run_full(aligner, pairs, code, mat, o, e, binary=binary)


@pytest.mark.parametrize("binary", [False, True])
def test_kernel_b_tied_walks(aligner, binary):
    """walk_tie_pairs(): the diagonal before F before E, extension before opening."""
    for (key, o, e), pairs in _groups(lc.walk_tie_pairs()).items():
        code, mat = lc.scoring(key)
        _run_full(aligner, pairs, code, mat, o, e, binary=binary)


@pytest.mark.parametrize("binary", [False, True])
def test_kernel_b_long_gaps_across_the_carry_row(aligner, binary):
    """seam_gap_pairs(64): deletions that begin above row 64 k and end below it, insertions longer than a strip has lanes."""
    for (key, o, e), pairs in _groups(lc.seam_gap_pairs(64)).items():
        code, mat = lc.scoring(key)
        _run_full(aligner, pairs, code, mat, o, e, binary=binary, cigar_stride=1024)


def test_kernel_b_large_pairs(aligner):
    """tl and ql of 1 500 .. 3 000 (up to 47 strips); targets of exactly 64 k and 64 k + 1 rows; an identical pair of 1 234 ('1234M',
    a run of four digits); a deletion of 1 000."""
    from mgl_amd import protein

    rng = np.random.default_rng(209)
    code, mat = protein.blosum62()

    def mutated(s, rate=0.1):
        out = bytearray()
        for ch in s:
            r = rng.random()
            if r < 0.01:
                continue
            if r < 0.02:
                out += _prot(rng, rng.integers(1, 4))
            out.append(PROT[int(rng.integers(20))] if rng.random() < rate else ch)
        return bytes(out)

    pairs = []
    t = _prot(rng, 1234)
    pairs.append((t, t))
    t = _prot(rng, 3000)
    pairs.append((t, t[200:900] + t[1900:2800]))                       # 700M1000D900M
    pairs.append((t[200:1000] + t[1500:2900], t[100:2950]))            # an insertion of 500
    for tl in (64 * 24, 64 * 24 + 1, 64 * 32, 64 * 32 + 1, 64 * 47, 64 * 47 - 1):
        t = _prot(rng, tl)
        pairs.append((t, mutated(t[int(rng.integers(0, 100)):])[:3000]))
    pairs.append((_prot(rng, 2500), _prot(rng, 1500)))                 # unrelated
    t = _prot(rng, 1600)
    pairs.append((t, _prot(rng, 900) + t[900:] + _prot(rng, 500)))     # the hit deep in both
    pairs.append((mutated(t, 0.3), t))
    assert len(pairs) >= 12 and max(len(p[0]) for p in pairs) >= 3000
    expect = [lt.local_align_np(t, q, code, mat, 11, 1) for t, q in pairs]
    assert expect[0][5] == "1234M" and "1000D" in expect[1][5] and "500I" in expect[2][5]
    _run_full(aligner, pairs, code, mat, 11, 1, cigar_stride=4096, expect=expect)
    _run_full(aligner, pairs, code, mat, 11, 1, cigar_stride=4096, expect=expect, binary=True)


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


def _ragged(rng, n):
    """The batch of test_gpu_local.py's test_kernel_b_ragged_protein."""
    ts, qs = [], []
    for k in range(n):
        tl = int(rng.integers(0, 300)) if k % 11 else 0
        t = bytes(PROTA[rng.integers(len(PROT), size=tl)]) if tl else b""
        kind = k % 5
        if kind == 0 and tl > 20:
            q = _mutate(rng, t[int(rng.integers(0, tl // 3)):])
        elif kind == 1:
            q = bytes(PROTA[rng.integers(len(PROT), size=int(rng.integers(1, 250)))]).lower()
        elif kind == 2:
            q = bytes(rng.integers(0, 256, size=int(rng.integers(1, 120)), dtype=np.uint8))
        elif kind == 3:
            q = b"BZX*" * int(rng.integers(1, 20)) + (t[:40] if t else b"")
        else:
            q = bytes(PROTA[rng.integers(len(PROT), size=int(rng.integers(0, 200)))])
        if k % 13 == 5:
            q = b""
        ts.append(t)
        qs.append(q)
    return ts, qs


def _launches(aligner):
    """Kernel launches of the last call on this aligner (mgl_sw_ctx_get_timing counts per call)."""
    return int(aligner.timing().dp_launches)


def test_kernel_b_chunked_equals_one_launch(aligner, small_aligner):
    """The ragged batch under a workspace limit of 1 MiB: a slot is the largest pair's (about 100 KiB for 299 x 249), so 300 pairs
    take 8 launches or more, every one but the first with a.first > 0 into reused slots.  Hits, CIGARs and statuses equal those of
    the one-launch run and the textbook's."""
    from mgl_amd import protein

    code, mat = protein.blosum62()
    ts, qs = _ragged(np.random.default_rng(11), 300)
    pairs = list(zip(ts, qs))
    expect = [lt.local_align_np(t, q, code, mat, 11, 1) for t, q in pairs]
    one = _run_full(aligner, pairs, code, mat, 11, 1, expect=expect)
    assert _launches(aligner) == 1
    cut = _run_full(small_aligner, pairs, code, mat, 11, 1, expect=expect)
    assert _launches(small_aligner) >= 8, _launches(small_aligner)
    for name in ("hits", "status", "cigar_len", "cigars"):
        assert torch.equal(getattr(one, name), getattr(cut, name)), name


def test_small_workspace_pairs_too_large_for_it(small_aligner):
    """Two pairs of 1 000 x 1 000 need 1.1 MB of decisions each, more than the whole limit: MGL_SW_ERR_UNSUPPORTED for them, a zero hit,
    no CIGAR; the others are right."""
    from mgl_amd import _lib, protein

    rng = np.random.default_rng(210)
    code, mat = protein.blosum62()
    ts = [_prot(rng, rng.integers(1, 200)) for _ in range(40)]
    qs = [_mutate(rng, t) or b"A" for t in ts]
    big = (7, 31)
    for k in big:
        ts[k] = _prot(rng, 1000)
        qs[k] = ts[k]
    b = _batch(ts, qs, cigar_stride=256)
    b.cigars.fill_(0xA5)
    b.hits.fill_(-7)
    b.cigar_len.fill_(-7)
    protein.run_local(b, small_aligner, code, mat, 11, 1)
    torch.cuda.synchronize()
    hits, st, ln, raw = b.hits.cpu().numpy(), b.status.cpu().numpy(), b.cigar_len.cpu().numpy(), b.cigars.cpu().numpy()
    cig = b.cigar_strings()
    for k, (t, q) in enumerate(zip(ts, qs)):
        if k in big:
            assert st[k] == _lib.ERR_UNSUPPORTED and (hits[k] == 0).all() and ln[k] == 0 and (raw[k] == 0xA5).all(), (k, st[k], hits[k], ln[k])
        else:
            want = lt.local_align_np(t, q, code, mat, 11, 1)
            assert st[k] == 0 and tuple(int(x) for x in hits[k]) == want[:5] and cig[k] == want[5], (k, st[k], hits[k], cig[k], want)
            assert (raw[k, ln[k]:] == 0xA5).all()
    assert _kernel(small_aligner) == B


def test_small_workspace_kernel_a_not_taken(aligner, small_aligner):
    """24 shared-target tiles inside kernel A's guard: 1 MiB holds the regions of 15 wave slots (66 048 bytes each at max_ql = 100), fewer
    than the tiles, so the score pass falls to kernel B (1 024 pairs a launch: 3 launches) with the scores kernel A gives."""
    from mgl_amd import protein

    rng = np.random.default_rng(211)
    code, mat = protein.blosum62()
    targets, tix, qs = _mixed_tiles(rng, 24, (40, 33, 64, 20), 100, _prot, last_short=50)
    a = _run_tiles(aligner, targets, tix, qs, code, mat, 11, 1, A, max_ql=100)
    b = _run_tiles(small_aligner, targets, tix, qs, code, mat, 11, 1, B, max_ql=100, want=a)
    assert (a == b).all() and _launches(small_aligner) == 3


def test_kernel_b_per_pair_bad_arg(aligner):
    """Lengths beyond the declared max_tl / max_ql and a negative length, scattered among good pairs: MGL_SW_ERR_BAD_ARG, a zero hit and
    no CIGAR for those; the others are right."""
    from mgl_amd import _lib, protein

    rng = np.random.default_rng(212)
    code, mat = protein.blosum62()
    ts = [_prot(rng, rng.integers(1, 100)) for _ in range(50)]
    qs = [_mutate(rng, t)[:90] or b"A" for t in ts]
    ts[3], qs[20] = _prot(rng, 101), _prot(rng, 91)            # one beyond each bound
    ts[44], qs[44] = _prot(rng, 150), _prot(rng, 150)          # both
    t_len, q_len = [len(t) for t in ts], [len(q) for q in qs]
    t_len[9], q_len[30], q_len[49] = -1, -5, -(1 << 31)
    bad = {3, 20, 44, 9, 30, 49}
    for score_only in (False, True):
        b = _batch(ts, qs, cigar_stride=256, max_tl=100, max_ql=90, t_len=t_len, q_len=q_len)
        b.cigars.fill_(0xA5)
        b.hits.fill_(-7)
        b.cigar_len.fill_(-7)
        protein.run_local(b, aligner, code, mat, 11, 1, score_only=score_only)
        torch.cuda.synchronize()
        hits, st, ln, raw = b.hits.cpu().numpy(), b.status.cpu().numpy(), b.cigar_len.cpu().numpy(), b.cigars.cpu().numpy()
        for k, (t, q) in enumerate(zip(ts, qs)):
            if k in bad:
                assert st[k] == _lib.ERR_BAD_ARG and (hits[k] == 0).all() and (raw[k] == 0xA5).all(), (k, st[k], hits[k])
                assert score_only or ln[k] == 0
                continue
            want = lt.local_align_np(t, q, code, mat, 11, 1)
            if score_only:
                assert st[k] == 0 and hits[k, 0] == want[0] and (hits[k, 1:] == 0).all() and (raw[k] == 0xA5).all(), (k, hits[k], want)
            else:
                assert st[k] == 0 and tuple(int(x) for x in hits[k]) == want[:5] and raw[k, :ln[k]].tobytes().decode() == want[5], (k, hits[k], want)
                assert (raw[k, ln[k]:] == 0xA5).all()
        assert _kernel(aligner) == B


@pytest.mark.parametrize("binary", [False, True])
def test_cigar_stride_exactly_the_size_needed(aligner, binary):
    """cigar_stride equal to a pair's size: status 0 and the whole CIGAR; one less: MGL_SW_ERR_CIGAR_OVERFLOW, cigar_len the size, the hit
    complete, nothing written to the row.  Every pair of the batch is judged against the stride the same way."""
    from mgl_amd import _lib, protein

    rng = np.random.default_rng(213)
    code, mat = protein.blosum62()
    ts = [_prot(rng, 180) for _ in range(24)]
    qs = [_mutate(rng, t, 0.2, 0.04 + 0.004 * k) for k, t in enumerate(ts)]
    want = [lt.local_align_np(t, q, code, mat, 11, 1) for t, q in zip(ts, qs)]
    size = [4 * len(lc.cigar_runs(w[5], 0)) if binary else len(w[5]) for w in want]
    pick = int(np.argsort(size)[len(size) // 2])
    assert size[pick] >= 8 and min(size) < size[pick] < max(size)
    for stride in (size[pick], size[pick] - 1):
        b = _batch(ts, qs, cigar_stride=stride)
        b.cigars.fill_(0xA5)
        protein.run_local(b, aligner, code, mat, 11, 1, binary_cigar=binary)
        torch.cuda.synchronize()
        hits, st, ln, raw = b.hits.cpu().numpy(), b.status.cpu().numpy(), b.cigar_len.cpu().numpy(), b.cigars.cpu().numpy()
        for k, w in enumerate(want):
            assert tuple(int(x) for x in hits[k]) == w[:5] and ln[k] == size[k], (k, stride, hits[k], ln[k], size[k], w)
            if size[k] <= stride:
                got = lt.cigar_binary_to_text(raw[k, :ln[k]].view(np.uint32)) if binary else raw[k, :ln[k]].tobytes().decode()
                assert st[k] == 0 and got == w[5] and (raw[k, ln[k]:] == 0xA5).all(), (k, stride, st[k], got, w)
            else:
                assert st[k] == _lib.ERR_CIGAR_OVERFLOW and (raw[k] == 0xA5).all(), (k, stride, st[k])
        assert (st[pick] == 0) == (stride == size[pick])
    assert _kernel(aligner) == B


def test_kernel_b_writes_nothing_outside_a_pairs_outputs(aligner):
    """Canaries: cigars pre-filled with 0xA5, hits with -7.  Every byte at or beyond cigar_len[k] of row k stays 0xA5; the row of a hole,
    of a pair that scores 0 and of a pair with an error status holds no CIGAR byte; a pair with BAD_ARG gets a zero hit (include/mgl_sw.h
    says so)."""
    from mgl_amd import _lib, protein

    rng = np.random.default_rng(214)
    code, mat = lt.dna_matrix(2, -3)
    ts, qs = [], []
    for k in range(64):
        t = _raw(rng, rng.integers(1, 150), 4)
        t = bytes(b"ACGT"[c] for c in t)
        ts.append(t)
        gapped = bytes(c for x, c in enumerate(t) if x % 12 != 7)  # a deletion every 12 residues: a CIGAR beyond 16 bytes
        qs.append([t[5:] or t, b"", b"N" * 20, gapped][k % 4])
    t_len = [len(t) for t in ts]
    t_len[12], t_len[41] = 1000, -2  # beyond max_tl, negative
    b = _batch(ts, qs, cigar_stride=16, t_len=t_len)
    b.cigars.fill_(0xA5)
    b.hits.fill_(-7)
    b.cigar_len.fill_(-7)
    b.status.fill_(-7)
    protein.run_local(b, aligner, code, mat, 5, 2)
    torch.cuda.synchronize()
    hits, st, ln, raw = b.hits.cpu().numpy(), b.status.cpu().numpy(), b.cigar_len.cpu().numpy(), b.cigars.cpu().numpy()
    seen = set()
    for k, (t, q) in enumerate(zip(ts, qs)):
        if k in (12, 41):
            assert st[k] == _lib.ERR_BAD_ARG and (hits[k] == 0).all() and ln[k] == 0 and (raw[k] == 0xA5).all(), (k, st[k], hits[k], ln[k])
            continue
        want = lt.local_align_np(t, q, code, mat, 5, 2)
        assert tuple(int(x) for x in hits[k]) == want[:5], (k, hits[k], want)
        if want[0] == 0:
            seen.add("zero")
            assert st[k] == 0 and ln[k] == 0 and (raw[k] == 0xA5).all(), (k, st[k], ln[k])
        elif len(want[5]) > 16:
            seen.add("overflow")
            assert st[k] == _lib.ERR_CIGAR_OVERFLOW and ln[k] == len(want[5]) and (raw[k] == 0xA5).all(), (k, st[k], ln[k], want)
        else:
            seen.add("fits")
            assert st[k] == 0 and raw[k, :ln[k]].tobytes().decode() == want[5] and (raw[k, ln[k]:] == 0xA5).all(), (k, st[k], want)
    assert seen == {"zero", "overflow", "fits"}
    assert _kernel(aligner) == B


# ---- LocalSearch -----------------------------------------------------------------------------------------------------------------------
def _search(aligner, seqs, queries, top_k):
    from mgl_amd import protein

    code, mat = protein.blosum62()
    lens = np.array([len(s) for s in seqs])
    db = np.frombuffer(b"".join(seqs), np.uint8).copy()
    db_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    s = protein.LocalSearch(db, db_off, queries, torch.device("cuda", 0))
    res = s.run(aligner, code, mat, 11, 1, top_k=top_k)
    want_scores = np.array([lt.local_scores_np(t, queries, code, mat, 11, 1) for t in seqs]).reshape(len(seqs), len(queries))
    assert (res["scores"].cpu().numpy() == want_scores).all()
    K = min(top_k, len(seqs))
    want_idx = lt.top_k(want_scores.T, K)
    assert res["index"].shape == (len(queries), K) and (res["index"] == want_idx).all()
    for q in range(len(queries)):
        for r in range(K):
            want = lt.local_align_np(seqs[want_idx[q, r]], queries[q], code, mat, 11, 1)
            assert res["status"][q, r] == 0 and res["score"][q, r] == want[0] and tuple(res["hits"][q, r]) == want[:5] and res["cigars"][q][r] == want[5], (q, r, want)
    return res


def test_local_search_degenerate_shapes(aligner):
    """D = 1; Q = 1; top_k > D; Q = 128 and 129 exactly (one full tile; one full tile and one pair); every query empty."""
    rng = np.random.default_rng(215)
    seqs = [_prot(rng, rng.integers(20, 120)) for _ in range(5)]
    some = lambda n: [_mutate(rng, seqs[int(rng.integers(len(seqs)))][5:70]) or b"W" for _ in range(n)]  # noqa: E731
    _search(aligner, seqs[:1], some(9), top_k=1)            # D = 1
    _search(aligner, seqs, some(1), top_k=3)                # Q = 1
    _search(aligner, seqs[:3], some(6), top_k=10)           # top_k > D
    _search(aligner, seqs[:1], some(1), top_k=4)            # all three
    _search(aligner, seqs, some(128), top_k=2)
    _search(aligner, seqs, some(129), top_k=2)
    res = _search(aligner, seqs, [b""] * 7, top_k=2)        # every query empty: all scores 0, the first database sequences, empty CIGARs
    assert (res["score"] == 0).all() and (res["index"] == [0, 1]).all() and all(c == ["", ""] for c in res["cigars"])
