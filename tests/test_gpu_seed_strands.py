"""mgl_sw_seed_strands_batch_device on the GPU: every output over the 2n rows -- d_cand_start_out, the three candidate arrays up to
d_cand_start_out[2n], the rows' lengths, the status -- bit for bit the textbook's (tests/strand_textbook.py: seed_textbook.seed_batch on
the rows (T, Q), (T, rc(Q))), canaries of 16 entries behind every array and in the candidate arrays from d_cand_start_out[2n] on.

The sizes the kernel streams or sorts in (mgl_amd/csrc/sw_seed_strands.h, sw_seed.h): SEED_BLOCK = 1024 k-mer positions are sketched at
once -- the reverse row's from the read's far end --; an orientation's table leaves LDS above STRAND_LDS_TAB = 2048 entries and ends at
8192; a row's raw hits leave LDS above 2048 and end at max_cand <= 8192."""
import functools
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seed_cases as cases  # noqa: E402
import seed_textbook as tb  # noqa: E402
import strand_textbook as stb  # noqa: E402
from mgl_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

PAD = 16
NAMES = ("cand_start", "cand_t", "cand_q", "cand_len", "row_t_len", "row_q_len", "status")
STRAND_LDS_TAB = 2048
rc = stb.revcomp


@pytest.fixture(scope="module")
def aligner():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mgl_amd import smithwaterman as sw

    a = sw.MicrosoftSmithWaterman(0)
    assert a.load()
    yield a
    a.close()


def _pack(Ts, Qs):
    from mgl_amd.smithwaterman import _pack_pairs

    return _pack_pairs(Ts, Qs, torch.device("cuda", 0), None, False)


def _expected(Ts, Qs, params, merge, max_cand, capacity):
    """the textbook's arrays as the canaried arrays must look"""
    rT, rQ = stb.rows(Ts, Qs)
    want = cases.expected(rT, rQ, *params, merge, max_cand, capacity, PAD)
    lens = [np.full(2 * len(Ts) + PAD, cases.CANARY, np.int32) for _ in range(2)]
    lens[0][:2 * len(Ts)] = [len(T) for T in rT]
    lens[1][:2 * len(Ts)] = [len(Q) for Q in rQ]
    return want[:4] + lens + want[4:]


def _run(al, Ts, Qs, params, merge, max_cand, capacity, absent=(), fill=cases.CANARY):
    """one call into arrays that are CANARY everywhere and PAD entries longer than their capacity -> the whole arrays, as numpy;
    `absent`: the optional outputs (4, 5: the rows' lengths, 6: the status) passed as null"""
    dev = torch.device("cuda", 0)
    n, packed, _ = _pack(Ts, Qs)
    sizes = (2 * n + 1, capacity, capacity, capacity, 2 * n, 2 * n, 2 * n)
    full = [torch.full((size + PAD,), fill, dtype=torch.int64 if i == 0 else torch.int32, device=dev) for i, size in enumerate(sizes)]
    views = [None if i in absent else x[:size] for i, (x, size) in enumerate(zip(full, sizes))]
    try:
        al.seed_strands_device(*packed[:6], *params, merge, max_cand, capacity, out=tuple(views))
    finally:
        torch.cuda.synchronize()
    return [x.cpu().numpy() for x in full]


def _compare(got, want, absent=()):
    for i, name in enumerate(NAMES):
        if i in absent:
            assert (got[i] == cases.CANARY).all(), name  # a null output: nothing written for it
        else:
            bad = np.flatnonzero(got[i] != want[i])
            assert bad.size == 0, (name, bad[:8], got[i][bad[:8]], want[i][bad[:8]])


def _check(al, Ts, Qs, params, merge, max_cand, slack=5, absent=()):
    """the batch at a capacity `slack` above what it needs, against the textbook -> the expected arrays"""
    rT, rQ = stb.rows(Ts, Qs)
    total = tb.seed_batch(rT, rQ, *params, merge, max_cand, 1 << 30)[0][-1]
    want = _expected(Ts, Qs, params, merge, max_cand, total + slack)
    _compare(_run(al, Ts, Qs, params, merge, max_cand, total + slack, absent), want, absent)
    return want


def _framed(Ts, Qs):
    """refused and empty pairs at the front, in the middle and at the end"""
    m = len(Ts) // 2
    Ts = [b"", b"ACGTACGTAC"] + Ts[:m] + [b"ACGTTGCAACGTACGTTTGACA", b"AC"] + Ts[m:] + [b"NNNNNNNNNNNNNNNNNNNNNNNN", b"ACGT"]
    Qs = [b"ACGT", b"TTTTTTTTTT"] + Qs[:m] + [b"", b"AC"] + Qs[m:] + [b"NNNNNNNNNNNNNNNNNNNNNNNN", b""]
    return Ts, Qs


@functools.lru_cache(maxsize=None)
def _edge_batch(k, w):
    """windows that hold a piece of the read's forward strand AND a piece of its reverse strand, so that both rows find hits"""
    rng = np.random.default_rng(100 * k + w)
    Ts, Qs = [], []
    for alphabet in (b"AT", b"ACGT"):
        for _ in range(3):
            x = cases.rand_seq(rng, int(rng.integers(60, 160)), alphabet)
            Qs.append(x)
            Ts.append(cases.mutate(rng, x[:len(x) // 2 + k]) + rc(cases.mutate(rng, x[len(x) // 3:])))
        x = cases.rand_seq(rng, 90, alphabet)
        Qs.append(rc(x)), Ts.append(cases.mutate(rng, x))  # (a read of the other strand alone)
    base = cases.rand_seq(rng, 3 * (k + w) + 20)
    window = base + b"N" + rc(base)
    for n in (k - 1, k, k + w):  # reads around the shortest that have a k-mer, a window
        Qs.append(base[5:5 + n]), Ts.append(window)
        Qs.append(rc(base)[7:7 + n]), Ts.append(base)
    short = base[:2 * k + w + 3]
    for i in (0, len(short) // 2, len(short) - 1):  # a stray N at the read's first, middle and last byte; lower case
        Qs.append(short[:i] + b"N" + short[i + 1:]), Ts.append(window)
        Qs.append(short[:i] + short[i:i + 1].lower() + short[i + 1:]), Ts.append(window)
    Qs.append(short.lower()), Ts.append(window)
    Qs.append(base + rc(base)), Ts.append(window)  # a read equal to its own reverse complement: the two rows are equal
    return _framed(Ts, Qs)


@pytest.mark.parametrize("k", [4, 11, 15, 16])
def test_random_pairs_short_reads_stray_bytes_and_refused_pairs(aligner, k):
    seen = set()
    for w in (1, 10, 32):
        Ts, Qs = _edge_batch(k, w)
        n, packed, _ = _pack(Ts, Qs)
        for merge in (0, 1):
            want = _check(aligner, Ts, Qs, (k, w, 8), merge, 4096)
            seen |= set(want[6][:2 * n].tolist())
            # row 2p is what the one-strand entry gives for pair p
            one = [x.cpu().numpy() for x in aligner.seed_device(*packed[:6], k, w, 8, merge, 4096)]
            for p in range(n):
                a, b, c, d = want[0][2 * p], want[0][2 * p + 1], one[0][p], one[0][p + 1]
                assert b - a == d - c and want[6][2 * p] == one[4][p]
                assert all((want[i][a:b] == one[i][c:d]).all() for i in (1, 2, 3))
        per_row = np.diff(want[0][:2 * n + 1])
        assert per_row[0::2].sum() > 0 and per_row[1::2].sum() > 0  # (the batch has candidates on forward rows and on reverse rows)
        # every combination of the optional outputs null
        for absent in ((6,), (4, 5), (4,), (5, 6), (4, 5, 6)):
            _check(aligner, Ts, Qs, (k, w, 8), 1, 4096, absent=absent)
    assert seen == {0, _lib.ERR_BAD_ARG}


def test_palindromes_homopolymers_and_two_letter_reads(aligner):
    # k = 4: ACGT, CGTA, GTAC, TACG are their own reverse complements or each other's; the tie rule on the reverse row
    Ts = [b"ACGT" * 12, b"ACGT" * 9 + b"N" + b"TTTT" + b"ACGT" * 5, b"A" * 40 + b"T" * 40, b"T" * 50, b"AC" * 25 + b"GT" * 25, b"GT" * 30, b"AT" * 40,
          b"CG" * 31 + b"C"]
    Qs = [b"ACGT" * 10, b"CGTA" * 7 + b"C", b"A" * 37, b"A" * 37, b"CA" * 20 + b"C", b"AC" * 20, b"TA" * 33, b"GC" * 17]
    for k, w, occ in ((4, 1, 64), (4, 3, 64), (6, 4, 64), (6, 4, 8), (5, 32, 30)):
        for merge in (0, 1):
            _check(aligner, Ts, Qs, (k, w, occ), merge, 4096)


@functools.lru_cache(maxsize=None)
def _block_pairs():
    """k = 15: reads whose k-mer positions number SEED_BLOCK and twice that, +- 1, plain and with a stray byte a little behind the seam
    counted from the read's start and from its end (the reverse row's seam); windows of either strand"""
    rng = np.random.default_rng(41)
    Ts, Qs = [], []
    for nk in [m * cases.SEED_BLOCK + d for m in (1, 2) for d in (-1, 0, 1)]:
        Q = bytearray(cases.rand_seq(rng, nk + 14))
        Qs.append(bytes(Q)), Ts.append(rc(cases.mutate(rng, bytes(Q))))
        Q[cases.SEED_BLOCK + 3] = ord("N")
        Qs.append(bytes(Q)), Ts.append(cases.mutate(rng, bytes(Q))[:1500] + rc(bytes(Q))[200:])
        Q[len(Q) - 1 - (cases.SEED_BLOCK + 3)] = ord("n")
        Qs.append(bytes(Q)), Ts.append(rc(cases.mutate(rng, bytes(Q))))
    return Ts, Qs


@pytest.mark.parametrize("w", [1, 32])
def test_read_lengths_around_the_streamed_block_from_either_end(aligner, w):
    Ts, Qs = _block_pairs()
    for merge in (0, 1):
        want = _check(aligner, Ts, Qs, (15, w, 8), merge, 4096)
        assert (want[6][:2 * len(Ts)] == 0).all() and np.diff(want[0][:2 * len(Ts) + 1])[1::2].min() >= 1  # (every reverse row finds its window)


def test_sketch_sizes_around_the_sorts_the_lds_table_and_the_bound(aligner):
    # k = 12, w = 1: every position of an ACGT read is in either sketch, so a read of m + 11 bases sorts m entries per row
    rng = np.random.default_rng(42)
    long = cases.rand_seq(rng, 8192 + 12)
    sizes = [m + d for m in (256, STRAND_LDS_TAB, 4096, tb.MAX_QUERY_SEEDS) for d in (-1, 0, 1)]
    Qs = [long[:m + 11] for m in sizes]
    Ts = [Q[max(0, len(Q) - 150):][:120] + b"N" + rc(Q)[5:90] for Q in Qs]
    for merge in (0, 1):
        want = _check(aligner, Ts, Qs, (12, 1, 8), merge, 1024)
        assert want[6][:2 * len(Ts)].tolist() == [0] * (2 * len(Ts) - 2) + [_lib.ERR_UNSUPPORTED] * 2  # 8193 positions on both rows
        assert np.diff(want[0][:2 * len(Ts) - 1]).min() >= (40 if merge == 0 else 1)


def test_raw_hits_around_the_lds_buffer_and_at_max_cand_on_one_row_while_the_other_is_empty(aligner):
    # k = 4, w = 1, max_occ = 64: homopolymers of a and b positions have a * b raw hits on the row whose read is the window's letter and none
    # on the other: 2047, 2048, 2049 around the LDS buffer, 8192 = max_cand and 8193
    shapes = ((89, 23), (32, 64), (683, 3), (128, 64), (2731, 3))
    Ts = [b"A" * (a + 3) for a, _ in shapes] * 2
    Qs = [b"T" * (b + 3) for _, b in shapes] + [b"A" * (b + 3) for _, b in shapes]  # the reverse row's hits, then the forward row's
    unsupported = _lib.ERR_UNSUPPORTED
    for merge in (0, 1):
        want = _check(aligner, Ts, Qs, (4, 1, 64), merge, 8192)
        assert want[6][:20].tolist() == [0] * 9 + [unsupported] + [0] * 8 + [unsupported, 0]
        counts = np.diff(want[0][:21])
        assert merge or counts.tolist() == [0, 2047, 0, 2048, 0, 2049, 0, 8192, 0, 0, 2047, 0, 2048, 0, 2049, 0, 8192, 0, 0, 0]
        # max_cand = 2048: no hit leaves LDS, and the rows above it are refused
        want = _check(aligner, Ts, Qs, (4, 1, 64), merge, 2048)
        assert want[6][:10].tolist() == [0, 0, 0, 0] + [0, unsupported] * 3 and want[6][10:20].tolist() == [0, 0, 0, 0] + [unsupported, 0] * 3
    # both rows above the LDS buffer at once: a window of A and T runs, a read of A
    _check(aligner, [b"A" * 95 + b"T" * 95], [b"A" * 26], (4, 1, 64), 1, 8192)


def test_the_capacity_cut_before_between_and_behind_the_rows_of_a_pair(aligner):
    rng = np.random.default_rng(5)
    s = [cases.rand_seq(rng, 40) for _ in range(4)]
    Ts = [s[0] + b"N" + rc(s[0]), s[1], b"", s[2] + rc(s[2]), rc(s[3]), s[0] + b"N" + rc(s[0])]
    Qs = [s[0], s[3], s[0], s[2], s[3], s[0]]
    start = stb.seed_strands_batch(Ts, Qs, 8, 1, 8, 1, 256, 1 << 30)[0]
    counts = np.diff(start)
    assert counts[0] > 0 and counts[1] > 0 and counts[6] > 0 and counts[7] > 0
    seen = set()
    for cap in sorted({0, start[1] - 1, start[1], start[2] - 1, start[2], start[7] - 1, start[7], start[8] - 1, start[8], start[-1] - 1, start[-1], 400}):
        want = _expected(Ts, Qs, (8, 1, 8), 1, 256, int(cap))
        seen.add(tuple(want[6][:12].tolist()))
        _compare(_run(aligner, Ts, Qs, (8, 1, 8), 1, 256, int(cap)), want)
        _compare(_run(aligner, Ts, Qs, (8, 1, 8), 1, 256, int(cap), absent=(6,)), want, absent=(6,))
    assert len(seen) >= 6 and any(x[6] == 0 and x[7] == _lib.ERR_NOMEM for x in seen)  # (a cut between the two rows of pair 3)
    # more rows than the scan takes in one step, the cut in its second step
    Ts, Qs = [s[0] + rc(s[0]), s[1] + s[2]] * 290, [s[0], s[2] + b"N" + s[1]] * 290
    start = stb.seed_strands_batch(Ts, Qs, 8, 1, 8, 1, 256, 1 << 30)[0]
    for cap in (start[1101] - 1, start[1101]):
        _compare(_run(aligner, Ts, Qs, (8, 1, 8), 1, 256, int(cap)), _expected(Ts, Qs, (8, 1, 8), 1, 256, int(cap)))


def test_a_workspace_that_holds_one_slot_and_one_that_holds_none(aligner):
    from mgl_amd import smithwaterman as sw

    small = sw.MicrosoftSmithWaterman(0)
    try:
        small.set_workspace(1 << 20)
        Ts, Qs = _block_pairs()
        # 36 pairs at max_cand = 1024: 512 + 72 * 12 288 bytes of staging leave 163 328 of one MiB, one slot of 2 * 65 536: one workgroup
        # works all pairs off.  The sketch of a read of 24 000 bases has more than 4096 entries: both tables live in that slot
        long = cases.rand_seq(np.random.default_rng(45), 24000)
        assert len(tb.sketch(long, 15, 10)) > 4096 and len(tb.sketch(rc(long), 15, 10)) > 4096
        Ts36, Qs36 = (Ts * 2)[:35] + [long[100:300] + rc(long)[4000:4200]], (Qs * 2)[:35] + [long]
        want = _check(small, Ts36, Qs36, (15, 10, 8), 1, 1024)
        assert (want[6][:72] == 0).all() and want[0][71] - want[0][70] >= 1 and want[0][72] - want[0][71] >= 1
        _compare(_run(aligner, Ts36, Qs36, (15, 10, 8), 1, 1024, int(want[0][72]) + 5), want)  # the default workspace: a slot per workgroup
        # 40 pairs: 512 + 80 * 12 288 leave 65 024, less than a slot
        Ts40, Qs40 = (Ts * 3)[:40], (Qs * 3)[:40]
        with pytest.raises(_lib.MglSwError) as e:
            got = _run(small, Ts40, Qs40, (15, 10, 8), 1, 1024, 4096, fill=7)
        assert e.value.status == _lib.ERR_NOMEM
        n, packed, _ = _pack(Ts40, Qs40)
        dev = torch.device("cuda", 0)
        out = (torch.full((2 * n + 1,), 7, dtype=torch.int64, device=dev),) + tuple(torch.full((m,), 7, dtype=torch.int32, device=dev)
                                                                                     for m in (4096, 4096, 4096, 2 * n, 2 * n, 2 * n))
        with pytest.raises(_lib.MglSwError):
            small.seed_strands_device(*packed[:6], 15, 10, 8, True, 1024, out=out)
        torch.cuda.synchronize()
        assert all(bool((x == 7).all()) for x in out)  # not one entry was written
        _check(small, Ts40, Qs40, (15, 10, 8), 1, 512)  # (half the staging: it fits)
    finally:
        small.close()


def test_seed_strands_over_lists_and_an_empty_batch(aligner):
    Ts, Qs = _block_pairs()
    res = aligner.seed_strands(Ts[:2] + [b""], Qs[:2] + [b"ACGT"])
    assert res.status.tolist() == [0, 0, 0, 0, _lib.ERR_BAD_ARG, _lib.ERR_BAD_ARG]
    want = [tb.seed_pair(T, Q, 15, 10, 8, 1, 4096).cands for T, Q in zip(*stb.rows(Ts[:2], Qs[:2]))]
    assert res.candidates == want + [[], []] and len(want[1]) > 5 and len(want[2]) > 5  # (a reverse row and a forward row that find their window)
    got = _run(aligner, [], [], (15, 10, 8), 1, 64, 8)
    assert got[0][0] == 0 and all((x == cases.CANARY).all() for x in [got[0][1:]] + got[1:])
