"""mgl_sw_seed_index_batch_device on the GPU: every output over the strands * n rows -- d_cand_start_out, the three candidate arrays up
to d_cand_start_out[rows], the rows' lengths, the status -- bit for bit the textbook's (tests/index_textbook.py: seed_index_batch),
canaries of 16 entries behind every array and in the candidate arrays from d_cand_start_out[rows] on.

The sizes the kernel streams or sorts in (mgl_amd/csrc/sw_index.hip, sw_seed.h): SEED_BLOCK = 1024 k-mer positions are sketched at once;
a row's table leaves LDS above SEED_LDS_TAB = 4096 entries and ends at 8192; a row's raw hits leave LDS above 2048 and end at
max_cand <= 8192; sw_seed_scan_kernel sums 1024 rows a step."""
import functools
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import index_textbook as itb  # noqa: E402
import seed_cases as cases  # noqa: E402
import seed_textbook as tb  # noqa: E402
import strand_textbook as stb  # noqa: E402
from mgl_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

PAD = 16
NAMES = ("cand_start", "cand_t", "cand_q", "cand_len", "row_t_len", "row_q_len", "status")
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


class Ref:
    """a reference with its index on the device and the textbook's"""

    def __init__(self, al, R, k, w):
        self.R, self.k, self.w = R, k, w
        self.table = itb.by_key(itb.build_index(R, k, w))
        self.index = al.build_index(R, k, w)

    def close(self):
        self.index.close()


def _pack(Qs):
    from mgl_amd.smithwaterman import _pack_pairs

    return _pack_pairs(Qs, Qs, torch.device("cuda", 0), None, False)


def _arrays(batch, rows, capacity):
    """a textbook batch as the canaried arrays must look"""
    start, ct, cq, cl, status, rt, rq = batch
    sizes = (rows + 1, capacity, capacity, capacity, rows, rows, rows)
    want = [np.full(size + PAD, cases.CANARY, np.int64 if i == 0 else np.int32) for i, size in enumerate(sizes)]
    for arr, vals in zip(want, (start, ct, cq, cl, rt, rq, status)):
        arr[:len(vals)] = vals
    return want


def _expected(ref, Qs, strands, occ, merge, max_cand, capacity):
    return _arrays(itb.seed_index_batch(ref.table, len(ref.R), Qs, ref.k, ref.w, strands, *occ, merge, max_cand, capacity), strands * len(Qs), capacity)


def _run(al, ref, Qs, strands, occ, merge, max_cand, capacity, absent=(), fill=cases.CANARY):
    """one call into arrays that are CANARY everywhere and PAD entries longer than their capacity -> the whole arrays, as numpy;
    `absent`: the optional outputs (4, 5: the rows' lengths, 6: the status) passed as null"""
    dev = torch.device("cuda", 0)
    n, packed, _ = _pack(Qs)
    rows = strands * n
    sizes = (rows + 1, capacity, capacity, capacity, rows, rows, rows)
    full = [torch.full((size + PAD,), fill, dtype=torch.int64 if i == 0 else torch.int32, device=dev) for i, size in enumerate(sizes)]
    views = [None if i in absent else x[:size] for i, (x, size) in enumerate(zip(full, sizes))]
    try:
        al.seed_index_device(ref.index, *packed[3:6], strands, *occ, merge, max_cand, capacity, out=tuple(views))
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


def _check(al, ref, Qs, strands, occ, merge, max_cand, slack=5, absent=()):
    """the batch at a capacity `slack` above what it needs (the textbook at any capacity that holds it is the same), against the
    textbook -> the expected arrays"""
    batch = itb.seed_index_batch(ref.table, len(ref.R), Qs, ref.k, ref.w, strands, *occ, merge, max_cand, 1 << 30)
    want = _arrays(batch, strands * len(Qs), batch[0][-1] + slack)
    _compare(_run(al, ref, Qs, strands, occ, merge, max_cand, batch[0][-1] + slack, absent), want, absent)
    return want


@functools.lru_cache(maxsize=None)
def _edge_batch(k, w):
    """a reference of pieces, and reads of either strand of them: short ones, stray bytes, lower case, an absent one, refused ones"""
    rng = np.random.default_rng(100 * k + w)
    segs = [cases.rand_seq(rng, int(rng.integers(120, 200)), alphabet) for alphabet in (b"ACGT", b"ACGT", b"ACGT", b"AT")]
    base = cases.rand_seq(rng, 3 * (k + w) + 20)
    R = b"N".join(segs + [base, rc(segs[0][:60])])
    Qs = [b""]
    for x in segs:
        Qs += [cases.mutate(rng, x[:len(x) // 2 + k]), rc(cases.mutate(rng, x[len(x) // 3:])), x[:70] + rc(x[60:])]
    Qs.append(cases.rand_seq(rng, 150, b"CG"))  # absent from the reference (but by chance at small k)
    Qs.append(b"")
    for n in (k - 1, k, k + w):  # reads around the shortest that have a k-mer, a window
        Qs += [base[5:5 + n], rc(base)[7:7 + n]]
    short = base[:2 * k + w + 3]
    for i in (0, len(short) // 2, len(short) - 1):  # a stray N at the read's first, middle and last byte; lower case
        Qs += [short[:i] + b"N" + short[i + 1:], short[:i] + short[i:i + 1].lower() + short[i + 1:]]
    Qs += [short.lower(), base + rc(base), b"N" * 40, b""]
    return R, Qs


@pytest.mark.parametrize("k", [4, 11, 15, 16])
def test_parameter_grid_short_reads_stray_bytes_and_refused_reads_on_one_and_two_strands(aligner, k):
    seen = set()
    for w in (1, 10, 32):
        R, Qs = _edge_batch(k, w)
        ref = Ref(aligner, R, k, w)
        try:
            n = len(Qs)
            for merge in (0, 1):
                two = _check(aligner, ref, Qs, 2, (8, 64), merge, 4096)
                one = _check(aligner, ref, Qs, 1, (8, 64), merge, 4096)
                seen |= set(two[6][:2 * n].tolist())
                for p in range(n):  # row 2p of two strands is row p of one
                    a, b, c, d = two[0][2 * p], two[0][2 * p + 1], one[0][p], one[0][p + 1]
                    assert b - a == d - c and two[6][2 * p] == one[6][p]
                    assert all((two[i][a:b] == one[i][c:d]).all() for i in (1, 2, 3))
            per_row = np.diff(two[0][:2 * n + 1])
            assert per_row[0::2].sum() > 0 and per_row[1::2].sum() > 0  # (candidates on forward rows and on reverse rows)
            for absent in ((6,), (4, 5), (4,), (5, 6), (4, 5, 6)):  # every combination of the optional outputs null
                _check(aligner, ref, Qs, 2, (8, 64), 1, 4096, absent=absent)
            _check(aligner, ref, Qs, 1, (3, 2), 1, 4096, absent=(5,))
        finally:
            ref.close()
    assert {0, _lib.ERR_BAD_ARG} <= seen


def test_reads_against_an_index_without_entries(aligner):
    ref = Ref(aligner, b"N" * 500 + b"acgt" * 50, 11, 5)
    try:
        assert ref.index.info.entries == 0
        want = _check(aligner, ref, [b"ACGTTGCAAGCTTGACCAGT" * 5, b"", b"ACGT"], 2, (8, 64), 1, 256)
        assert want[0][:7].tolist() == [0] * 7 and want[6][:6].tolist() == [0, 0, 1, 1, 0, 0]
    finally:
        ref.close()


def test_occurrences_at_and_above_either_cap(aligner):
    rng = np.random.default_rng(3)
    kmer = b"ACGTTGCAAGC"
    pad = lambda: cases.rand_seq(rng, 9, b"CT")  # noqa: E731
    R = b"".join(pad() + kmer for _ in range(5)) + pad() + rc(kmer) + pad()
    Q = pad() + kmer + pad()
    Q2 = pad() + kmer + pad() + kmer
    ref = Ref(aligner, R, len(kmer), 1)
    try:
        assert len(ref.table[tb.kmers(kmer, 11)[0]]) == 5
        counts = {}
        for occ in ((8, 5), (8, 4), (2, 5), (1, 5), (1, 1), (64, 8192)):
            for merge in (0, 1):
                want = _check(aligner, ref, [Q, Q2, rc(Q2)], 2, occ, merge, 4096)
                counts[occ, merge] = np.diff(want[0][:7]).tolist()
        assert counts[(8, 5), 0][0] >= counts[(8, 4), 0][0] + 5    # the key five times in the index: kept at 5, dropped at 4
        assert counts[(2, 5), 0][2] >= counts[(1, 5), 0][2] + 10  # twice in the read: kept at 2, dropped at 1
        assert counts[(2, 5), 0][5] == counts[(2, 5), 0][2]        # (the reverse row of the reverse read is the read)
    finally:
        ref.close()


def test_raw_hits_around_the_lds_buffer_and_at_max_cand(aligner):
    # k = 4, w = 1: a reference of a A-positions and a read of b have a * b raw hits on the row that reads A and none on the other: 2047,
    # 2048, 2049 around the LDS buffer, 8192 = max_cand and 8193
    unsupported = _lib.ERR_UNSUPPORTED
    for (a, b), status in zip(((89, 23), (32, 64), (683, 3), (128, 64), (2731, 3)), (0, 0, 0, 0, unsupported)):
        ref = Ref(aligner, b"A" * (a + 3), 4, 1)
        try:
            Qs = [b"A" * (b + 3), b"T" * (b + 3)]
            for merge in (0, 1):
                want = _check(aligner, ref, Qs, 2, (64, 8192), merge, 8192)
                assert want[6][:4].tolist() == [status, 0, 0, status]
                assert merge or np.diff(want[0][:5]).tolist() == ([a * b, 0, 0, a * b] if not status else [0] * 4)
                want = _check(aligner, ref, Qs, 2, (64, 8192), merge, 2048)  # no hit leaves LDS, and the rows above it are refused
                assert want[6][:4].tolist() == [unsupported if a * b > 2048 else 0, 0, 0, unsupported if a * b > 2048 else 0]
            # the reference's cap at and below the A-positions, the read's at and below its own
            assert np.diff(_check(aligner, ref, Qs, 1, (64, a), 0, 8192)[0][:3]).tolist() == [a * b if not status else 0, 0]
            assert np.diff(_check(aligner, ref, Qs, 1, (64, a - 1), 0, 8192)[0][:3]).tolist() == [0, 0]
            assert np.diff(_check(aligner, ref, Qs, 1, (b - 1, 8192), 0, 8192)[0][:3]).tolist() == [0, 0]
        finally:
            ref.close()


def test_sketch_sizes_around_the_sorts_the_lds_table_and_the_bound(aligner):
    # k = 12, w = 1: every position of an ACGT read is in its sketch, so a read of m + 11 bases sorts m entries per row
    rng = np.random.default_rng(42)
    long = cases.rand_seq(rng, 8192 + 12)
    sizes = [m + d for m in (256, 2048, cases.SEED_LDS_TAB, tb.MAX_QUERY_SEEDS) for d in (-1, 0, 1)]
    Qs = [long[:m + 11] for m in sizes]
    ref = Ref(aligner, long[100:220] + b"N" + rc(long[30:130]) + b"N" + long[4000:4100], 12, 1)
    try:
        for merge in (0, 1):
            want = _check(aligner, ref, Qs, 2, (8, 64), merge, 1024)
            assert want[6][:2 * len(Qs)].tolist() == [0] * (2 * len(Qs) - 2) + [_lib.ERR_UNSUPPORTED] * 2  # 8193 positions on both rows
            assert np.diff(want[0][:2 * len(Qs) - 1]).min() >= (80 if merge == 0 else 1)
    finally:
        ref.close()


@functools.lru_cache(maxsize=None)
def _block_reads():
    """k = 15: reads whose k-mer positions number SEED_BLOCK and twice that, +- 1, plain and with a stray byte a little behind the seam
    counted from the read's start and from its end (the reverse row's seam), and the reference they come from"""
    rng = np.random.default_rng(41)
    R = cases.rand_seq(rng, 9000)
    Qs = []
    for i, nk in enumerate([m * cases.SEED_BLOCK + d for m in (1, 2) for d in (-1, 0, 1)]):
        Q = bytearray(cases.mutate(rng, R[1000 * i:1000 * i + nk + 40])[:nk + 14])
        Qs.append(bytes(Q) if i % 2 else rc(bytes(Q)))
        Q[cases.SEED_BLOCK + 3] = ord("N")
        Qs.append(bytes(Q))
        Q[len(Q) - 1 - (cases.SEED_BLOCK + 3)] = ord("n")
        Qs.append(rc(bytes(Q)))
    return R, Qs


@pytest.mark.parametrize("w", [1, 32])
def test_read_lengths_around_the_streamed_block_from_either_end(aligner, w):
    R, Qs = _block_reads()
    ref = Ref(aligner, R, 15, w)
    try:
        for merge in (0, 1):
            want = _check(aligner, ref, Qs, 2, (8, 64), merge, 4096)
            counts = np.diff(want[0][:2 * len(Qs) + 1]).reshape(-1, 2)
            assert (want[6][:2 * len(Qs)] == 0).all() and (counts.max(axis=1) >= 5).all()  # (every read finds its place on one of its rows)
    finally:
        ref.close()


def test_the_capacity_cut_before_between_and_behind_the_rows_of_a_read(aligner):
    rng = np.random.default_rng(5)
    s = [cases.rand_seq(rng, 40) for _ in range(4)]
    ref = Ref(aligner, s[0] + b"N" + rc(s[0]) + b"N" + s[1] + b"N" + s[2] + b"N" + rc(s[2]), 8, 1)
    try:
        Qs = [s[0], s[3], b"", s[2], rc(s[1]), s[0]]
        start = itb.seed_index_batch(ref.table, len(ref.R), Qs, 8, 1, 2, 8, 64, 1, 256, 1 << 30)[0]
        counts = np.diff(start)
        assert counts[0] > 0 and counts[1] > 0 and counts[6] > 0 and counts[7] > 0 and counts[9] > 0
        seen = set()
        for cap in sorted({0, start[1] - 1, start[1], start[2] - 1, start[2], start[7] - 1, start[7], start[8] - 1, start[8], start[-1] - 1, start[-1], 400}):
            want = _expected(ref, Qs, 2, (8, 64), 1, 256, int(cap))
            seen.add(tuple(want[6][:12].tolist()))
            _compare(_run(aligner, ref, Qs, 2, (8, 64), 1, 256, int(cap)), want)
            _compare(_run(aligner, ref, Qs, 2, (8, 64), 1, 256, int(cap), absent=(6,)), want, absent=(6,))
        assert len(seen) >= 6 and any(x[6] == 0 and x[7] == _lib.ERR_NOMEM for x in seen)  # (a cut between the two rows of read 3)
        # more rows than the scan takes in one step, the cut in its second step; one strand and two
        Qs = [s[0], s[2] + b"N" + s[1]] * 290
        start = itb.seed_index_batch(ref.table, len(ref.R), Qs, 8, 1, 2, 8, 64, 1, 256, 1 << 30)[0]
        for cap in (start[1101] - 1, start[1101]):
            _compare(_run(aligner, ref, Qs, 2, (8, 64), 1, 256, int(cap)), _expected(ref, Qs, 2, (8, 64), 1, 256, int(cap)))
        Qs = Qs * 2
        start = itb.seed_index_batch(ref.table, len(ref.R), Qs, 8, 1, 1, 8, 64, 1, 256, 1 << 30)[0]
        _compare(_run(aligner, ref, Qs, 1, (8, 64), 1, 256, int(start[1101]) - 1), _expected(ref, Qs, 1, (8, 64), 1, 256, int(start[1101]) - 1))
    finally:
        ref.close()


def test_a_workspace_that_holds_one_slot_and_one_that_holds_none(aligner):
    from mgl_amd import smithwaterman as sw

    small = sw.MicrosoftSmithWaterman(0)
    R, Qs = _block_reads()
    long = cases.rand_seq(np.random.default_rng(45), 24000)
    assert len(tb.sketch(long, 15, 10)) > 4096 and len(tb.sketch(rc(long), 15, 10)) > 4096
    R = R + b"N" + long[100:300] + rc(long)[4000:4200]
    ref = Ref(small, R, 15, 10)  # (an index serves every context of its device)
    try:
        small.set_workspace(1 << 20)
        # 39 reads at max_cand = 1024: 512 + 78 * 12 288 bytes of staging leave 89 600 of one MiB, one slot of 65 536: one workgroup works
        # all reads off.  The sketch of a read of 24 000 bases has more than 4096 entries: its table lives in that slot
        Qs39 = (Qs * 3)[:38] + [long]
        want = _check(small, ref, Qs39, 2, (8, 64), 1, 1024)
        assert (want[6][:78] == 0).all() and want[0][77] - want[0][76] >= 1 and want[0][78] - want[0][77] >= 1
        _compare(_run(aligner, ref, Qs39, 2, (8, 64), 1, 1024, int(want[0][78]) + 5), want)  # the default workspace: a slot per workgroup
        # 40 reads: 512 + 80 * 12 288 leave 65 024, less than a slot
        Qs40 = (Qs * 3)[:40]
        n, packed, _ = _pack(Qs40)
        dev = torch.device("cuda", 0)
        out = (torch.full((2 * n + 1,), 7, dtype=torch.int64, device=dev),) + tuple(torch.full((m,), 7, dtype=torch.int32, device=dev)
                                                                                     for m in (4096, 4096, 4096, 2 * n, 2 * n, 2 * n))
        with pytest.raises(_lib.MglSwError) as e:
            small.seed_index_device(ref.index, *packed[3:6], 2, 8, 64, True, 1024, out=out)
        assert e.value.status == _lib.ERR_NOMEM
        torch.cuda.synchronize()
        assert all(bool((x == 7).all()) for x in out)  # not one entry was written
        _check(small, ref, Qs40, 2, (8, 64), 1, 512)  # (half the staging: it fits)
        _check(small, ref, Qs40, 1, (8, 64), 1, 1024)  # (half the rows: it fits)
    finally:
        ref.close()
        small.close()


def test_seed_index_over_lists_and_an_empty_batch(aligner):
    R, Qs = _block_reads()
    ref = Ref(aligner, R, 15, 10)
    try:
        res = aligner.seed_index(ref.index, Qs[:2] + [b""], max_cand=4096)
        assert res.status.tolist() == [0, 0, 0, 0, _lib.ERR_BAD_ARG, _lib.ERR_BAD_ARG]
        want = [itb.seed_index_row(ref.table, len(R), Q, 15, 10, 8, 64, 1, 4096).cands for Q in stb.rows(Qs[:2], Qs[:2])[1]]
        assert res.candidates == want + [[], []] and len(want[1]) > 5 and len(want[2]) > 5  # (a reverse row and a forward row that find their place)
        one = aligner.seed_index(ref.index, Qs[:2], strands=1)
        assert one.candidates == [want[0], want[2]]
        for strands in (1, 2):
            got = _run(aligner, ref, [], strands, (8, 64), 1, 64, 8)
            assert got[0][0] == 0 and all((x == cases.CANARY).all() for x in [got[0][1:]] + got[1:])
    finally:
        ref.close()
