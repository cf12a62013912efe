"""mgl_sw_seed_batch_device on the GPU: every output -- d_cand_start_out, the three candidate arrays up to d_cand_start_out[n], the
status -- bit for bit the textbook's (tests/seed_textbook.py), canaries of 16 entries behind every array and in the candidate arrays from
d_cand_start_out[n] on; and reads -> seeds -> chain -> alignment on one stream against the textbook's candidates uploaded from the host.

The sizes the kernel streams or sorts in, named in tests/seed_cases.py: SEED_BLOCK = 1024 k-mer positions are sketched at once; the
query's table is bitonic-sorted padded to a power of two and leaves LDS above SEED_LDS_TAB = 4096 entries; the raw hits leave LDS above
SEED_LDS_HITS = 2048; a query's sketch ends at 8192 positions and a pair's raw hits at max_cand <= 8192."""
import functools
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seed_cases as cases  # noqa: E402
import seed_textbook as tb  # noqa: E402
from mgl_amd import _lib, synth  # noqa: E402

pytestmark = pytest.mark.gpu

PAD = 16
NAMES = ("cand_start", "cand_t", "cand_q", "cand_len", "status")
GATK = (200, -150, 260, 11)
CHAINING = dict(max_pred=64, max_dist=1000, bw=500, pen_gap=38, pen_skip=0)  # DESIGN 9g's


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


def _run(al, Ts, Qs, params, merge, max_cand, capacity, status=True, fill=cases.CANARY):
    """one call into arrays that are CANARY everywhere and PAD entries longer than their capacity -> the whole arrays, as numpy"""
    dev = torch.device("cuda", 0)
    n, packed, _ = _pack(Ts, Qs)
    sizes = (n + 1, capacity, capacity, capacity, n)
    full = [torch.full((size + PAD,), fill, dtype=torch.int64 if i == 0 else torch.int32, device=dev) for i, size in enumerate(sizes)]
    views = [None if not status and i == 4 else x[:size] for i, (x, size) in enumerate(zip(full, sizes))]
    try:
        al.seed_device(*packed[:6], *params, merge, max_cand, capacity, out=tuple(views))
    finally:
        torch.cuda.synchronize()
    return [x.cpu().numpy() for x in full]


def _compare(got, want, skip=()):
    for i, name in enumerate(NAMES):
        if i not in skip:
            bad = np.flatnonzero(got[i] != want[i])
            assert bad.size == 0, (name, bad[:8], got[i][bad[:8]], want[i][bad[:8]])


def _check(al, Ts, Qs, params, merge, max_cand, slack=5, status=True):
    """the batch at a capacity `slack` above what it needs, against the textbook -> the expected arrays"""
    total = tb.seed_batch(Ts, Qs, *params, merge, max_cand, 1 << 30)[0][-1]
    want = cases.expected(Ts, Qs, *params, merge, max_cand, total + slack, PAD)
    got = _run(al, Ts, Qs, params, merge, max_cand, total + slack, status)
    if status:
        _compare(got, want)
    else:
        _compare(got, want, skip=(4,))
        assert (got[4] == cases.CANARY).all()
    return want


def _framed(group):
    """a parameter set's cases with refused and empty pairs at the front, in the middle and at the end"""
    Ts, Qs = [T for _, T, _ in group], [Q for _, _, Q in group]
    m = len(Ts) // 2
    Ts = [b"", b"ACGTACGTAC"] + Ts[:m] + [b"ACGTTGCAACGTACGTTTGACA", b"AC"] + Ts[m:] + [b"NNNNNNNNNNNNNNNNNNNNNNNN", b"ACGT"]
    Qs = [b"ACGT", b"TTTTTTTTTT"] + Qs[:m] + [b"", b"AC"] + Qs[m:] + [b"NNNNNNNNNNNNNNNNNNNNNNNN", b""]
    return Ts, Qs


def test_the_case_list_with_refused_and_empty_pairs_around_it(aligner):
    groups = cases.by_params(cases.edge_cases() + cases.random_cases())
    assert len(groups) > 50
    seen = set()
    for params, group in groups.items():
        Ts, Qs = _framed(group)
        for merge in (0, 1):
            want = _check(aligner, Ts, Qs, params, merge, 4096)
            seen |= set(want[4][:len(Ts)].tolist())
        _check(aligner, Ts, Qs, params, 1, 4096, status=False)  # d_status_out null: the rest is the same, nothing written for it
    assert seen == {0, _lib.ERR_BAD_ARG}


@functools.lru_cache(maxsize=None)
def _block_pairs():
    """k = 15, w = 10: windows and reads whose k-mer positions number SEED_BLOCK and twice that, +- 1, some with a stray byte at the seam"""
    rng = np.random.default_rng(31)
    Ts, Qs = [], []
    for nk in [m * cases.SEED_BLOCK + d for m in (1, 2) for d in (-1, 0, 1)]:
        T = bytearray(cases.rand_seq(rng, nk + 14))
        Ts.append(bytes(T)), Qs.append(cases.mutate(rng, bytes(T)))
        T[cases.SEED_BLOCK + 3] = ord("N")
        Ts.append(cases.mutate(rng, bytes(T))), Qs.append(bytes(T))  # (the read's length at the edge, the window's beside it)
    return Ts, Qs


def test_lengths_around_the_streamed_block(aligner):
    Ts, Qs = _block_pairs()
    for merge in (0, 1):
        want = _check(aligner, Ts, Qs, (15, 10, 8), merge, 1024)
        assert (want[4][:len(Ts)] == 0).all() and np.diff(want[0][:len(Ts) + 1]).min() > 5
    # w = 32 and w = 1 across the seams of the blocks; a repeat that many windows tie on
    _check(aligner, Ts[:4] + [b"AC" * 1100, b"A" * 2100], Qs[:4] + [b"CA" * 1050, b"A" * 1030], (11, 32, 64), 1, 8192)
    _check(aligner, Ts[:2], Qs[:2], (15, 1, 8), 1, 2048)


def test_sketch_sizes_around_the_sorts_the_lds_table_and_the_bound(aligner):
    # k = 12, w = 1: every position of an ACGT read is in its sketch, so a read of m + 11 bases sorts m entries
    rng = np.random.default_rng(32)
    long = cases.rand_seq(rng, 8192 + 12)
    sizes = [m + d for m in cases.SORT_SIZES + (cases.SEED_LDS_TAB, tb.MAX_QUERY_SEEDS) for d in (-1, 0, 1)]
    Qs = [long[:m + 11] for m in sizes]
    Ts = [Q[max(0, len(Q) - 150):][:120] + b"N" + Q[5:90] for Q in Qs]
    for merge in (0, 1):
        want = _check(aligner, Ts, Qs, (12, 1, 8), merge, 1024)
        assert want[4][:len(Ts)].tolist() == [0] * (len(Ts) - 1) + [_lib.ERR_UNSUPPORTED]  # 8193 positions
        assert np.diff(want[0][:len(Ts)]).min() >= (40 if merge == 0 else 2)


@functools.lru_cache(maxsize=None)
def _hit_pairs():
    """k = 4, w = 1, max_occ = 64.  Homopolymers of a and b positions have a * b raw hits on a + b - 1 diagonals: 2047, 2048, 2049 around
    SEED_LDS_HITS, 8192 = max_cand and 8193; and two-letter reads of a few hundred bases with thousands of hits"""
    rng = np.random.default_rng(33)
    Ts = [b"A" * (a + 3) for a in (89, 32, 683, 128, 2731)] + [cases.rand_seq(rng, 300, b"AC"), cases.rand_seq(rng, 330, b"GT"), b"ACGTTGCA"]
    Qs = [b"A" * (b + 3) for b in (23, 64, 3, 64, 3)] + [cases.rand_seq(rng, 300, b"AC"), cases.rand_seq(rng, 350, b"GT"), b"ACGTTGCA"]
    return Ts, Qs


def test_raw_hits_around_the_lds_buffer_and_at_max_cand(aligner):
    Ts, Qs = _hit_pairs()
    raw = [len(tb.seed_pair(T, Q, 4, 1, 64, 0, 8192).raw) for T, Q in zip(Ts[:4], Qs[:4])]
    assert raw == [2047, 2048, 2049, 8192]
    for merge in (0, 1):
        want = _check(aligner, Ts, Qs, (4, 1, 64), merge, 8192)
        assert want[4][:8].tolist() == [0, 0, 0, 0, _lib.ERR_UNSUPPORTED, 0, 0, 0]
        # max_cand = 2048: no hit leaves LDS, and the pairs above it are refused
        want = _check(aligner, Ts, Qs, (4, 1, 64), merge, 2048)
        assert want[4][:5].tolist() == [0, 0] + [_lib.ERR_UNSUPPORTED] * 3


def test_the_capacity_rule(aligner):
    rng = np.random.default_rng(4)
    s = [cases.rand_seq(rng, 40) for _ in range(4)]
    Ts = [s[0] + b"N" + s[1], s[2], b"", s[3], s[0], s[1], b"", s[2]]
    Qs = [s[0] + s[1], s[3], s[0], s[3], s[1], s[1], s[1], s[0]]
    for cap, status in ((4, [0, 0, 1, 0, 0, 0, 1, 0]), (3, [0, 0, 1, 0, 0, 3, 1, 3]), (2, [0, 0, 1, 3, 3, 3, 1, 3]), (0, [3, 3, 1, 3, 3, 3, 1, 3]), (40, None)):
        want = cases.expected(Ts, Qs, 8, 1, 8, 1, 256, cap, PAD)
        assert status is None or want[4][:8].tolist() == status
        _compare(_run(aligner, Ts, Qs, (8, 1, 8), 1, 256, cap), want)
        _compare(_run(aligner, Ts, Qs, (8, 1, 8), 1, 256, cap, status=False), want, skip=(4,))
    # more pairs than the scan takes in one step, the cut in its second step
    Ts, Qs = [s[0], s[1] + s[2]] * 560, [s[0], s[2] + b"N" + s[1]] * 560
    for cap in (3 * 530, 3 * 530 + 2):
        _compare(_run(aligner, Ts, Qs, (8, 1, 8), 1, 256, cap), cases.expected(Ts, Qs, 8, 1, 8, 1, 256, cap, PAD))


def test_a_workspace_that_holds_one_slot_and_one_that_holds_none(aligner):
    from mgl_amd import smithwaterman as sw

    small = sw.MicrosoftSmithWaterman(0)
    try:
        small.set_workspace(1 << 20)
        Ts, Qs = _block_pairs()
        # 75 pairs at max_cand = 1024: 512 + 3 * 307 200 bytes of staging leave 126 464 of one MiB, one slot of 65 536: one workgroup works
        # all pairs off.  The sketch of a read of 24 000 bases has more than SEED_LDS_TAB entries: its table lives in that slot
        long = cases.rand_seq(np.random.default_rng(35), 24000)
        assert len(tb.sketch(long, 15, 10)) > cases.SEED_LDS_TAB
        Ts75, Qs75 = (Ts * 7)[:74] + [long[100:300]], (Qs * 7)[:74] + [long]
        want = _check(small, Ts75, Qs75, (15, 10, 8), 1, 1024)
        assert (want[4][:75] == 0).all() and want[0][75] - want[0][74] >= 1
        _check(aligner, Ts75, Qs75, (15, 10, 8), 1, 1024)  # the default workspace: a slot per workgroup
        # 80 pairs: 512 + 3 * 327 680 leave 65 024, less than a slot
        Ts80, Qs80 = (Ts * 7)[:80], (Qs * 7)[:80]
        with pytest.raises(_lib.MglSwError) as e:
            _run(small, Ts80, Qs80, (15, 10, 8), 1, 1024, 4096, fill=7)
        assert e.value.status == _lib.ERR_NOMEM
        n, packed, _ = _pack(Ts80, Qs80)
        dev = torch.device("cuda", 0)
        out = (torch.full((n + 1,), 7, dtype=torch.int64, device=dev),) + tuple(torch.full((m,), 7, dtype=torch.int32, device=dev) for m in (4096, 4096, 4096, n))
        with pytest.raises(_lib.MglSwError):
            small.seed_device(*packed[:6], 15, 10, 8, True, 1024, out=out)
        torch.cuda.synchronize()
        assert all(bool((x == 7).all()) for x in out)  # not one entry was written
        _check(small, Ts80, Qs80, (15, 10, 8), 1, 512)  # (half the staging: it fits)
    finally:
        small.close()


def test_seed_over_lists(aligner):
    Ts, Qs = _block_pairs()
    res = aligner.seed(Ts[:3] + [b""], Qs[:3] + [b"ACGT"])
    assert res.status.tolist() == [0, 0, 0, _lib.ERR_BAD_ARG]
    assert res.candidates == [tb.seed_pair(T, Q, 15, 10, 8, 1, 4096).cands for T, Q in zip(Ts[:3], Qs[:3])] + [[]]


# ---- reads -> seeds -> chain -> alignment

def _same(got, want, n):
    """every output array of align_chain_device equal; a CIGAR row up to its length (the entry writes no byte at or beyond it)"""
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape
        if i == 4:
            a, b = a.reshape(n, -1), b.reshape(n, -1)
            assert all((a[p, :got[5][p]] == b[p, :got[5][p]]).all() for p in range(n))
        else:
            assert (a == b).all(), i


@pytest.mark.parametrize("k,w", [(15, 10), (11, 5)])
def test_reads_to_alignment_on_one_stream_equals_the_textbooks_candidates_uploaded(aligner, k, w):
    pairs = synth.chain_pairs(11, 16, length=2000)
    Ts, Qs = [p[0] for p in pairs], [p[1] for p in pairs]
    n, packed, stride = _pack(Ts, Qs)
    dev = torch.device("cuda", 0)
    start, ct, cq, cl, status = tb.seed_batch(Ts, Qs, k, w, 8, 1, 1024, 1 << 30)
    cap = start[-1] + 7
    align = dict(CHAINING, to_query_end=True, cigar_stride=stride, sides=True, gap_scores=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        seeds, chain, got = aligner.align_reads_device(*packed, 64, -1, GATK, k, w, 8, True, 1024, cap, **align)
    torch.cuda.synchronize()  # the one synchronisation: nothing above waited for the device
    g = lambda x, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=dt))).to(dev)  # noqa: E731
    pad = [0] * (cap - start[-1])  # (the arrays as long as the stage's: d_gap_score_out has one entry per candidate index)
    host = (g(start, np.int64), g(ct + pad, np.int32), g(cq + pad, np.int32), g(cl + pad, np.int32))
    want_chain, want = aligner.align_candidates_device(*packed[:6], *host, *packed[6:], 1024, 64, -1, GATK, **align)
    torch.cuda.synchronize()
    seeds = [x.cpu().numpy() for x in seeds]
    assert seeds[0].tolist() == start and (seeds[4] == 0).all() and status == [0] * n
    assert [x[:start[-1]].tolist() for x in seeds[1:4]] == [ct, cq, cl]
    tot = int(chain[0][-1])
    for i, (a, b) in enumerate(zip(chain, want_chain)):
        assert (a is None) == (b is None)
        if a is not None:
            a, b = a.cpu().numpy(), b.cpu().numpy()
            assert (a[:tot] == b[:tot]).all() if i in (1, 2, 3) else (a == b).all(), i
    got, want = [x.cpu().numpy() for x in got], [x.cpu().numpy() for x in want]
    assert len(got) == len(want) == 7
    for arr in (got, want):  # a gap score has one entry per candidate index: those behind the chains are not written
        arr[3] = arr[3][:tot]
    _same(got, want, n)
    assert (got[6] == 0).all() and (chain[-1].cpu().numpy() == 0).all()
    aln = got[0]
    assert (aln[:, 1] <= 200).all() and (aln[:, 2] >= np.array([len(T) for T in Ts]) - 200).all()
