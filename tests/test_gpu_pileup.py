"""mgl_sw_pileup_alignments_batch_device and mgl_sw_pileup_sites_device on the GPU against tests/pileup_textbook.py, word for word.
The table of the first entry stands between PAD canary words in front of plane 0 and behind plane 7 -- a step over a plane's border
shows in the neighbour plane, one over the table's in the canaries --, the outputs of the second are PAD entries longer than their
size and start as canaries.  The cases are tests/pileup_cases.py's and, through it, tests/describe_cases.py's."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import describe_cases as dc  # noqa: E402
import pileup_cases as pc  # noqa: E402
import pileup_textbook as ptb  # noqa: E402
from mgl_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

BINARY = pytest.mark.parametrize("binary", [False, True], ids=["text", "binary"])
PAD = pc.PAD


@pytest.fixture(scope="module")
def aligner():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mgl_amd import smithwaterman as sw

    a = sw.MicrosoftSmithWaterman(0)
    assert a.load()
    yield a
    a.close()


def run(aligner, cases, binary, region=None, gaps=None, select=None, before=None, t_start=None, times=1, status=True, status_in=True,
        copies=1):
    """the batch -- ``copies`` of it in one call, at the same positions -- ``times`` times into one table -> (the table's body
    [8, region_len] uint32, the textbook's)"""
    dev = torch.device("cuda", 0)
    n = len(cases) * copies
    p = dc.pack(cases * copies, binary, None, gaps)
    if t_start is not None:
        p["t_start"] = np.asarray(t_start, np.int64)
    if copies > 1:  # every copy reads the first one's targets
        p["t_start"] = np.tile(p["t_start"][:len(cases)], copies)
    beg, length = region = region or (0, len(p["targets"]))
    assert status_in or not any(c.status_in for c in cases)
    g = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    buf = torch.full((8 * length + 2 * PAD,), pc.CANARY, dtype=torch.int32, device=dev)
    table = buf[PAD:PAD + 8 * length]
    if before is None:
        table.zero_()
    else:
        table.copy_(g(np.asarray(before, np.uint32).reshape(-1).view(np.int32)))
    st = torch.full((n + PAD,), pc.CANARY, dtype=torch.int32, device=dev) if status else None
    for _ in range(times):
        got = aligner.pileup_device(g(p["targets"]), g(p["t_start"]), g(p["t_len"]), g(p["queries"]), g(p["q_start"]), g(p["q_len"]), g(p["aln"]),
                                    g(p["cigar"]), p["cigar_stride"], g(p["cigar_len"]), g(p["status_in"]) if status_in else None,
                                    g(np.asarray(select, np.int32)) if select is not None else None, region, binary_cigar=binary, out=(table, st))
        assert got[0] is table
    torch.cuda.synchronize()
    want, want_st = pc.expected(cases, p["t_start"][:len(cases)], region, select, before, times * copies)
    want_st = np.concatenate([np.tile(want_st[:len(cases)], copies), want_st[len(cases):]])
    x = buf.cpu().numpy().view(np.uint32)
    if not (x == want).all():
        k = int(np.flatnonzero(x != want)[0]) - PAD
        raise AssertionError("the table differs first at word %d (plane %d, position %d of the region): got %r, want %r" % (
            k, k // length, k % length, x[k + PAD:k + PAD + 8].tolist(), want[k + PAD:k + PAD + 8].tolist()))
    if status:
        y = st.cpu().numpy()
        assert (y == want_st).all(), (np.flatnonzero(y != want_st)[:8].tolist(), y[:n].tolist(), want_st[:n].tolist())
    return x[PAD:-PAD].reshape(8, length), want[PAD:-PAD].reshape(8, length)


@BINARY
def test_step_seams(aligner, binary):
    cases = [c for c in dc.seam_cases(np.random.default_rng(1))]
    assert {c.cigar[0][0] for c in cases} >= set(dc.STEP_COLUMNS)
    got, _ = run(aligner, cases, binary)
    assert int(got[:5].sum()) == sum(c.cigar[0][0] for c in cases) and not got[5:].any()


@BINARY
def test_indels_chunks_and_bytes(aligner, binary):
    cases = dc.indel_cases(np.random.default_rng(2))
    assert max(len(c.cigar) for c in cases) == 6000 > 512  # more than one LDS chunk
    got, _ = run(aligner, cases, binary)
    assert got[5].any() and got[6].any() and got[4].any()


@BINARY
def test_leading_trailing_adjacent_and_odd_bytes(aligner, binary):
    cases = pc.leading_insertions(np.random.default_rng(12))
    got, _ = run(aligner, cases, binary)
    # the leading I at position 0 is dropped; the second alignment's is counted on the last byte of the first one's target
    assert got[6, 29] == 2 and got[7, 29] == 10 and got[7, 59] == 5 and got[4].sum() >= 8
    assert got[6, -1] == 1 and got[7, -1] == 3  # the I-only alignment behind the buffer's last byte


@BINARY
def test_every_byte_offset(aligner, binary):
    cases, gaps = dc.offset_cases(np.random.default_rng(3))
    run(aligner, cases, binary, gaps=gaps)


@BINARY
def test_region_edges(aligner, binary):
    rng = np.random.default_rng(13)
    case, columns = pc.edge_alignment(rng)
    other = dc.case(*dc.random_alignment(rng, 5))
    cases = [other, case, other]
    first = len(other.t) + case.rec[0]  # the position of the alignment's column 0
    total = 2 * len(other.t) + len(case.t)
    for c in columns:
        run(aligner, cases, binary, region=(first + c, total - first - c + 5))  # beginning at column c
        run(aligner, cases, binary, region=(0, first + c))                      # ending in front of it
    got, _ = run(aligner, cases, binary, region=(first + 149, 1))               # region_len = 1: the position the I stands behind
    assert got[6, 0] == 1 and got[7, 0] == 5 and got[:5].sum() == 1
    got, _ = run(aligner, cases, binary, region=(first + 75, 1))                # inside the D run
    assert got[5, 0] == 1 and got.sum() == 1
    got, _ = run(aligner, cases, binary, region=(total + 1000, 50))             # a region that no alignment touches
    assert not got.any()


def test_text_and_binary_give_equal_tables(aligner):
    cases = dc.mixed_batch(np.random.default_rng(9), 60)
    a, _ = run(aligner, cases, False)
    b, _ = run(aligner, cases, True)
    assert (a == b).all() and a.any()


@BINARY
def test_identical_alignments_lose_no_add(aligner, binary):
    cases, t_start = pc.stacked(np.random.default_rng(14), 300, 200)
    got, _ = run(aligner, cases, binary, t_start=t_start, region=(0, 200))
    depth = got[:6].sum(axis=0)
    assert (depth == 300).all() and got[6, 89] == 300 and got[7, 89] == 1200 and set(got[:6].reshape(-1).tolist()) == {0, 300}


@BINARY
def test_accumulating_prefilled_and_wrapping(aligner, binary):
    cases, gaps = dc.offset_cases(np.random.default_rng(3))
    once, _ = run(aligner, cases, binary, gaps=gaps)
    twice, _ = run(aligner, cases, binary, gaps=gaps, times=2)
    assert (twice == 2 * once).all() and once.any()
    before = np.full(once.shape, 7, np.uint32)
    plane, pos = (int(v[0]) for v in np.nonzero(once))
    before[plane, pos] = 0xFFFFFFFF
    got, _ = run(aligner, cases, binary, gaps=gaps, before=before)
    assert got[plane, pos] == once[plane, pos] - 1 and got[plane, pos + 1] == once[plane, pos + 1] + 7


def test_refusals_in_text_add_nothing(aligner):
    cases = dc.refusals(np.random.default_rng(4))
    run(aligner, cases, False)
    assert sorted(set(pc.statuses(cases))) == [0, pc.BAD_ARG, 5]


def test_refusals_in_binary_add_nothing(aligner):
    cases = dc.binary_refusals(np.random.default_rng(5))
    run(aligner, cases, True)
    assert sorted(set(pc.statuses(cases))) == [0, pc.BAD_ARG, 5]


@BINARY
def test_poisoned_slots_under_a_status_and_under_a_zero_select(aligner, binary):
    cases = pc.poisoned(np.random.default_rng(15))
    under_status = [cases[0], cases[1]._replace(status_in=9, want=0), cases[2]]
    got, want = run(aligner, under_status, binary)
    assert want.any()
    run(aligner, cases, binary, select=[1, 0, 7], status_in=False)
    got, _ = run(aligner, cases, binary, select=[0, 0, 0])
    assert not got.any()
    run(aligner, [cases[0], cases[2]], binary, select=[0, 1], status=False)


@BINARY
def test_a_batch_larger_than_the_grid(aligner, binary):
    cases = dc.mixed_batch(np.random.default_rng(9), 300)
    run(aligner, cases, binary)
    run(aligner, cases, binary, copies=24)  # 7 200 alignments: more than the waves of the largest grid, so the persistent loop turns


def test_over_lists_and_an_empty_batch(aligner):
    rng = np.random.default_rng(11)
    als = [dc.random_alignment(rng, 7, p_mismatch=0.2) for _ in range(9)]
    text = ["".join("%d%s" % e for e in a[2]) for a in als]
    positions = [100 * k for k in range(9)]
    for binary in (False, True):
        got = aligner.pileup([a[0] for a in als], [a[1] for a in als], text, positions=positions, region=(50, 900), binary_cigar=binary)
        want = ptb.pileup([(p, a[1], a[2]) for p, a in zip(positions, als)], 50, 900)
        assert got.dtype == np.uint32 and got.tolist() == want
    with pytest.raises(_lib.MglSwError):
        aligner.pileup([b"ACGT"], [b"ACGT"], ["3M"])
    counts, st = aligner.pileup([b"ACGT"], [b"ACGT"], ["3M"], return_status=True)
    assert st.tolist() == [pc.BAD_ARG] and not counts.any()
    run(aligner, [], False, region=(0, 10))


# ---- the sites entry

def run_sites(aligner, counts, ref, params, textbook, capacity, region_beg=0, call=True, flags=True, sites=True):
    dev = torch.device("cuda", 0)
    length = counts.shape[1]
    g = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    u8 = lambda m: torch.full((m + PAD,), pc.CANARY & 0xff, dtype=torch.uint8, device=dev)  # noqa: E731
    out = (u8(length) if call else None, u8(length) if flags else None,
           torch.full(((capacity + PAD) * 8,), pc.CANARY, dtype=torch.int32, device=dev) if sites else None,
           torch.full((1 + PAD,), pc.CANARY, dtype=torch.int64, device=dev))
    got = aligner.pileup_sites_device(g(counts.view(np.int32)), g(np.frombuffer(ref, np.uint8).copy()), region_beg, *params, site_capacity=capacity, out=out)
    torch.cuda.synchronize()
    assert got is out
    want = pc.sites_expected(textbook, capacity)
    for name, x, y in zip(("call", "flags", "sites", "n_sites"), out, want):
        if x is None:
            continue
        x = x.cpu().numpy()
        if not (x == y).all():
            k = int(np.flatnonzero(x != y)[0])
            raise AssertionError("%s differs first at entry %d: got %r, want %r (length %d, capacity %d)" % (
                name, k, x[k:k + 8].tolist(), y[k:k + 8].tolist(), length, capacity))
    return int(want[3][0])


def test_sites_ties_on_every_pair_of_channels(aligner):
    counts, ref = pc.tie_tables()
    for params in ((1, 1, 1), (4, 2, 64)):
        tb = pc.sites_textbook(counts, ref, 0, params)
        assert run_sites(aligner, counts, ref, params, tb, len(tb[2])) == len(tb[2]) > 0
    shifted = b"TTT" + ref + b"T"
    tb = pc.sites_textbook(counts, shifted, 3, (1, 1, 1))
    assert tb == pc.sites_textbook(counts, ref, 0, (1, 1, 1))
    run_sites(aligner, counts, shifted, (1, 1, 1), tb, len(tb[2]), region_beg=3)


def test_sites_thresholds_odd_reference_bytes_and_clipping(aligner):
    counts, ref, params = pc.threshold_tables()
    tb = pc.sites_textbook(counts, ref, 0, params)
    assert max(s.depth for s in tb[2]) == ptb.CLIP
    run_sites(aligner, counts, ref, params, tb, len(tb[2]))
    for other in ((1, 1, 1), (1, 1, 256), (params[0] + 1, params[1], params[2]), (params[0], params[1] + 1, params[2]), (params[0], params[1], params[2] + 1)):
        tb = pc.sites_textbook(counts, ref, 0, other)
        run_sites(aligner, counts, ref, other, tb, len(tb[2]))


@pytest.mark.parametrize("length", pc.REGION_LENGTHS)
def test_sites_region_lengths_and_capacities(aligner, length):
    assert pc.SITE_BLOCK - 1 in pc.REGION_LENGTHS and pc.SITE_BLOCK + 1 in pc.REGION_LENGTHS
    counts, ref = pc.region_table(np.random.default_rng(length), length, "edges")
    params = (4, 2, 64)
    tb = pc.sites_textbook(counts, ref, 0, params)
    total = len(tb[2])
    assert total >= 1 and tb[2][0].pos == 0 and tb[2][-1].pos == length - 1
    for capacity in sorted({0, total - 1, total}):
        assert run_sites(aligner, counts, ref, params, tb, capacity) == total
    run_sites(aligner, counts, ref, params, tb, 0, call=False, flags=False, sites=False)  # the sizing pass with nothing else written


@pytest.mark.parametrize("kind", ["none", "all"])
def test_sites_none_and_everywhere(aligner, kind):
    for length in (1, 1025):
        counts, ref = pc.region_table(np.random.default_rng(17), length, kind)
        tb = pc.sites_textbook(counts, ref, 0, (4, 2, 64))
        assert len(tb[2]) == (0 if kind == "none" else length)
        for capacity in sorted({0, max(len(tb[2]) - 1, 0), len(tb[2]), len(tb[2]) + 3}):
            run_sites(aligner, counts, ref, (4, 2, 64), tb, capacity)


def test_sites_behind_the_pileup_on_one_stream(aligner):
    cases, t_start = pc.stacked(np.random.default_rng(14), 12, 200)
    dev = torch.device("cuda", 0)
    p = dc.pack(cases, False)
    g = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    ref = g(p["targets"][:200])
    counts, st = aligner.pileup_device(ref, g(np.asarray(t_start, np.int64)), g(p["t_len"]), g(p["queries"]), g(p["q_start"]), g(p["q_len"]), g(p["aln"]),
                                       g(p["cigar"]), p["cigar_stride"], g(p["cigar_len"]), region=(0, 200))
    call, flags, sites, ns = aligner.pileup_sites_device(counts, ref)
    torch.cuda.synchronize()  # the one synchronisation
    table = ptb.pileup(pc.alignments(cases, t_start), 0, 200)
    want = ptb.sites(table, bytes(p["targets"][:200]), 0, 4, 2, 64)
    total = int(ns[0])
    assert counts.cpu().numpy().view(np.uint32).tolist() == table and not st.cpu().numpy().any()
    assert call.cpu().numpy().tobytes() == want[0] and flags.cpu().numpy().tolist() == want[1] and total == len(want[2]) > 10
    assert [tuple(r) for r in sites.cpu().numpy()[:total].tolist()] == [tuple(s) for s in want[2]]
