"""mgl_sw_pileup_insertions_batch_device on the GPU against tests/calls_textbook.py, word for word.  The table stands between PAD canary
words in front of its first row and behind its last -- a step over a row's border shows in the neighbour row, one over the table's in
the canaries --, the site records behind the active ones are poison, and the status array is PAD entries longer than its size.  The
cases are tests/calls_cases.py's and, through it, tests/pileup_cases.py's and tests/describe_cases.py's."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import calls_cases as cc  # noqa: E402
import calls_textbook as ctb  # noqa: E402
import describe_cases as dc  # noqa: E402
import pileup_cases as pc  # noqa: E402
from mgl_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

BINARY = pytest.mark.parametrize("binary", [False, True], ids=["text", "binary"])
PAD = cc.PAD


@pytest.fixture(scope="module")
def aligner():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mgl_amd import smithwaterman as sw

    a = sw.MicrosoftSmithWaterman(0)
    assert a.load()
    yield a
    a.close()


def run(aligner, cases, sites, binary, max_ins=8, region_beg=0, n_sites=None, capacity=None, select=None, before=None, t_start=None, times=1, status=True,
        status_in=True, gaps=None):
    """the batch ``times`` times into one table over ``sites`` -> (the table's body [capacity, W] uint32, the textbook's)"""
    dev = torch.device("cuda", 0)
    n = len(cases)
    p = dc.pack(cases, binary, None, gaps)
    if t_start is not None:
        p["t_start"] = np.asarray(t_start, np.int64)
    capacity = max(len(sites), 1) if capacity is None else capacity
    n_sites = len(sites) if n_sites is None else n_sites
    width = ctb.width(max_ins)
    assert status_in or not any(c.status_in for c in cases)
    g = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    buf = torch.full((capacity * width + 2 * PAD,), cc.CANARY, dtype=torch.int32, device=dev)
    table = buf[PAD:PAD + capacity * width]
    if before is None:
        table.zero_()
    else:
        table.copy_(g(np.asarray(before, np.uint32).reshape(-1).view(np.int32)))
    st = torch.full((n + PAD,), cc.CANARY, dtype=torch.int32, device=dev) if status else None
    rows = g(cc.site_rows(sites[:capacity], capacity))
    ns = g(np.asarray([n_sites], np.int64))
    for _ in range(times):
        got = aligner.pileup_insertions_device(g(p["targets"]), g(p["t_start"]), g(p["t_len"]), g(p["queries"]), g(p["q_start"]), g(p["q_len"]), g(p["aln"]),
                                               g(p["cigar"]), p["cigar_stride"], g(p["cigar_len"]), rows, ns, g(p["status_in"]) if status_in else None,
                                               g(np.asarray(select, np.int32)) if select is not None else None, region_beg, max_ins, binary_cigar=binary,
                                               out=(table.view(capacity, width), st))
        assert got[1] is st
    torch.cuda.synchronize()
    want, want_st = cc.insertions_expected(cases, p["t_start"], region_beg, sites, n_sites, capacity, max_ins, select, before, times)
    x = buf.cpu().numpy().view(np.uint32)
    if not (x == want).all():
        k = int(np.flatnonzero(x != want)[0]) - PAD
        raise AssertionError("the table differs first at word %d (row %d, word %d of %d): got %r, want %r" % (
            k, k // width, k % width, width, x[k + PAD:k + PAD + 8].tolist(), want[k + PAD:k + PAD + 8].tolist()))
    if status:
        y = st.cpu().numpy()
        assert (y == want_st).all(), (np.flatnonzero(y != want_st)[:8].tolist(), y[:n].tolist(), want_st[:n].tolist())
    return x[PAD:-PAD].reshape(capacity, width), want[PAD:-PAD].reshape(capacity, width)


@BINARY
@pytest.mark.parametrize("k", cc.SITE_LIST_SIZES)
def test_site_lists_first_middle_last_and_no_site(aligner, binary, k):
    cases, sites = cc.site_list_case(np.random.default_rng(30 + k), k)
    got, _ = run(aligner, cases, sites, binary)
    assert int(got[:, :9].sum()) == min(k, 3)                  # the insertion behind NO_SITE adds nothing
    if k >= 3:
        assert got[0, 3] == 1 and got[-1, 4] == 1 and got[[s.pos for s in sites].index(cc.MIDDLE), 2] == 1


@BINARY
def test_n_sites_above_the_capacity_below_zero_and_below_the_records(aligner, binary):
    cases, sites = cc.site_list_case(np.random.default_rng(31), 65)
    got, _ = run(aligner, cases, sites, binary, n_sites=65 + 7)                 # clipped to the capacity
    assert got[-1, 4] == 1
    got, _ = run(aligner, cases, sites, binary, n_sites=(1 << 40))
    assert got[-1, 4] == 1
    got, _ = run(aligner, cases, sites, binary, n_sites=-3)                     # no active site
    assert not got.any()
    mid = [s.pos for s in sites].index(cc.MIDDLE)
    got, _ = run(aligner, cases, sites, binary, n_sites=mid + 1)                # the records behind the active ones are not matched
    assert got[mid, 2] == 1 and not got[mid + 1:].any()
    got, _ = run(aligner, cases, sites, binary, capacity=80)                    # rows behind the sites: poison records, untouched rows
    assert not got[65:].any()


@BINARY
@pytest.mark.parametrize("max_ins", [1, 64])
def test_lengths_one_max_ins_and_one_more(aligner, binary, max_ins):
    cases, sites = cc.length_cases(np.random.default_rng(32), max_ins)
    got, _ = run(aligner, cases, sites, binary, max_ins=max_ins)
    assert got[:, 0].sum() == 1 and got[:, max_ins].sum() >= 2 and got[-1, 1] == 1
    assert got[:, max_ins + 1:].sum() == (got[:, 1:max_ins + 1] * np.arange(1, max_ins + 1)).sum()   # a column word per inserted base


@BINARY
def test_leading_trailing_i_only_and_region_beg(aligner, binary):
    cases = pc.leading_insertions(np.random.default_rng(12))
    total = sum(len(c.t) for c in cases)
    everywhere = [cc.site(p) for p in range(total)]
    got, _ = run(aligner, cases, everywhere, binary, max_ins=5)
    # the leading I at position -1 matches no site; the second alignment's stands behind the last byte of the first one's target
    assert got[29, 5] == 2 and got[59, 5] == 1 and got[:, 0].sum() == 1 and got[total - 1, 3] == 1
    # with a region_beg the same positions are other sites, and the first alignment's leading I lies in front of the region still
    got, _ = run(aligner, cases, [cc.site(p) for p in range(total - 20)], binary, max_ins=5, region_beg=20)
    assert got[9, 5] == 2 and got[39, 5] == 1
    # a region that begins behind the first target: that leading I is inside it now -- at pos 0 with t_start moved
    moved = [100 + int(s) for s in np.cumsum([0] + [len(c.t) for c in cases[:-1]])]
    got, _ = run(aligner, cases, [cc.site(p) for p in range(0, total + 60)], binary, max_ins=5, region_beg=50, t_start=moved)
    assert got[49, 5] == 1 and got[79, 5] == 2
    # ... and a hand-made site at -1 is a site like any other: the rule is the equality of the positions
    got, _ = run(aligner, cases, [cc.site(-1), cc.site(29)], binary, max_ins=5)
    assert got[0, 5] == 1 and got[1, 5] == 2


@BINARY
def test_lane_and_chunk_seams(aligner, binary):
    cases, sites = cc.seam_case(np.random.default_rng(33), binary)
    got, _ = run(aligner, cases, sites, binary, max_ins=3)
    assert got[:, :4].sum() == 10 and got[:, 1:4].sum(axis=0).tolist() == [3, 4, 3]


@BINARY
def test_lower_case_n_and_odd_bytes(aligner, binary):
    cases, sites = cc.odd_bytes_case()
    got, _ = run(aligner, cases, sites, binary, max_ins=16)
    assert got[0, 16] == 1 and got[0, 17:].reshape(16, 5).argmax(axis=1).tolist() == [0, 1, 2, 3, 4, 4, 4, 4, 4, 4, 4, 4, 0, 1, 2, 3]


@BINARY
def test_identical_alignments_lose_no_add(aligner, binary):
    cases, t_start = pc.stacked(np.random.default_rng(14), 300, 200)
    got, _ = run(aligner, cases, [cc.site(50), cc.site(89), cc.site(150)], binary, t_start=t_start)
    assert got[1, 4] == 300 and got[1, 9:29].sum() == 1200 and set(got.reshape(-1).tolist()) == {0, 300} and not got[0].any() and not got[2].any()


@BINARY
def test_two_calls_accumulate_prefilled_and_wrapping(aligner, binary):
    cases, sites = cc.site_list_case(np.random.default_rng(34), 64)
    once, _ = run(aligner, cases, sites, binary)
    twice, _ = run(aligner, cases, sites, binary, times=2)
    assert (twice == 2 * once).all() and once.any()
    before = np.full(once.shape, 7, np.uint32)
    before[0, 3] = 0xFFFFFFFF
    got, _ = run(aligner, cases, sites, binary, before=before)
    assert got[0, 3] == 0 and got[0, 2] == 7 and got[-1, 4] == 8
    # two batches over one site list are the one batch of both
    more, more_sites = cc.length_cases(np.random.default_rng(35), 8)
    both = cases + more
    shared = sorted({s.pos for s in sites} | {s.pos + len(cases[0].t) for s in more_sites})
    shared = [cc.site(p) for p in shared]
    whole, _ = run(aligner, both, shared, binary)
    first, _ = run(aligner, cases, shared, binary)
    second, _ = run(aligner, more, shared, binary, region_beg=0, t_start=[len(cases[0].t) + int(s) for s in np.cumsum([0] + [len(c.t) for c in more[:-1]])],
                    before=first)
    assert (second == whole).all()


def test_text_and_binary_give_equal_tables(aligner):
    cases = dc.mixed_batch(np.random.default_rng(9), 60)
    total = sum(len(c.t) for c in cases)
    sites = [cc.site(p) for p in range(0, total, 2)]
    a, _ = run(aligner, cases, sites, False, max_ins=16)
    b, _ = run(aligner, cases, sites, True, max_ins=16)
    assert (a == b).all() and a[:, 0].any() and a[:, 1:17].any()


@BINARY
def test_a_batch_larger_than_the_grid(aligner, binary):
    cases = dc.mixed_batch(np.random.default_rng(9), 300) * 24   # 7 200 alignments: the persistent loop turns
    starts = np.tile(np.cumsum([0] + [len(c.t) for c in cases[:299]]), 24)
    total = int(starts[299]) + len(cases[299].t)
    run(aligner, cases, [cc.site(p) for p in range(0, total, 3)], binary, max_ins=4, t_start=starts)


@BINARY
def test_poisoned_slots_under_a_status_and_under_a_zero_select(aligner, binary):
    cases = pc.poisoned(np.random.default_rng(15))
    total = sum(len(c.t) for c in cases)
    sites = [cc.site(p) for p in range(total)]
    under_status = [cases[0], cases[1]._replace(status_in=9, want=0), cases[2]]
    got, want = run(aligner, under_status, sites, binary)
    assert want.any()
    run(aligner, cases, sites, binary, select=[1, 0, 7], status_in=False)
    got, _ = run(aligner, cases, sites, binary, select=[0, 0, 0])
    assert not got.any()
    run(aligner, [cases[0], cases[2]], sites, binary, select=[0, 1], status=False)


def test_refused_alignments_add_nothing(aligner):
    for binary, cases in ((False, dc.refusals(np.random.default_rng(4))), (True, dc.binary_refusals(np.random.default_rng(5)))):
        total = sum(len(c.t) for c in cases)
        got, _ = run(aligner, cases, [cc.site(p) for p in range(total)], binary)
        assert sorted(set(pc.statuses(cases))) == [0, pc.BAD_ARG, 5] and got.any()


def test_an_empty_batch_and_every_call_level_refusal(aligner):
    run(aligner, [], [cc.site(3)], False)
    dev = torch.device("cuda", 0)
    cases, sites = cc.odd_bytes_case()
    p = dc.pack(cases, False)
    g = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    t = {k: g(v) for k, v in p.items() if k != "cigar_stride"}
    rows, ns = g(cc.site_rows(sites)), g(np.asarray([1], np.int64))
    table = torch.zeros((1, ctb.width(8)), dtype=torch.int32, device=dev)
    names = ["targets", "t_start", "t_len", "queries", "q_start", "q_len", "aln", "cigar"]

    def call(ctx=None, n=1, stride=p["cigar_stride"], beg=0, cap=1, max_ins=8, flags=0, null=None, status_in=True, select=True, status=True):
        ptr = lambda name, x: None if name == null else x.data_ptr()  # noqa: E731
        sel = torch.ones(1, dtype=torch.int32, device=dev)
        return _lib.lib().mgl_sw_pileup_insertions_batch_device(
            aligner.ctx if ctx is None else ctx, None, n, *[ptr(k, t[k]) for k in names], stride, ptr("cigar_len", t["cigar_len"]),
            t["status_in"].data_ptr() if status_in else None, sel.data_ptr() if select else None, beg, ptr("sites", rows), ptr("n_sites", ns), cap, max_ins,
            ptr("ins", table), torch.empty(1, dtype=torch.int32, device=dev).data_ptr() if status else None, flags)

    bad = _lib.ERR_BAD_ARG
    for null in names + ["cigar_len", "sites", "n_sites", "ins"]:
        assert call(null=null) == bad, null
    assert call(n=-1) == bad and call(n=(1 << 30) + 1) == bad and call(stride=0) == bad and call(stride=p["cigar_stride"] + 1, flags=_lib.FLAG_BINARY_CIGAR) == bad
    assert call(beg=-1) == bad and call(cap=0) == bad and call(cap=(1 << 30) + 1) == bad and call(max_ins=0) == bad and call(max_ins=65) == bad
    assert b"max_ins outside 1 .. 64" in _lib.lib().mgl_sw_last_error(aligner.ctx)
    torch.cuda.synchronize()
    assert not table.cpu().numpy().any()                        # nothing was launched
    # on the other side of every edge the call is taken
    assert call() == call(n=0) == call(max_ins=1) == call(status_in=False, select=False, status=False) == _lib.OK
    torch.cuda.synchronize()
    assert table.cpu().numpy().view(np.uint32)[0, 8] == 0 and table.cpu().numpy()[0, 0] == 3   # three times longer than max_ins = 8 or 1: word 0
