"""mgl_sw_genotype_sites_device on the GPU against tests/calls_textbook.py, record for record, on hand-made tables with no alignment
behind them (tests/calls_cases.py).  The outputs are PAD entries longer than their capacity and start as canaries; the site records
behind the active ones continue the runs they cut."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import calls_cases as cc  # noqa: E402
import calls_textbook as ctb  # noqa: E402
import pileup_textbook as ptb  # noqa: E402
from mgl_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
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


def run(aligner, t, capacity=None, n_sites=None, region_beg=0, seq=True, calls=True):
    """-> the total.  ``capacity`` None: exactly the textbook's total"""
    dev = torch.device("cuda", 0)
    tb = cc.calls_textbook(t, n_sites)
    capacity = len(tb[0]) if capacity is None else capacity
    g = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    counts = g(np.asarray(t.counts, np.uint64).astype(np.uint32).view(np.int32))
    ref = g(np.frombuffer(b"T" * region_beg + t.ref, np.uint8).copy())
    sites = g(np.asarray(t.sites, np.int64).astype(np.int32).reshape(-1, 8))
    ns = g(np.asarray([t.n_sites if n_sites is None else n_sites], np.int64))
    ins = g(np.asarray(t.ins, np.uint64).astype(np.uint32).view(np.int32)) if t.ins is not None else None
    out = (torch.full(((capacity + PAD) * 16,), cc.CANARY, dtype=torch.int32, device=dev) if calls else None,
           torch.full((1 + PAD,), cc.CANARY, dtype=torch.int64, device=dev),
           torch.full(((capacity + PAD) * t.max_ins,), cc.CANARY & 0xff, dtype=torch.uint8, device=dev) if seq else None)
    got = aligner.genotype_sites_device(counts, ref, sites, ns, ins, region_beg, t.max_ins, t.max_del, costs=t.costs, call_capacity=capacity, out=out)
    torch.cuda.synchronize()
    assert got is out
    want = cc.calls_expected(tb, capacity, t.max_ins, seq)
    for name, x, y, width in zip(("calls", "n_calls", "seq"), out, want, (16, 1, t.max_ins)):
        if x is None:
            continue
        x = x.cpu().numpy()
        if not (x == y).all():
            k = int(np.flatnonzero(x != y)[0])
            raise AssertionError("%s differs first at entry %d (record %d): got %r, want %r (capacity %d)" % (
                name, k, k // width, x[k // width * width:k // width * width + width].tolist(), y[k // width * width:k // width * width + width].tolist(), capacity))
    return len(tb[0])


def test_each_kind_alone_together_odd_references_and_a_site_outside(aligner):
    t = cc.kinds_table()
    assert run(aligner, t) == 8
    assert run(aligner, t, region_beg=5) == 8                   # the reference bytes lie behind region_beg


def test_without_the_insertion_table(aligner):
    t = cc.kinds_table()._replace(ins=None)
    assert run(aligner, t) == 6
    assert run(aligner, t, seq=False) == 6                      # ... and then without the sequence rows


@pytest.mark.parametrize("max_del", [1, 2, 5, 6, 11, 4096])
def test_deletion_runs_at_max_del(aligner, max_del):
    t = cc.runs_table(5)._replace(max_del=max_del)
    total = run(aligner, t)
    calls = cc.calls_textbook(t)[0]
    assert total == len(calls) and (max_del != 5 or [(c.len, c.flags) for c in calls[:5]] == [(1, 0), (2, 0), (5, 0), (5, 1), (5, 1)])


def test_runs_broken_by_a_gap_and_cut_by_n_sites(aligner):
    t = cc.runs_table(5)
    lens = lambda n: [c.len for c in cc.calls_textbook(t, n)[0] if c.kind == ctb.DELETION]  # noqa: E731
    assert lens(None)[-1] == 2 and lens(len(t.sites))[-1] == 4
    for n in (len(t.sites), len(t.sites) - 1, len(t.sites) - 2, len(t.sites) - 3, len(t.sites) + 9, 1 << 40):
        run(aligner, t, n_sites=n)


def test_a_run_and_all_kinds_over_the_blocks_seam(aligner):
    t = cc.block_seam_table()
    assert [s.pos for s in t.sites[255:257]] == [505, 506] and run(aligner, t) == 604
    for capacity in (0, 258, 259, 260, 603, 604, 700):         # the capacity ends inside a site's events, at the seam and at the end
        assert run(aligner, t, capacity) == 604
    for n in (255, 256, 257):                                   # the run is cut at the seam
        run(aligner, t, n_sites=n)


def test_modal_length_and_column_plurality_on_ties(aligner):
    t = cc.insertion_ties_table()
    assert run(aligner, t) == 5
    assert cc.calls_textbook(t)[1] == [b"CT\0\0", b"TGC\0", b"AAAA", b"A\0\0\0", b"NT\0\0"]


def test_max_ins_of_one_and_sixty_four(aligner):
    for m in (1, 64):
        word = {m: 9, **{cc.col(m, j, (j + 1) % 5): 9 for j in range(m)}}
        t = cc.table([dict(pos=3, c=[16, 0, 0, 0, 0, 0, 9, 9 * m], flags=cc.INS_F, ins=word), dict(pos=5, c=[8, 0, 8], flags=cc.SNV_F, alt=2)], max_ins=m)
        assert run(aligner, t) == 2
        assert cc.calls_textbook(t)[1][0] == bytes(b"CGTNA"[j % 5] for j in range(m))


def test_the_genotypes_worked_by_hand(aligner):
    for t, rows in cc.genotype_tables():
        assert run(aligner, t) == len(rows)
        calls = cc.calls_textbook(t)[0]
        assert [(c.gt, (c.pl0, c.pl1, c.pl2), c.gq) for c in calls] == [(g[3], g[4], g[5]) for g in rows]


def test_capacities_and_no_sites(aligner):
    t = cc.kinds_table()
    for capacity in (0, 7, 8, 11):
        assert run(aligner, t, capacity) == 8
    assert run(aligner, t, 0, calls=False, seq=False) == 8      # the sizing pass with nothing else written
    for n in (0, -1):
        assert run(aligner, t, n_sites=n) == 0 and run(aligner, t, 4, n_sites=n) == 0


def test_every_call_level_refusal(aligner):
    dev = torch.device("cuda", 0)
    t = cc.kinds_table()
    g = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    bufs = dict(counts=g(np.asarray(t.counts, np.uint64).astype(np.uint32).view(np.int32)), targets=g(np.frombuffer(t.ref, np.uint8).copy()),
                sites=g(np.asarray(t.sites, np.int64).astype(np.int32)), n_sites=g(np.asarray([len(t.sites)], np.int64)),
                ins=g(np.asarray(t.ins, np.uint64).astype(np.uint32).view(np.int32)), calls=torch.full((30, 16), cc.CANARY, dtype=torch.int32, device=dev),
                n_calls=torch.full((1,), cc.CANARY, dtype=torch.int64, device=dev), seq=torch.zeros((30, 64), dtype=torch.uint8, device=dev))

    def call(length=40, beg=0, cap=len(t.sites), max_ins=4, max_del=8, costs=cc.Q20, call_cap=30, null=(), ctx=None):
        p = {k: None if k in null else v.data_ptr() for k, v in bufs.items()}
        return _lib.lib().mgl_sw_genotype_sites_device(ctx or aligner.ctx, None, p["counts"], length, p["targets"], beg, p["sites"], p["n_sites"], cap, p["ins"], max_ins,
                                                       max_del, *costs, p["calls"], call_cap, p["n_calls"], p["seq"])

    bad = _lib.ERR_BAD_ARG
    for null in ("counts", "targets", "sites", "n_sites", "n_calls", "calls", "seq"):
        assert call(null=(null,)) == bad, null
    assert call(length=0) == bad and call(length=1 << 31) == bad and call(beg=-1) == bad and call(cap=0) == bad and call(cap=(1 << 30) + 1) == bad
    assert call(max_ins=0) == bad and call(max_ins=65) == bad and call(max_del=0) == bad and call(max_del=4097) == bad
    assert call(costs=(0, 2, 3)) == bad and call(costs=(1, 2, (1 << 20) + 1)) == bad and call(costs=(2, 2, 3)) == bad and call(costs=(1, 3, 3)) == bad
    assert call(call_cap=-1) == bad and call(call_cap=(1 << 30) + 1) == bad
    assert b"call_capacity outside 0 .. 2^30" in _lib.lib().mgl_sw_last_error(aligner.ctx)
    torch.cuda.synchronize()
    assert int(bufs["n_calls"][0]) == cc.CANARY and (bufs["calls"].cpu().numpy() == cc.CANARY).all()       # nothing was launched
    # on the other side of the edges the call is taken
    assert call() == call(null=("ins", "seq")) == call(call_cap=0, null=("calls", "seq")) == call(costs=(1, 2, 3)) == call(max_del=4096) == _lib.OK
    torch.cuda.synchronize()
    assert int(bufs["n_calls"][0]) == 8
    # a workspace limit that does not hold the blocks' counts: MGL_SW_ERR_NOMEM before any device work (a context of its own)
    from mgl_amd import smithwaterman as sw

    with sw.MicrosoftSmithWaterman(0) as small:
        small.set_workspace(1 << 20)
        assert call(cap=1 << 30, call_cap=0, ctx=small.ctx) == _lib.ERR_NOMEM
        assert call(ctx=small.ctx) == _lib.OK
        torch.cuda.synchronize()
