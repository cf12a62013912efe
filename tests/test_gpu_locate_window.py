"""mgl_sw_locate_window_batch_device on the GPU against tests/index_textbook.py's locate_window, bit for bit, out of place and in place:
the hand-made chains of tests/index_cases.py, more pairs than one launch has waves in flight per block, an empty anchor array, and
refused pairs at the front, in the middle and at the end whose anchors stay untouched.  Canaries of 16 entries behind every array."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import index_cases as ic  # noqa: E402
import index_textbook as itb  # noqa: E402
from mgl_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

PAD = 16
CANARY = ic.CANARY


@pytest.fixture(scope="module")
def aligner():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mgl_amd import smithwaterman as sw

    a = sw.MicrosoftSmithWaterman(0)
    assert a.load()
    yield a
    a.close()


def _check(al, ref_len, q_len, chains, slack, max_tl, in_place, status=True):
    """one call into canaried arrays against the textbook -> (t_start, t_len, status) as the textbook has them"""
    dev = torch.device("cuda", 0)
    n = len(q_len)
    start, at, aq, al_ = ic.csr(chains)
    total = len(at)
    want = itb.locate_window(ref_len, q_len, start, at, aq, al_, slack, max_tl)
    g = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    t_in = torch.full((total + PAD,), CANARY, dtype=torch.int32, device=dev)
    t_in[:total] = g(at)
    full = [torch.full((n + PAD,), CANARY, dtype=torch.int64, device=dev), torch.full((n + PAD,), CANARY, dtype=torch.int32, device=dev),
            t_in if in_place else torch.full((total + PAD,), CANARY, dtype=torch.int32, device=dev), torch.full((n + PAD,), CANARY, dtype=torch.int32, device=dev)]
    out = (full[0][:n], full[1][:n], full[2][:total], full[3][:n] if status else None)
    got = al.locate_window_device(ref_len, g(np.asarray(q_len, np.int32)), g(start), t_in[:total], g(aq), g(al_), slack, max_tl, out=out)
    torch.cuda.synchronize()
    assert got is out
    got = [x.cpu().numpy() for x in full]
    # an anchor no pair wrote: the input's value in place, the canary out of place
    exp_t = np.array([(int(at[i]) if in_place else CANARY) if v is None else v for i, v in enumerate(want[2])] + [CANARY] * PAD, np.int64)
    exp = [np.array(want[0] + [CANARY] * PAD), np.array(want[1] + [CANARY] * PAD), exp_t, np.array((want[3] if status else [CANARY] * n) + [CANARY] * PAD)]
    for name, a, b in zip(("t_start", "t_len", "anchor_t", "status"), got, exp):
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, (name, bad[:8], a[bad[:8]], b[bad[:8]])
    if not in_place:
        assert (t_in.cpu().numpy()[:total] == at).all()  # the input is read only
    return want[0], want[1], want[3]


@pytest.mark.parametrize("in_place", [False, True])
def test_hand_made_chains(aligner, in_place):
    ref_len, slack, max_tl, chains = ic.locate_cases()
    q_len, anchors = [c[1] for c in chains], [c[2] for c in chains]
    _, _, status = _check(aligner, ref_len, q_len, anchors, slack, max_tl, in_place)
    assert status == [c[3] for c in chains] and {0, itb.BAD_ARG, itb.UNSUPPORTED} == set(status)
    _check(aligner, ref_len, q_len, anchors, slack, max_tl, in_place, status=False)
    _check(aligner, ref_len, q_len, anchors, 0, max_tl, in_place)              # slack = 0
    _check(aligner, (1 << 31) - 1, q_len, anchors, slack, max_tl, in_place)    # the largest reference: nothing is clipped at its end
    # refused pairs at the front, in the middle and at the end, their anchors untouched
    bad = [("l<1", 500, [(100, 10, 10), (200, 110, 0)]), ("max_tl+1", 1300, [(2000, 0, 10), (3291, 1290, 10)])]
    framed = [bad[0]] + [c[:3] for c in chains[:3]] + bad + [c[:3] for c in chains[:2]] + [bad[1], bad[0]]
    _, _, status = _check(aligner, ref_len, [c[1] for c in framed], [c[2] for c in framed], slack, max_tl, in_place)
    assert status == [1, 0, 0, 0, 1, 5, 0, 0, 5, 1]


@pytest.mark.parametrize("in_place", [False, True])
def test_more_pairs_than_a_grid_step_of_one_anchor_each_and_an_empty_batch(aligner, in_place):
    rng = np.random.default_rng(1025)
    n = 1025
    q_len = rng.integers(50, 400, n).tolist()
    chains = [[(int(rng.integers(0, 90000)), int(rng.integers(0, ql - 20)), 20)] for ql in q_len]
    chains[7], chains[1024] = [], [(99990, 5, 20)]  # an unmapped read; an anchor that leaves the reference
    t_start, t_len, status = _check(aligner, 100000, q_len, chains, 150, 690, in_place)  # (a window is ql + 300 unless clipped: the longest reads are refused)
    assert status.count(0) >= 900 and status[1024] == itb.BAD_ARG and status.count(itb.UNSUPPORTED) >= 1 and (t_start[7], t_len[7]) == (0, 0)
    # no anchors at all, and no pairs
    _check(aligner, 100000, [100, 200, 0], [[], [], []], 10, 600, in_place)
    _check(aligner, 100000, [], [], 10, 600, in_place)


def test_ranges_of_anchor_start_that_descend_or_leave_the_anchors(aligner):
    dev = torch.device("cuda", 0)
    g = lambda x, dt: torch.from_numpy(np.asarray(x, dtype=dt)).to(dev)  # noqa: E731
    at, aq, al_ = [3000, 3400, 5000], [10, 420, 7], [20, 30, 9]
    for start in ([0, 2, 3], [2, 0, 3], [-1, 2, 3], [0, 2, 4], [0, 3, 2]):
        want = itb.locate_window(10000, [1000, 100], start, at, aq, al_, 50, 2000)
        got = aligner.locate_window_device(10000, g([1000, 100], np.int32), g(start, np.int64), g(at, np.int32), g(aq, np.int32), g(al_, np.int32), 50, 2000)
        torch.cuda.synchronize()
        t_start, t_len, t_out, status = (x.cpu().numpy().tolist() for x in got)
        assert (t_start, t_len, status) == (want[0], want[1], want[3]), start
        assert all(v is None or v == t_out[i] for i, v in enumerate(want[2]))
    assert _lib.ERR_BAD_ARG == itb.BAD_ARG and _lib.ERR_UNSUPPORTED == itb.UNSUPPORTED
