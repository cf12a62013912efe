"""mgl_sw_locate_window_contigs_batch_device on the GPU against tests/contig_textbook.py's locate_window_contigs, bit for bit, out of
place and in place, with and without the status: the hand-made chains of tests/contig_cases.py (windows clipped on either side, a
chain over two contigs refused), refused reads at the front, in the middle and at the end, chains of more than 64 anchors, more reads
than a grid step, and an index without contigs, which is tests/index_textbook.py's locate_window.  Canaries behind every array."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contig_cases as cc  # noqa: E402
import contig_textbook as gtb  # noqa: E402
import index_textbook as itb  # noqa: E402

pytestmark = pytest.mark.gpu

PAD = 16
CANARY = cc.CANARY


@pytest.fixture(scope="module")
def aligner():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mgl_amd import smithwaterman as sw

    a = sw.MicrosoftSmithWaterman(0)
    assert a.load()
    yield a
    a.close()


@pytest.fixture(scope="module")
def indexes(aligner):
    """the table of contig_cases.locate_cases over a buffer of 3 502 bytes, and the same buffer without contigs"""
    start, length, _, _, _ = cc.locate_cases()
    buffer = bytearray(b"ACGGT" * 701)[:3502]
    for c in range(2):
        buffer[start[c] + length[c]] = ord("N")
    with aligner.build_index_contigs_device(bytes(buffer), start, length, k=15, w=10) as index, aligner.build_index(bytes(buffer), 15, 10) as plain:
        yield index, plain


def _check(al, index, table, q_len, chains, slack, max_tl, in_place, status=True):
    dev = torch.device("cuda", 0)
    n = len(q_len)
    a_start, at, aq, al_ = cc.csr(chains)
    total = len(at)
    want = gtb.locate_window_contigs(*table, q_len, a_start, at, aq, al_, slack, max_tl)
    g = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    new = lambda size, dt=torch.int32: torch.full((size + PAD,), CANARY, dtype=dt, device=dev)  # noqa: E731
    t_in = new(total)
    t_in[:total] = g(at)
    full = [new(n, torch.int64), new(n), t_in if in_place else new(total), new(n), new(n)]
    out = (full[0][:n], full[1][:n], full[2][:total], full[3][:n] if status else None, full[4][:n])
    got = al.locate_window_contigs_device(index, g(np.asarray(q_len, np.int32)), g(a_start), t_in[:total], g(aq), g(al_), slack, max_tl, out=out)
    torch.cuda.synchronize()
    assert got is out
    got = [x.cpu().numpy() for x in full]
    exp_t = np.array([(int(at[i]) if in_place else CANARY) if v is None else v for i, v in enumerate(want[2])] + [CANARY] * PAD, np.int64)
    tail = [CANARY] * PAD
    exp = [np.array(want[0] + tail), np.array(want[1] + tail), exp_t, np.array((want[3] if status else [CANARY] * n) + tail), np.array(want[4] + tail)]
    for name, a, b in zip(("t_start", "t_len", "anchor_t", "status", "rid"), got, exp):
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, (name, bad[:8], a[bad[:8]], b[bad[:8]])
    if not in_place:
        assert (t_in.cpu().numpy()[:total] == at).all()
    return want


@pytest.mark.parametrize("in_place", [False, True])
def test_hand_made_chains(aligner, indexes, in_place):
    index, plain = indexes
    start, length, slack, max_tl, cases = cc.locate_cases()
    table = (start, length)
    q_len, chains = [c[1] for c in cases], [c[2] for c in cases]
    want = _check(aligner, index, table, q_len, chains, slack, max_tl, in_place)
    assert want[3] == [c[3] for c in cases] and want[0] == [c[4] for c in cases] and want[1] == [c[5] for c in cases] and want[4] == [c[6] for c in cases]
    _check(aligner, index, table, q_len, chains, slack, max_tl, in_place, status=False)
    _check(aligner, index, table, q_len, chains, 0, max_tl, in_place)
    # refused reads at the front, in the middle and at the end
    order = [5, 0, 1, 9, 6, 2, 8, 3, 11, 4, 10, 7]
    want = _check(aligner, index, table, [q_len[i] for i in order], [chains[i] for i in order], slack, max_tl, in_place)
    assert want[3][0] == want[3][-1] == gtb.BAD_ARG and want[4][0] == want[4][-1] == -1
    # no contigs: the whole buffer is one, and the result is the plain stage's
    want = _check(aligner, plain, ([0], [3502]), q_len, chains, slack, max_tl, in_place)
    a_start, at, aq, al_ = cc.csr(chains)
    assert list(want[:4]) == list(itb.locate_window(3502, q_len, a_start, at, aq, al_, slack, max_tl)) and set(want[4]) == {0, -1}


@pytest.mark.parametrize("in_place", [False, True])
def test_long_chains_many_reads_and_empty_batches(aligner, indexes, in_place):
    index, _ = indexes
    start, length, _, _, _ = cc.locate_cases()
    table = (start, length)
    rng = np.random.default_rng(1025)
    # chains of 63 .. 130 anchors inside contig 1; one of them with ONE anchor (the last of the second 64) in contig 2
    chains, q_len = [], []
    for k in (63, 64, 65, 128, 130, 130):
        chains.append([(1100 + 10 * i, 5 + 10 * i, 7) for i in range(k)])
        q_len.append(10 * k + 20)
    chains[5][127] = (3100, chains[5][127][1], 7)
    want = _check(aligner, index, table, q_len, chains, 30, 2000, in_place)
    assert want[3] == [0] * 5 + [gtb.BAD_ARG] and want[4] == [1] * 5 + [-1]
    # more reads than a grid step, one anchor each, anywhere in the buffer
    n = 1025
    q_len = rng.integers(50, 400, n).tolist()
    chains = [[(int(rng.integers(-3, 3500)), int(rng.integers(0, ql - 20)), int(rng.integers(1, 21)))] for ql in q_len]
    chains[7] = []
    want = _check(aligner, index, table, q_len, chains, 150, 600, in_place)
    assert {0, gtb.BAD_ARG, gtb.UNSUPPORTED} == set(want[3]) and set(want[4]) == {-1, 0, 1, 2} and want[4][7] == -1
    _check(aligner, index, table, [100, 200, 0], [[], [], []], 10, 600, in_place)
    _check(aligner, index, table, [], [], 10, 600, in_place)
