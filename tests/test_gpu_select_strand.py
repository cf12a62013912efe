"""mgl_sw_select_strand_batch_device on the GPU against tests/strand_textbook.py (select_strand), bit for bit, on hand-made chain
arrays: the strands, the oriented reads (the output buffer is CANARY bytes beforehand: no byte outside a chosen read is written), the
anchors' prefix sum and copies, the scores and the statuses; canaries of 16 entries behind every array and in the anchor arrays from
d_anchor_start_out[n] on."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seed_cases as cases  # noqa: E402
import strand_textbook as stb  # noqa: E402
from mgl_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

PAD = 16
BYTE = 0xA5  # the canary of the byte buffer
NAMES = ("strand", "queries_out", "anchor_start", "anchor_t", "anchor_q", "anchor_len", "score", "status")


@pytest.fixture(scope="module")
def aligner():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mgl_amd import smithwaterman as sw

    a = sw.MicrosoftSmithWaterman(0)
    assert a.load()
    yield a
    a.close()


def _check(al, queries, q_start, q_len, chain_start, chain, score, absent=(), total=None):
    """chain: [(t, q, l)] over all rows.  One call into canaried arrays against the textbook -> the textbook's tuple"""
    dev = torch.device("cuda", 0)
    n = len(q_start)
    ct, cq, cl = ([c[i] for c in chain] for i in range(3))
    total = len(chain) if total is None else total
    want = stb.select_strand(queries, q_start, q_len, chain_start, ct, cq, cl, score, total_chain=total)
    g = lambda x, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=dt))).to(dev)  # noqa: E731
    sizes = (n, len(queries), n + 1, total, total, total, n, n)
    kinds = (torch.int32, torch.uint8, torch.int64, torch.int32, torch.int32, torch.int32, torch.int32, torch.int32)
    full = [torch.full((size + PAD,), BYTE if i == 1 else cases.CANARY, dtype=kind, device=dev) for i, (size, kind) in enumerate(zip(sizes, kinds))]
    views = tuple(None if i in absent else x[:size] for i, (x, size) in enumerate(zip(full, sizes)))
    qd = g(np.frombuffer(bytes(queries), np.uint8), np.uint8)
    # (the chain arrays as long as `total`, which may be below what the lists hold)
    al.select_strand_device(qd, g(q_start, np.int64), g(q_len, np.int32), g(chain_start, np.int64), g(ct, np.int32)[:total], g(cq, np.int32)[:total],
                            g(cl, np.int32)[:total], g(score, np.int32), out=views)
    torch.cuda.synchronize()
    got = [x.cpu().numpy() for x in full]
    k = want[2][-1]
    expect = [np.full(size + PAD, BYTE if i == 1 else cases.CANARY, got[i].dtype) for i, size in enumerate(sizes)]
    expect[0][:n], expect[2][:n + 1], expect[6][:n], expect[7][:n] = want[0], want[2], want[6], want[7]
    for i in (3, 4, 5):
        expect[i][:k] = want[i]
    # the textbook's buffer is 0 where no read was written: there the canary stays
    written = np.zeros(len(queries), bool)
    for p in range(n):
        if want[7][p] == 0:
            written[q_start[p]:q_start[p] + q_len[p]] = True
    expect[1][:len(queries)][written] = np.frombuffer(want[1], np.uint8)[written]
    for i, name in enumerate(NAMES):
        if i in absent:
            assert (got[i] == cases.CANARY).all(), name
        else:
            bad = np.flatnonzero(got[i] != expect[i])
            assert bad.size == 0, (name, bad[:8], got[i][bad[:8]], expect[i][bad[:8]])
    return want


def _reads(rng, lens, gap=(0, 1, 2, 3)):
    """reads of these lengths laid down with gaps, so that their starts run through every residue mod 4 -> (buffer, starts)"""
    buf, starts = bytearray(), []
    for i, n in enumerate(lens):
        buf += b"." * gap[i % len(gap)]
        starts.append(len(buf))
        buf += cases.rand_seq(rng, n, b"ACGTNacgtn")
    return bytes(buf) + b"..", starts


def test_ties_zeros_empty_rows_and_refused_pairs(aligner):
    rng = np.random.default_rng(51)
    lens = [9, 12, 7, 30, 5, 16, 11, 8, 6, 10]
    buf, starts = _reads(rng, lens)
    chain = [(int(rng.integers(0, 100)), int(rng.integers(0, 100)), int(rng.integers(1, 30))) for _ in range(24)]
    #        tie      both 0   row 1 empty  row 0 empty  rev wins  descends  fwd wins   leaves     ql = 0   score but no anchors
    cs = [0, 2, 4,    4, 4,    7, 7,        7, 9,        10, 13,   12, 13,   15, 17,    17, 17,    19, 20,  20, 24]
    score = [50, 50,  0, 0,    40, 99,      99, 3,       10, 11,   5, 6,     7, 6,      1, 2,      8, 9,    70, 80]
    lens[8] = 0
    starts[7] = len(buf) - 5  # the read leaves the buffer by 3 bytes
    want = _check(aligner, buf, starts, lens, cs, chain, score)
    assert want[0] == [0, 0, 0, 1, 1, 0, 0, 0, 0, 1] and want[7] == [0, 0, 0, 0, 0, 1, 0, 1, 1, 0]
    assert np.diff(want[2]).tolist() == [2, 0, 3, 2, 3, 0, 2, 0, 0, 4] and want[6] == [50, 0, 40, 3, 11, 0, 7, 0, 0, 80]
    for absent in ((6,), (7,), (6, 7)):
        _check(aligner, buf, starts, lens, cs, chain, score, absent=absent)
    # a range that leaves [0, total_chain] at its end, and a start below 0
    _check(aligner, buf, starts[:2], lens[:2], [0, 2, 4, 24, 25], chain, [5, 6, 7, 8])
    want = _check(aligner, buf, [-1, starts[1], len(buf) - 12], [9, 12, 12], [0, 2, 4, 4, 6, 6, 8], chain, [5, 6, 7, 8, 1, 9], total=8)
    assert want[7] == [1, 0, 0] and want[0] == [0, 1, 1]  # (the last read ends with the buffer)


def test_read_lengths_around_the_word_at_every_alignment_on_both_strands(aligner):
    rng = np.random.default_rng(52)
    lens, starts, buf = [], [], bytearray()
    for res in range(4):
        for m in (1, 2, 3, 4, 5, 63, 64, 65):
            buf += b"."  # (a byte between two reads that no read may touch)
            buf += b"." * ((res - len(buf)) % 4)
            starts.append(len(buf)), lens.append(m)
            buf += cases.rand_seq(rng, m, b"ACGTNacgtn")
    buf, n = bytes(buf) + b"...", len(lens)
    assert [s % 4 for s in starts] == [r for r in range(4) for _ in range(8)]
    chain = [(p, 2 * p, 3) for p in range(2 * n)]
    for pick in (0, 1):  # every read forward, then every read reversed
        score = [5 + (r % 2 == pick) for r in range(2 * n)]
        want = _check(aligner, buf, starts, lens, list(range(2 * n + 1)), chain, score)
        assert want[0] == [pick] * n and want[7] == [0] * n
    _check(aligner, buf, starts, lens, list(range(2 * n + 1)), chain, rng.integers(0, 3, 2 * n).tolist())


def test_1025_pairs_of_one_anchor_each_no_anchors_at_all_and_no_pairs(aligner):
    rng = np.random.default_rng(53)
    n = 1025
    lens = rng.integers(1, 9, n).tolist()
    buf, starts = _reads(rng, lens)
    chain = [(r, r + 1, 1 + r % 7) for r in range(2 * n)]
    # one anchor per row: K_p = 1 whatever the strand, so anchor_start[p] = p into the scan's second step
    want = _check(aligner, buf, starts, lens, list(range(2 * n + 1)), chain, rng.integers(0, 4, 2 * n).tolist())
    assert want[2] == list(range(n + 1)) and 300 < sum(want[0]) < 700
    # rows of 0 or 3 anchors, some pairs refused
    cs = np.concatenate([[0], np.cumsum(rng.choice([0, 3], 2 * n))]).tolist()
    chain = [(r, r + 1, 1 + r % 7) for r in range(cs[-1])]
    lens[1000] = 0
    _check(aligner, buf, starts, lens, cs, chain, rng.integers(0, 4, 2 * n).tolist())
    # total_chain = 0: every row empty, every read forward
    want = _check(aligner, buf, starts[:40], lens[:40], [0] * 81, [], [3, 4] * 40)
    assert want[0] == [0] * 40 and want[2] == [0] * 41 and want[7] == [0] * 40
    want = _check(aligner, buf, [], [], [0], chain[:5], [])
    assert want[2] == [0]
    assert _lib.ERR_BAD_ARG == 1
