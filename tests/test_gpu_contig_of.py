"""mgl_sw_index_build_contigs_device, mgl_sw_index_get_contigs and mgl_sw_index_contig_of_batch_device on the GPU against
tests/contig_textbook.py: tables of 1, 2, 4 096 (the last that is searched in LDS), 4 097 and 20 000 contigs, anchors at every edge of a
contig, no anchors, an index of the build without contigs, and a base in the first, a middle and the last gap."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contig_cases as cc  # noqa: E402
import contig_textbook as gtb  # noqa: E402
import index_textbook as itb  # noqa: E402
from mgl_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

PAD = 16
K, W = 15, 10


@pytest.fixture(scope="module")
def aligner():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mgl_amd import smithwaterman as sw

    a = sw.MicrosoftSmithWaterman(0)
    assert a.load()
    yield a
    a.close()


def _table(rng, count, lo, hi):
    """``count`` random contigs of lo .. hi bases with gaps of 1 or 2 -> (buffer, start, length)"""
    contigs = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), int(rng.integers(lo, hi + 1)))) for _ in range(count)]
    start, at, parts = [], 0, []
    for c, s in enumerate(contigs):
        start.append(at)
        gap = b"" if c == count - 1 else b"N" * int(rng.integers(1, 3))
        parts += [s, gap]
        at += len(s) + len(gap)
    return b"".join(parts), start, [len(s) for s in contigs]


def _anchors(rng, start, length, ref_len):
    """every edge of the first, the last and up to 300 other contigs, and 3 000 random anchors"""
    some = sorted({0, len(start) - 1, *rng.integers(0, len(start), 300).tolist()})
    edges = cc.contig_of_edges([start[c] for c in some], [length[c] for c in some])
    t = rng.integers(-3, ref_len + 3, 3000)
    return edges + list(zip(t.tolist(), rng.integers(0, 4, 3000).tolist()))


def _check(index, start, length, anchors):
    dev = torch.device("cuda", 0)
    total = len(anchors)
    t = torch.tensor([a[0] for a in anchors], dtype=torch.int32, device=dev)
    l = torch.tensor([a[1] for a in anchors], dtype=torch.int32, device=dev)
    full = torch.full((total + PAD,), cc.CANARY, dtype=torch.int32, device=dev)
    assert index.contig_of_device(t, l, out=full[:total]) is not None
    torch.cuda.synchronize()
    got = full.cpu().numpy()
    want = np.asarray([gtb.contig_of(start, length, *a) for a in anchors] + [cc.CANARY] * PAD, np.int64)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]], [anchors[i] for i in bad[:8] if i < total])
    return want[:total]


@pytest.mark.parametrize("count,lo,hi", [(1, 200, 200), (2, 50, 80), (4096, 1, 40), (4097, 1, 40), (20000, 1, 3)])
def test_tables_of_every_size(aligner, count, lo, hi):
    rng = np.random.default_rng(count)
    buffer, start, length = _table(rng, count, lo, hi)
    assert gtb.table_ok(len(buffer), start, length) and gtb.gaps_ok(buffer, start, length)
    with aligner.build_index_contigs_device(buffer, start, length, k=K, w=W) as index:
        s, n = index.get_contigs()
        assert s.tolist() == start and n.tolist() == length and index.contigs.names[-1] == "contig%d" % (count - 1)
        assert index.info.ref_len == len(buffer) and index.info.entries == len(itb.build_index(buffer, K, W))
        want = _check(index, start, length, _anchors(rng, start, length, len(buffer)))
        assert set(want.tolist()) >= {-1, 0, count - 1}
        _check(index, start, length, [])


def test_the_hand_table_and_an_index_without_contigs(aligner):
    start, length = cc.TABLE
    buffer = bytearray(b"ACGT" * 40)[:cc.TABLE_LEN]
    for c in range(3):
        for i in range(start[c] + length[c], start[c + 1]):
            buffer[i] = ord("N")
    buffer = bytes(buffer)
    edges = cc.contig_of_edges(start, length) + [(t, l) for t in range(-2, cc.TABLE_LEN + 3) for l in (1, 2, 3)]
    with aligner.build_index_contigs_device(buffer, start, length, ["a", "b", "c", "d"], k=K, w=W) as index:
        assert index.contigs.names == ["a", "b", "c", "d"]
        _check(index, start, length, edges)
    with aligner.build_index(buffer, K, W) as plain:  # ONE contig [0, ref_len)
        s, n = plain.get_contigs()
        assert (s.tolist(), n.tolist(), plain.contigs) == ([0], [cc.TABLE_LEN], None)
        _check(plain, [0], [cc.TABLE_LEN], edges)
    # the list form lays the contigs out itself
    pieces = [("x", b"ACGTACGTAC"), ("y", b"G"), ("z", b"TTTTT")]
    with aligner.build_index_contigs(pieces, k=K, w=W, gap=3) as index:
        s, n = index.get_contigs()
        assert (s.tolist(), n.tolist()) == ([0, 13, 17], [10, 1, 5]) and bytes(index.ref.cpu().numpy()) == b"ACGTACGTACNNNGNNNTTTTT"
        _check(index, [0, 13, 17], [10, 1, 5], [(t, l) for t in range(-1, 24) for l in (1, 2, 5, 6)])


def test_a_base_in_a_gap_refuses_the_build(aligner):
    rng = np.random.default_rng(3)
    buffer, start, length = _table(rng, 300, 5, 30)
    for c in (0, 150, 298):  # the first, a middle and the last gap; its last byte
        bad = bytearray(buffer)
        bad[start[c + 1] - 1] = ord("G")
        assert not gtb.gaps_ok(bytes(bad), start, length)
        with pytest.raises(_lib.MglSwError) as e:
            aligner.build_index_contigs_device(bytes(bad), start, length, k=K, w=W)
        assert e.value.status == _lib.ERR_BAD_ARG and "gap" in str(e.value)
    lower = bytearray(buffer)
    lower[start[1] - 1] = ord("g")  # no base to the seed stage
    aligner.build_index_contigs_device(bytes(lower), start, length, k=K, w=W).close()
    # the host's rules, with a GPU behind them
    for s, n in ((start, length[:-1] + [length[-1] - 1]), ([1] + start[1:], length), (start, [length[0] + (start[1] - start[0] - length[0])] + length[1:])):
        with pytest.raises(_lib.MglSwError) as e:
            aligner.build_index_contigs_device(buffer, s, n, k=K, w=W)
        assert e.value.status == _lib.ERR_BAD_ARG
