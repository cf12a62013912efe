"""Reads in, positions and CIGARs out (map_reads_device): the index of the whole reference -> seeds of both orientations -> chains of the
2n rows -> the strand -> the window -> the alignment on the reference in place, on a stream of its own with one synchronisation at the
end.  Every array of every stage against the textbook composition (tests/index_textbook.py: map_reads), the alignment against
align_chain_device fed the textbook's windows, oriented reads and rebased anchors from the host.  The 16 reads of
tests/index_cases.py (tests/test_index_textbook.py proves the textbook maps them) and one short read of unrelated sequence."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import index_cases as ic  # noqa: E402
import seed_cases as cases  # noqa: E402
from mgl_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

GATK = (200, -150, 260, 11)
UNRELATED = cases.rand_seq(np.random.default_rng(2), 120)  # (a seed at which it shares no minimizer with the reference at either (k, w))


@pytest.fixture(scope="module")
def aligner():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mgl_amd import smithwaterman as sw

    a = sw.MicrosoftSmithWaterman(0)
    assert a.load()
    yield a
    a.close()


def _same(name, got, want, upto=None):
    got = got.cpu().numpy()
    want = np.asarray(want)
    upto = len(want) if upto is None else upto
    bad = np.flatnonzero(got[:upto] != want[:upto])
    assert bad.size == 0, (name, bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("k,w", [(15, 10), (11, 5)])
def test_the_pipeline_equals_the_textbook_composition_stage_by_stage(aligner, k, w):
    from mgl_amd.smithwaterman import _pack_pairs

    dev = torch.device("cuda", 0)
    ref, reads, truth, (seeded, chained, chosen, located, fed) = ic.mapped(k, w, (UNRELATED,))
    n = len(reads)
    assert n == 17 and chained[0][32] == chained[0][34] and chosen[2][16] == chosen[2][17]  # the unrelated read has a chain on neither row
    _, packed, _ = _pack_pairs(reads, reads, dev, None, False)
    max_ql = packed[7]
    stride = 2 * max(ic.MAX_TL, max_ql)
    align = dict(to_query_end=True, cigar_stride=stride, sides=True)
    stages = dict(ic.SEEDING, **ic.CHAINING)
    index = aligner.build_index(ref, k, w)
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            seeds, chain, choice, window, got = aligner.map_reads_device(index, *packed[3:6], ic.MAX_TL, max_ql, 64, -1, GATK, slack=ic.SLACK, strands=2, **stages,
                                                                         **align)
        torch.cuda.synchronize()  # the one synchronisation: nothing above waited for the device

        # ---- every stage's arrays
        total = seeded[0][-1]
        for name, g, t in zip(("cand_start", "cand_t", "cand_q", "cand_len", "row_t_len", "row_q_len", "seed status"), seeds,
                              seeded[:4] + (seeded[5], seeded[6], seeded[4])):
            _same(name, g, t, total if name in ("cand_t", "cand_q", "cand_len") else None)
        chain_total = chained[0][-1]
        for name, i in (("chain_start", 0), ("chain_t", 1), ("chain_q", 2), ("chain_len", 3), ("chain score", 4), ("chain status", 7)):
            _same(name, chain[i], chained[i], chain_total if i in (1, 2, 3) else None)
        anchors = chosen[2][-1]
        reads_out, q_start, q_len = choice[1].cpu().numpy(), packed[4].cpu().numpy(), packed[5].cpu().numpy()
        want_reads = np.frombuffer(chosen[1], np.uint8)
        assert all((reads_out[a:a + m] == want_reads[a:a + m]).all() for a, m in zip(q_start, q_len))
        for name, i in (("strand", 0), ("anchor_start", 2), ("anchor_t", 3), ("anchor_q", 4), ("anchor_len", 5), ("chosen score", 6), ("choice status", 7)):
            _same(name, choice[i], chosen[i], anchors if i in (3, 4, 5) else None)
        assert chosen[0] == [s for _, _, s in truth] + [0] and chosen[7] == [0] * 17
        _same("t_start", window[0], located[0])
        _same("t_len", window[1], located[1])
        _same("rebased anchor_t", window[2], located[2], anchors)
        _same("window status", window[3], located[3])
        assert located[3] == [0] * 17 and (located[0][16], located[1][16]) == (0, 0)

        # ---- the alignment: align_chain_device fed the textbook's windows, oriented reads and rebased anchors from the host
        g = lambda x, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=dt))).to(dev)  # noqa: E731
        _, oriented, _ = _pack_pairs([f[0] for f in fed], [f[0] for f in fed], dev, None, False)
        flat = np.asarray([a for f in fed for a in f[3]], dtype=np.int32).reshape(-1, 3)
        want = aligner.align_chain_device(g(np.frombuffer(ref, np.uint8).copy(), np.uint8), g(located[0], np.int64), g(located[1], np.int32), *oriented[3:6],
                                          g(chosen[2], np.int64), g(flat[:, 0], np.int32), g(flat[:, 1], np.int32), g(flat[:, 2], np.int32), ic.MAX_TL, max_ql,
                                          ic.CHAINING["max_dist"], ic.CHAINING["max_dist"], 64, -1, GATK, **align)
        torch.cuda.synchronize()
        got, want = [None if x is None else x.cpu().numpy() for x in got], [None if x is None else x.cpu().numpy() for x in want]
        assert len(got) == len(want) == 7
        for i, (a, b) in enumerate(zip(got, want)):
            assert (a is None) == (b is None)
            if a is None:
                continue
            if i == 4:
                a, b = a.reshape(n, -1), b.reshape(n, -1)
                assert all((a[p, :got[5][p]] == b[p, :got[5][p]]).all() for p in range(16))
            elif i in (0, 1, 2, 5):
                assert (a[:16] == b[:16]).all(), i  # (what a refused pair's record holds is not defined)
            else:
                assert (a == b).all(), i
        assert got[6].tolist() == [0] * 16 + [_lib.ERR_BAD_ARG]
        # the alignments lie where the reads come from: within the slack of the true span's ends
        rec, t_start = got[0][:16], np.asarray(located[0][:16])
        pos, length = np.array([t[0] for t in truth]), np.array([t[1] for t in truth])
        assert (np.abs(t_start + rec[:, 1] - pos) <= ic.SLACK).all() and (np.abs(t_start + rec[:, 2] - pos - length) <= ic.SLACK).all()

        # ---- over lists
        res = aligner.map_reads(index, reads, 64, -1, GATK, slack=ic.SLACK, strands=2, max_tl=ic.MAX_TL, **stages, to_query_end=True)
        assert res.status.tolist() == [0] * 16 + [_lib.ERR_BAD_ARG] and res.strand.tolist() == chosen[0]
        assert (res.ref_beg[:16] == t_start + rec[:, 1]).all() and (res.ref_end[:16] == t_start + rec[:, 2]).all() and (res.score[:16] == rec[:, 0]).all()
        assert res.ref_beg[16] == res.ref_end[16] == res.score[16] == 0 and res.cigars[16] == ""
        cg = got[4].reshape(n, -1)
        assert all(res.cigars[p] == cg[p, :got[5][p]].tobytes().decode() for p in range(16))
    finally:
        index.close()
