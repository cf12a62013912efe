"""Reads in, positions, CIGARs and mapping qualities out (map_reads_ranked_device): map_reads_device with the ranking stage beside it, on a
stream of its own with one synchronisation at the end.  The five existing stages' tuples against map_reads_device's on the same inputs
(the alignment is unchanged), the records against the textbook composition (tests/rank_cases.py: repeat_mapped), on the eight reads of
DESIGN.md section 9k -- four of them with a second copy of their window in the reference, exact or at one per cent -- and one short read of
unrelated sequence."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import index_cases as ic  # noqa: E402
import rank_cases as rc  # noqa: E402
import seed_cases as cases  # noqa: E402
from mgl_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

GATK = (200, -150, 260, 11)
UNRELATED = cases.rand_seq(np.random.default_rng(2), 120)  # (it shares no minimizer with the reference: the textbook finds no candidate)


@pytest.fixture(scope="module")
def aligner():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mgl_amd import smithwaterman as sw

    a = sw.MicrosoftSmithWaterman(0)
    assert a.load()
    yield a
    a.close()


def _eq(name, a, b, upto=None):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    upto = len(a) if upto is None else upto
    assert a.shape == b.shape and (a[:upto] == b[:upto]).all(), name


@pytest.mark.parametrize("divergence", [0.0, 0.01])
def test_the_ranked_pipeline(aligner, divergence):
    from mgl_amd.smithwaterman import _pack_pairs

    dev = torch.device("cuda", 0)
    ref, reads, truth, copy, textbook, (nc, recs, _, _, _, _, rank_status) = rc.repeat_mapped(divergence, (UNRELATED,))
    seeded, chained, chosen = textbook[:3]
    n = len(reads)
    assert n == 9 and nc[8] == 0 and chosen[2][8] == chosen[2][9]  # the unrelated read has a chain on neither row
    _, packed, _ = _pack_pairs(reads, reads, dev, None, False)
    max_ql = packed[7]
    stride = 2 * max(ic.MAX_TL, max_ql)
    align = dict(to_query_end=True, cigar_stride=stride, sides=True)
    stages = dict(ic.SEEDING, **ic.CHAINING)
    index = aligner.build_index(ref, rc.K, rc.W)
    try:
        plain = aligner.map_reads_device(index, *packed[3:6], ic.MAX_TL, max_ql, 64, -1, GATK, slack=ic.SLACK, strands=2, **stages, **align)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            got = aligner.map_reads_ranked_device(index, *packed[3:6], ic.MAX_TL, max_ql, 64, -1, GATK, slack=ic.SLACK, strands=2, **stages, **align,
                                                  **rc.RANKING)
        torch.cuda.synchronize()  # the one synchronisation: nothing above waited for the device
        assert len(got) == 6 and len(plain) == 5

        # ---- the five existing stages: what map_reads_device gives on the same inputs
        total, chain_total, anchors = seeded[0][-1], chained[0][-1], chosen[2][-1]
        for i, name in enumerate(("cand_start", "cand_t", "cand_q", "cand_len", "row_t_len", "row_q_len", "seed status")):
            _eq(name, got[0][i], plain[0][i], total if i in (1, 2, 3) else None)
        assert plain[1][5] is None and plain[1][6] is None and got[1][5] is not None and got[1][6] is not None
        for i, name in ((0, "chain_start"), (1, "chain_t"), (2, "chain_q"), (3, "chain_len"), (4, "chain score"), (7, "chain status")):
            _eq(name, got[1][i], plain[1][i], chain_total if i in (1, 2, 3) else None)
        q_start, q_len = packed[4].cpu().numpy(), packed[5].cpu().numpy()
        a, b = got[2][1].cpu().numpy(), plain[2][1].cpu().numpy()
        assert all((a[s:s + m] == b[s:s + m]).all() for s, m in zip(q_start, q_len))
        for i, name in ((0, "strand"), (2, "anchor_start"), (3, "anchor_t"), (4, "anchor_q"), (5, "anchor_len"), (6, "chosen score"), (7, "choice status")):
            _eq(name, got[2][i], plain[2][i], anchors if i in (3, 4, 5) else None)
        for i, name in enumerate(("t_start", "t_len", "rebased anchor_t", "window status")):
            _eq(name, got[3][i], plain[3][i], anchors if i == 2 else None)
        ga, pa = [None if x is None else x.cpu().numpy() for x in got[4]], [None if x is None else x.cpu().numpy() for x in plain[4]]
        assert len(ga) == len(pa) == 7 and ga[6].tolist() == pa[6].tolist() == [0] * 8 + [_lib.ERR_BAD_ARG]
        for i, (x, y) in enumerate(zip(ga, pa)):
            assert (x is None) == (y is None)
            if x is None:
                continue
            if i == 4:
                x, y = x.reshape(n, -1), y.reshape(n, -1)
                assert all((x[p, :ga[5][p]] == y[p, :ga[5][p]]).all() for p in range(8))
            else:
                assert (x[:8] == y[:8]).all(), i  # (what a refused pair's record holds is not defined)
        assert (got[2][0].cpu().numpy() == np.asarray(chosen[0])).all() and chosen[0] == [s for _, _, s in truth] + [0]

        # ---- the records: the textbook composition's
        n_chains, rec, status = got[5][0].cpu().numpy(), got[5][1].cpu().numpy(), got[5][6].cpu().numpy()
        assert all(x is None for x in got[5][2:6]) and rec.shape == (9, 4, 12)
        assert n_chains.tolist() == nc == [2] * 4 + [1] * 4 + [0] and status.tolist() == rank_status == [0] * 9
        for p in range(9):
            assert [tuple(int(v) for v in rec[p, c]) for c in range(nc[p])] == [tuple(r) for r in recs[p]], p
        for p in range(4):
            first, second = recs[p]
            assert second.parent == 0 and copy[p][0] <= second.t_beg < second.t_end <= copy[p][0] + copy[p][1]
            if divergence == 0.0:
                assert first.mapq == 0 and second.score == first.score
            else:
                assert 0 < first.mapq < 60
        assert all(recs[p][0].mapq == 60 for p in range(4, 8))
        # the first chain is the one that was aligned: within the slack of the alignment on the reference
        t_start = got[3][0].cpu().numpy()
        for p in range(8):
            assert abs(t_start[p] + ga[0][p, 1] - recs[p][0].t_beg) <= ic.SLACK and abs(t_start[p] + ga[0][p, 2] - recs[p][0].t_end) <= ic.SLACK

        # ---- over lists
        res = aligner.map_reads_ranked(index, reads, 64, -1, GATK, slack=ic.SLACK, strands=2, max_tl=ic.MAX_TL, **stages, to_query_end=True, **rc.RANKING)
        base = aligner.map_reads(index, reads, 64, -1, GATK, slack=ic.SLACK, strands=2, max_tl=ic.MAX_TL, **stages, to_query_end=True)
        for f in ("ref_beg", "ref_end", "strand", "score", "status"):
            assert (getattr(res, f) == getattr(base, f)).all(), f
        assert all(res.cigars[p] == base.cigars[p] for p in range(9)) and res.status.tolist() == [0] * 8 + [_lib.ERR_BAD_ARG]
        assert res.mapq.tolist() == [r[0].mapq if r else 0 for r in recs] and res.n_chains.tolist() == nc
        assert res.secondary == [[(r.t_beg, r.t_end, r.strand, r.score, r.parent) for r in rs[1:]] for rs in recs]
        assert res.mapq[8] == 0 and res.n_chains[8] == 0 and res.secondary[8] == [] and res.ref_beg[8] == res.ref_end[8] == 0  # unmapped
    finally:
        index.close()
