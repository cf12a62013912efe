"""Reads in, SAM out (map_reads_described_device, map_reads_described, formats.write_sam): map_reads_ranked_device with the describing
stage behind it, on a stream of its own with one synchronisation at the end.  The six existing tuples against map_reads_ranked_device's
on the same inputs, the seventh against the textbook composition (tests/describe_map_cases.py), at divergence 0 and 0.01, with
to_query_end true and false; the SAM written from map_reads_described round-trips against the reference; the unrelated read is an
unmapped line."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import describe_map_cases as dmc  # noqa: E402
import describe_textbook as dtb  # noqa: E402
import index_cases as ic  # noqa: E402
import rank_cases as rc  # noqa: E402
from mgl_amd import _lib, formats, synth  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def aligner():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mgl_amd import smithwaterman as sw

    a = sw.MicrosoftSmithWaterman(0)
    assert a.load()
    yield a
    a.close()


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and bool((a == b).all())


@pytest.mark.parametrize("to_query_end", [True, False])
@pytest.mark.parametrize("divergence", [0.0, 0.01])
def test_the_described_pipeline(aligner, tmp_path, divergence, to_query_end):
    from mgl_amd.smithwaterman import _pack_pairs

    dev = torch.device("cuda", 0)
    ref, reads, names, want, descs = dmc.mapped(divergence, to_query_end)
    n = len(reads)
    _, packed, _ = _pack_pairs(reads, reads, dev, None, False)
    max_ql = packed[7]
    stride = 2 * max(ic.MAX_TL, max_ql)
    align = dict(to_query_end=to_query_end, cigar_stride=stride)
    stages = dict(ic.SEEDING, **ic.CHAINING)
    index = aligner.build_index(ref, rc.K, rc.W)
    try:
        # every output of the plain pipeline that is not written everywhere starts from zeros in both runs, so that the tuples compare whole
        plain = aligner.map_reads_ranked_device(index, *packed[3:6], ic.MAX_TL, max_ql, dmc.BAND, dmc.ZDROP, dmc.GATK, slack=ic.SLACK, strands=2, **stages,
                                                **align, **rc.RANKING)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            got = aligner.map_reads_described_device(index, *packed[3:6], ic.MAX_TL, max_ql, dmc.BAND, dmc.ZDROP, dmc.GATK, slack=ic.SLACK, strands=2,
                                                     **stages, **align, **rc.RANKING)
        torch.cuda.synchronize()  # the one synchronisation: nothing above waited for the device
        assert len(got) == 7 and len(plain) == 6
        ok = np.asarray(want.status) == 0

        # ---- the six existing tuples: what map_reads_ranked_device gives on the same inputs (compared where they are defined: the
        # alignment's rows of mapped reads up to their lengths, everything else as tests/test_gpu_map_reads_ranked.py compares it)
        ga, pa = [None if x is None else x.cpu().numpy() for x in got[4]], [None if x is None else x.cpu().numpy() for x in plain[4]]
        assert ga[6].tolist() == pa[6].tolist() == want.status.tolist()
        assert (ga[0][ok] == pa[0][ok]).all() and (ga[5][ok] == pa[5][ok]).all()
        gc, pc = ga[4].reshape(n, stride), pa[4].reshape(n, stride)
        assert all((gc[p, :ga[5][p]] == pc[p, :ga[5][p]]).all() for p in np.flatnonzero(ok))
        for t in (2, 3):  # the strand choice and the window
            for i, (x, y) in enumerate(zip(got[t], plain[t])):
                if (t, i) in ((2, 0), (2, 6), (2, 7), (3, 0), (3, 1), (3, 3)):
                    assert _same(x.cpu().numpy(), y.cpu().numpy()), (t, i)
        assert _same(got[5][0].cpu().numpy(), plain[5][0].cpu().numpy()) and _same(got[5][6].cpu().numpy(), plain[5][6].cpu().numpy())
        nc = got[5][0].cpu().numpy()
        gr, pr = got[5][1].cpu().numpy(), plain[5][1].cpu().numpy()
        assert all((gr[p, :nc[p]] == pr[p, :nc[p]]).all() for p in range(n))
        for t in (0, 1):  # the seed and chain stages: their counts, starts and statuses
            for i in ((0, 4, 5, 6) if t == 0 else (0, 4, 7)):
                assert _same(got[t][i].cpu().numpy(), plain[t][i].cpu().numpy()), (t, i)

        # ---- the seventh: the textbook on the textbook alignment
        stats, md, xc, dst = (x.cpu().numpy() for x in got[6])
        assert dst.tolist() == want.status.tolist()
        md, xc = md.reshape(n, -1), xc.reshape(n, -1)
        t_start = got[3][0].cpu().numpy()
        for p in range(n):
            if not ok[p]:
                assert not stats[p].any()
                continue
            d = descs[p]
            assert stats[p].tolist() == dtb.stats(d), p
            assert md[p, :stats[p, 6]].tobytes() == d.md and xc[p, :stats[p, 7]].tobytes().decode() == dtb.xcigar_text(d.xcigar), p
            assert gc[p, :ga[5][p]].tobytes().decode() == want.cigars[p]
            assert (t_start[p] + ga[0][p, 1], t_start[p] + ga[0][p, 2], ga[0][p, 3], ga[0][p, 4], ga[0][p, 0]) == (
                want.ref_beg[p], want.ref_end[p], want.q_beg[p], want.q_end[p], want.score[p]), p

        # ---- over lists, and the SAM written from them
        res = aligner.map_reads_described(index, reads, dmc.BAND, dmc.ZDROP, dmc.GATK, slack=ic.SLACK, strands=2, max_tl=ic.MAX_TL, extended=True, **stages,
                                          to_query_end=to_query_end, **rc.RANKING)
        for f in ("ref_beg", "ref_end", "strand", "score", "status", "mapq", "n_chains", "q_beg", "q_end", "nm", "n_match", "block_len"):
            assert np.asarray(getattr(res, f)).tolist() == np.asarray(getattr(want, f)).tolist(), f
        assert list(res.cigars) == want.cigars and list(res.xcigars) == want.xcigars and res.md == want.md and res.secondary == want.secondary
        assert aligner.map_reads_described(index, reads[:3], dmc.BAND, dmc.ZDROP, dmc.GATK, slack=ic.SLACK, strands=2, max_tl=ic.MAX_TL, **stages,
                                           to_query_end=to_query_end, **rc.RANKING).xcigars is None
        for extended in (False, True):
            path = tmp_path / ("out%d.sam" % extended)
            formats.write_sam(path, "ref1", len(ref), names, reads, None, res, extended=extended)
            _, refs, records = formats.read_sam(path)
            assert refs == [("ref1", len(ref))] and len(records) == n
            for p, rec in enumerate(records):
                if not ok[p]:
                    assert (rec.flag, rec.pos, rec.cigar, rec.seq) == (4, -1, [], reads[p]) and p == 8  # the unrelated read: an unmapped line
                    continue
                assert rec.flag == (16 if res.strand[p] else 0) and rec.seq == (synth.revcomp(reads[p]) if res.strand[p] else reads[p])
                under, edits = formats.reference_under_read(rec)
                span = sum(k for k, op in rec.cigar if op in "M=XD")
                assert under == ref[rec.pos:rec.pos + span] and edits == rec.tags["NM"] == res.nm[p] and rec.mapq == res.mapq[p]
        paf = tmp_path / "out.paf"
        formats.write_paf(paf, "ref1", len(ref), names, reads, res)
        assert len(open(paf).read().splitlines()) == int(ok.sum())
    finally:
        index.close()
