"""map_reads_pileup on the GPU: reads in, the pileup of their primary and supplementary lines out, on tests/pileup_map_cases.py's two
sets -- lines_cases' contig reads against an index of contigs, and synth.variant_mapping_set against a plain index.  The table
equals the textbook over the lines that map_reads_all returns, word for word; the planted variants come out of the device's sites
and nothing else does; two batches accumulated into one table equal one batch of both; a min_mapq above a line's removes exactly
that line's counts.  tests/test_pileup_pipeline.py shows the same of the CPU textbooks' composition."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import index_cases as ic  # noqa: E402
import pileup_map_cases as pm  # noqa: E402
import pileup_textbook as ptb  # noqa: E402
import rank_cases as rc  # noqa: E402

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


def _table(als, length):
    return np.asarray(ptb.pileup(als, 0, length), np.uint32)


def _same(a, b):
    return a.n_lines.tolist() == b.n_lines.tolist() and a.lines == b.lines


def test_the_variant_set_and_its_planted_truth(aligner):
    ref, reads, planted = pm.variant_set()
    stages = pm.variant_stages()
    index = aligner.build_index(ref, rc.K, rc.W)
    try:
        res, counts = aligner.map_reads_pileup(index, reads, pm.BAND, pm.ZDROP, pm.GATK, max_tl=ic.MAX_TL, **dict(stages))
        every = aligner.map_reads_all(index, reads, pm.BAND, pm.ZDROP, pm.GATK, max_tl=ic.MAX_TL, **dict(stages))
        assert _same(res, every) and res.n_lines.tolist() == [1] * len(reads)
        assert counts.shape == (8, len(ref)) and counts.dtype == np.uint32
        assert (counts == _table(pm.result_alignments(every, reads), len(ref))).all()
        # the device's sites over the device's table
        dev = torch.device("cuda", 0)
        call, flags, sites, ns = aligner.pileup_sites_device(torch.from_numpy(counts.view(np.int32)).to(dev), index.ref)
        torch.cuda.synchronize()
        total = int(ns[0])
        rows = sites.cpu().numpy()[:total]
        pm.assert_planted_truth(ref, planted, rows)
        want = ptb.sites(counts.tolist(), ref, 0, *pm.SITES)
        assert call.cpu().numpy().tobytes() == want[0] and flags.cpu().numpy().tolist() == want[1] and [tuple(r) for r in rows.tolist()] == [tuple(s) for s in want[2]]

        # ---- two batches accumulated into one table equal one batch of both
        _, first = aligner.map_reads_pileup(index, reads[:20], pm.BAND, pm.ZDROP, pm.GATK, max_tl=ic.MAX_TL, **dict(stages))
        table = torch.from_numpy(first.view(np.int32).copy()).to(dev)
        _, both = aligner.map_reads_pileup(index, reads[20:], pm.BAND, pm.ZDROP, pm.GATK, max_tl=ic.MAX_TL, counts=table, **dict(stages))
        assert (both == counts).all() and first.any() and not (first == counts).all()
        assert (table.cpu().numpy().view(np.uint32) == counts).all()  # the table given is the table added into

        # ---- a min_mapq above every line's leaves nothing; one above the least removes exactly those lines
        mapqs = sorted({ln.mapq for ls in every.lines for ln in ls})
        _, none = aligner.map_reads_pileup(index, reads, pm.BAND, pm.ZDROP, pm.GATK, max_tl=ic.MAX_TL, min_mapq=mapqs[-1] + 1, **dict(stages))
        assert not none.any()
        _, fewer = aligner.map_reads_pileup(index, reads, pm.BAND, pm.ZDROP, pm.GATK, max_tl=ic.MAX_TL, min_mapq=mapqs[0] + 1, **dict(stages))
        assert (fewer == _table(pm.result_alignments(every, reads, min_mapq=mapqs[0] + 1), len(ref))).all()
    finally:
        index.close()


def test_the_contig_reads_secondary_and_supplementary_lines(aligner):
    import contig_cases as cc
    import lines_cases as lc

    reads, _ = lc.contig_reads()
    contigs, _, _ = cc.pipeline_set()
    stages = dict(ic.SEEDING, **ic.CHAINING, **cc.RANKING, slack=ic.SLACK, strands=2, to_query_end=False)
    index = aligner.build_index_contigs(contigs, cc.K, cc.W)
    try:
        starts = index.contigs.starts
        length = int(index.info.ref_len)
        res, counts = aligner.map_reads_pileup(index, reads, cc.BAND, cc.ZDROP, cc.GATK, max_tl=ic.MAX_TL, **dict(stages))
        every = aligner.map_reads_all(index, reads, cc.BAND, cc.ZDROP, cc.GATK, max_tl=ic.MAX_TL, **dict(stages))
        assert _same(res, every) and counts.shape == (8, length)
        flags = [ln.flag for ls in every.lines for ln in ls]
        assert any(f & 0x100 for f in flags) and any(f & 0x800 for f in flags)  # a secondary line, which is not counted, and a supplementary one, which is
        assert (counts == _table(pm.result_alignments(every, reads, starts), length)).all() and counts.any()
        # the CPU textbooks' composition gives the same table (tests/test_pileup_pipeline.py)
        tb = pm.contig_piled()
        m = min(len(tb[0]), length)
        assert (counts[:, :m] == np.asarray(tb[6], np.uint32)[:, :m]).all() and not counts[:, m:].any()
        # min_mapq: the lines below it, and exactly those, are gone
        mapqs = sorted({ln.mapq for ls in every.lines for ln in ls if not ln.flag & 0x100})
        assert len(mapqs) >= 2
        _, fewer = aligner.map_reads_pileup(index, reads, cc.BAND, cc.ZDROP, cc.GATK, max_tl=ic.MAX_TL, min_mapq=mapqs[0] + 1, **dict(stages))
        assert (fewer == _table(pm.result_alignments(every, reads, starts, min_mapq=mapqs[0] + 1), length)).all() and not (fewer == counts).all()
    finally:
        index.close()
