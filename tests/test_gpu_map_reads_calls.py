"""map_reads_calls on the GPU: reads in, variant calls out, on tests/calls_map_cases.py's sets -- synth.diploid_variant_set with its
heterozygous variants at the even and at the odd indices, and the haploid synth.variant_mapping_set.  The calls equal the textbook
over the device's own table and lines record for record, their sequence rows included; every planted variant is exactly one call with
its genotype; the VCF written from them rebuilds both haplotypes.  tests/test_calls_pipeline.py shows the same of the CPU textbooks'
composition."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import calls_map_cases as cm  # noqa: E402
import calls_textbook as ctb  # noqa: E402
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


@pytest.mark.parametrize("which", cm.SETS)
def test_reads_in_calls_out(aligner, which, tmp_path):
    from mgl_amd import smithwaterman as sw

    ref, reads, planted, zygosity = cm.variant_set(which)
    stages = pm.variant_stages()
    index = aligner.build_index(ref, rc.K, rc.W)
    try:
        res, counts, calls = aligner.map_reads_calls(index, reads, pm.BAND, pm.ZDROP, pm.GATK, max_tl=ic.MAX_TL, max_ins=cm.MAX_INS, max_del=cm.MAX_DEL,
                                                     error_phred=cm.ERROR_PHRED, **dict(stages))
        assert res.n_lines.tolist() == [1] * len(reads) and counts.shape == (8, len(ref))
        # the textbooks over the device's own lines and table: sites, insertion rows, calls, sequence rows
        als = pm.result_alignments(res, reads)
        assert (counts == np.asarray(ptb.pileup(als, 0, len(ref)), np.uint32)).all()
        table = counts.tolist()
        sites = ptb.sites(table, ref, 0, *pm.SITES)[2]
        ins, want, rows = cm.called(als, table, sites, ref)
        assert calls == cm.host_calls(want, rows, ref) and len(calls) == len(planted)
        # the planted truth and the VCF
        cm.assert_planted_calls(ref, planted, zygosity, calls, cm.depth_of(which))
        assert all(c.gt == 2 for c in calls) or which != "haploid"
        cm.assert_vcf_rebuilds_the_haplotypes(str(tmp_path / "calls.vcf"), ref, planted, zygosity, calls)

        # ---- the device form: the raw records, rows and insertion table, word for word, with one synchronisation at the end
        dev = torch.device("cuda", 0)
        g = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
        q = np.frombuffer(b"".join(reads), np.uint8).copy()
        lens = np.asarray([len(r) for r in reads], np.int32)
        starts = np.concatenate([[0], np.cumsum(lens[:-1])]).astype(np.int64)
        out = aligner.map_reads_calls_device(index, g(q), g(starts), g(lens), ic.MAX_TL, int(lens.max()), pm.BAND, pm.ZDROP, pm.GATK, site_capacity=40,
                                             max_ins=cm.MAX_INS, max_del=cm.MAX_DEL, error_phred=cm.ERROR_PHRED, call_capacity=50, xcigar=False, **dict(stages))
        torch.cuda.synchronize()
        found, (got_ins, _), (got_calls, n_calls, got_seq) = out[9], out[10], out[11]
        total = int(found[3][0])
        assert total == len(sites) <= 40 and [tuple(r) for r in found[2].cpu().numpy()[:total].tolist()] == [tuple(s) for s in sites]
        assert got_ins.shape == (40, ctb.width(cm.MAX_INS)) and got_ins.cpu().numpy().view(np.uint32)[:total].tolist() == ins
        assert not got_ins.cpu().numpy()[total:].any()
        assert int(n_calls[0]) == len(want) and [tuple(r) for r in got_calls.cpu().numpy()[:len(want)].tolist()] == [tuple(c) for c in want]
        assert [bytes(r) for r in got_seq.cpu().numpy()[:len(want)]] == rows
        assert [sw.make_call(r, s, ref) for r, s in zip(got_calls.cpu().numpy()[:len(want)], got_seq.cpu().numpy())] == calls
    finally:
        index.close()


def test_more_sites_than_slots_is_an_error_of_the_list_form(aligner):
    from mgl_amd import _lib

    ref, reads, planted, _ = cm.variant_set("haploid")
    index = aligner.build_index(ref, rc.K, rc.W)
    try:
        with pytest.raises(_lib.MglSwError):
            aligner.map_reads_calls(index, reads, pm.BAND, pm.ZDROP, pm.GATK, max_tl=ic.MAX_TL, site_capacity=5, **pm.variant_stages())
    finally:
        index.close()
