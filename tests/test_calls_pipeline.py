"""Without a GPU: what tests/test_gpu_map_reads_calls.py asserts of the device holds for the composition of the CPU textbooks on the
same inputs (tests/calls_map_cases.py) -- pileup_map_cases' composition extended by the insertions and genotype textbooks, over
synth.diploid_variant_set with its heterozygous variants at the even and at the odd indices and over the haploid set: every planted
variant comes out as exactly one call with its genotype, and the VCF rebuilds both haplotypes."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import calls_map_cases as cm  # noqa: E402
import calls_textbook as ctb  # noqa: E402
import pileup_textbook as ptb  # noqa: E402
from mgl_amd import formats, synth  # noqa: E402


def test_the_diploid_set_and_its_truth():
    ref, reads, planted, zygosity = synth.diploid_variant_set(5, "even")
    assert (ref, reads[:56], planted) == synth.variant_mapping_set(5) and len(reads) == 113
    assert zygosity == [1, 2] * 6 and synth.diploid_variant_set(5, "odd")[3] == [2, 1] * 6 and synth.diploid_variant_set(5, "odd")[2] == planted
    hap_b = synth.apply_variants(ref, planted[1::2])
    starts = list(range(0, len(hap_b) - 1000 + 1, 125))
    assert len(starts) == 57 and all((synth.revcomp(r) if k % 2 else r) == hap_b[s:s + 1000] for k, (s, r) in enumerate(zip(starts, reads[56:])))
    with pytest.raises(ValueError):
        synth.diploid_variant_set(5, "both")
    assert synth.apply_variants(ref, planted) != hap_b != ref


@pytest.mark.parametrize("which", ["even", "odd"])
def test_the_planted_variants_are_the_calls_with_their_genotypes(which, tmp_path):
    ref, reads, planted, zygosity, d, counts, sites, ins, calls, rows = cm.composed_calls(which)
    assert d["classified"].n_lines == [1] * len(reads)                                  # every read maps, once
    assert len(sites) == 14 and sorted(s.pos for s in sites) == sorted(p + k for kind, p, what in planted for k in range(len(what) if kind == "D" else 1))
    host = cm.host_calls(calls, rows, ref)
    cm.assert_planted_calls(ref, planted, zygosity, host, 16)
    assert len(calls) == len(planted)                                                   # the three deleted positions are ONE call
    dele = [c for c in calls if c.kind == ctb.DELETION][0]
    inse = [c for c in calls if c.kind == ctb.INSERTION][0]
    het, hom = (dele, inse) if which == "even" else (inse, dele)
    assert (het.ref_count, het.alt_count, het.gt, (het.pl0, het.pl1, het.pl2), het.gq, het.qual) == (8, 8, 1, (150, 0, 150), 99, 150)
    assert (hom.ref_count, hom.alt_count, hom.gt, (hom.pl0, hom.pl1, hom.pl2), hom.gq, hom.qual) == (0, 16, 2, (396, 48, 0), 48, 396)
    # the insertion's row of the table: sixteen (or eight) insertions of two bases, their bases in the columns
    what = [v for v in planted if v[0] == "I"][0]
    row = ins[[s.pos for s in sites].index(what[1])]
    n = inse.alt_count
    assert row[2] == n and sum(row[:cm.MAX_INS + 1]) == n
    assert [row[cm.MAX_INS + 1 + 5 * j + ptb.channel(b)] for j, b in enumerate(what[2])] == [n, n] and sum(row[cm.MAX_INS + 1:]) == 2 * n
    cm.assert_vcf_rebuilds_the_haplotypes(str(tmp_path / "calls.vcf"), ref, planted, zygosity, host)


def test_on_the_haploid_set_every_call_is_homozygous(tmp_path):
    ref, reads, planted, zygosity, d, counts, sites, ins, calls, rows = cm.composed_calls("haploid")
    host = cm.host_calls(calls, rows, ref)
    assert len(calls) == len(planted) and all(c.gt == 2 and c.depth == 8 and c.ref_count == 0 for c in calls)
    cm.assert_planted_calls(ref, planted, zygosity, host, 8)
    records = cm.assert_vcf_rebuilds_the_haplotypes(str(tmp_path / "calls.vcf"), ref, planted, zygosity, host)
    assert all(r.gt == "1/1" for r in records)


def test_write_vcf_filters_anchors_and_contigs(tmp_path):
    from mgl_amd.smithwaterman import Call

    ref = b"ACGTACGTAC" + b"GGTTCCAAGG"
    pl = (50, 0, 60)
    calls = [Call(0, 2, 2, b"AC", b"", 9, 4, 5, 1, 50, 50, pl, 0),          # the contig's first bases deleted: anchored on the base behind
             Call(3, 1, 1, b"T", b"G", 9, 4, 5, 1, 50, 50, pl, 0),
             Call(5, 3, 2, b"", b"TT", 9, 0, 9, 2, 30, 40, (40, 30, 0), 0),
             Call(7, 1, 1, b"T", b"A", 9, 9, 0, 0, 30, 0, (0, 30, 90), 0),   # 0/0: left out
             Call(9, 3, 1, b"", b"A", 9, 4, 5, 1, 50, 50, pl, 0),            # behind the last base of contig a
             Call(12, 2, 3, b"TTC", b"", 9, 4, 5, 1, 50, 20, (20, 0, 60), 1)]
    path = str(tmp_path / "x.vcf")
    assert formats.write_vcf(path, ["a", "b"], [10, 10], ref, calls, starts=[0, 10], sample="s1") == 5
    header, rec = formats.read_vcf(path)
    assert [h for h in header if h.startswith("##contig")] == ["##contig=<ID=a,length=10>", "##contig=<ID=b,length=10>"] and header[-1].endswith("\ts1")
    assert [(r.chrom, r.pos, r.ref, r.alt, r.filter, r.gt) for r in rec] == [
        ("a", 0, b"ACG", b"G", "PASS", "0/1"), ("a", 3, b"T", b"G", "PASS", "0/1"), ("a", 5, b"C", b"CTT", "PASS", "1/1"), ("a", 9, b"C", b"CA", "PASS", "0/1"),
        ("b", 1, b"GTTC", b"G", "LongDel", "0/1")]
    assert rec[2].ad == (0, 9) and rec[2].pl == (40, 30, 0) and rec[2].gq == 30 and rec[2].dp == 9 and rec[2].qual == 40
    assert formats.write_vcf(path, ["a", "b"], [10, 10], ref, calls, starts=[0, 10], min_qual=41) == 3
    assert [r.qual for r in formats.read_vcf(path)[1]] == [50, 50, 50]
    with pytest.raises(ValueError):
        formats.write_vcf(path, ["a", "b"], [10, 10], ref, calls)
    # an insertion in front of a contig's first base stands behind a position outside it: anchored on the base behind
    gap = b"AAAA" + b"N" + b"CCCC"
    assert formats.write_vcf(path, ["a", "b"], [4, 4], gap, [Call(4, 3, 2, b"", b"GG", 9, 0, 9, 2, 30, 40, (40, 30, 0), 0)], starts=[0, 5]) == 1
    assert [(r.chrom, r.pos, r.ref, r.alt) for r in formats.read_vcf(path)[1]] == [("b", 0, b"C", b"GGC")]
