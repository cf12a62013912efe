"""Without a GPU: what tests/test_gpu_map_reads_pileup.py asserts of the device holds for the composition of the CPU textbooks on the
same inputs (tests/pileup_map_cases.py) -- lines_cases.compose extended by the pileup and sites textbooks, over lines_cases' contig
reads and over synth.variant_mapping_set, whose planted variants must come out as sites and nothing else."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import describe_textbook as dtb  # noqa: E402
import pileup_map_cases as pm  # noqa: E402
import pileup_textbook as ptb  # noqa: E402
from mgl_amd import formats  # noqa: E402


def test_the_contig_reads_pile_up_as_their_lines_say():
    buffer, start, length, names, reads, d, counts, (call, flags, sites) = pm.contig_piled()
    e, c = d["expanded"], d["classified"]
    als = pm.alignments(d, reads)
    counted = [j for j, job in enumerate(e.jobs) if job.read >= 0 and pm.selected(c.lines[j], d["aln_status"][j])]
    assert len(als) == len(counted) >= len(reads) - 1 and any(c.lines[j].flag & 0x800 for j in counted)       # supplementary lines are counted
    assert any(c.lines[j] is not None and c.lines[j].flag & 0x100 for j in range(e.n_jobs))                     # secondary ones are there, and are not
    # the table is the lines' descriptions added up
    want = [dtb.describe(buffer[pos:pos + sum(n for n, op in cg if op != "I")], q, cg) for pos, q, cg in als]
    assert sum(sum(counts[k]) for k in range(5)) == sum(w.n_match + w.n_mismatch for w in want)
    assert sum(counts[ptb.DEL]) == sum(w.n_del for w in want) and sum(counts[ptb.INS_BASES]) == sum(w.n_ins for w in want)
    # every mismatch of a line is a site of a table one deep, and the sites lie inside contigs
    mism = sum(counts[k][i] for i in range(len(buffer)) for k in range(5) if k != ptb.channel(buffer[i]))
    assert mism == sum(w.n_mismatch for w in want) > 0 and len(sites) > 0
    for s in sites:
        assert any(b <= s.pos < b + n for b, n in zip(start, length)), s
    # a mapq above a line's removes exactly that line's counts
    least = min(c.lines[j].mapq for j in counted)
    fewer = pm.alignments(d, reads, least + 1)
    gone = [a for a in als if a not in fewer]
    assert 0 < len(gone) == sum(c.lines[j].mapq == least for j in counted)
    minus = ptb.pileup(fewer, 0, len(buffer))
    assert ptb.pileup(gone, 0, len(buffer), [list(r) for r in minus]) == counts


def test_the_planted_variants_are_the_sites():
    ref, reads, planted, d, counts, (call, flags, sites) = pm.variant_piled()
    assert d["classified"].n_lines == [1] * len(reads)                                   # every read maps, once
    pm.assert_planted_truth(ref, planted, sites)
    depth = [sum(counts[k][i] for k in range(6)) for i in range(len(ref))]
    assert set(depth[1000:7000]) == {8} and max(depth) == 8                              # a read every 125 bases, 1 000 long
    # the call is the donor: the reference with the planted substitutions, and a * over the deletion
    donor = bytearray(ref)
    for kind, pos, what in planted:
        if kind == "X":
            donor[pos] = what[0]
        elif kind == "D":
            donor[pos:pos + len(what)] = b"*" * len(what)
    assert call[1000:7000] == bytes(donor[1000:7000])
    ins = [v for v in planted if v[0] == "I"][0]
    assert counts[ptb.INS][ins[1]] == 8 and counts[ptb.INS_BASES][ins[1]] == 8 * len(ins[2])


def test_two_batches_accumulate_to_one():
    ref, reads, planted, d, counts, _ = pm.variant_piled()
    als = pm.alignments(d, reads)
    half = ptb.pileup(als[:20], 0, len(ref))
    assert ptb.pileup(als[20:], 0, len(ref), half) == counts


def test_write_sites(tmp_path):
    import numpy as np

    ref, reads, planted, d, counts, (call, flags, sites) = pm.variant_piled()
    path = str(tmp_path / "sites.tsv")
    formats.write_sites(path, "chr", len(ref), np.asarray(sites, np.int32), np.asarray(counts, np.uint32))
    rows = [r.split("\t") for r in open(path).read().splitlines()]
    assert rows[0][0] == "#contig" and len(rows) == 1 + len(sites) and all(len(r) == 14 for r in rows)
    for r, s in zip(rows[1:], sites):
        assert r[0] == "chr" and int(r[1]) == s.pos + 1 and r[2] == chr(ref[s.pos]) and r[3] == chr(call[s.pos]) and int(r[4]) == s.depth
        assert [int(v) for v in r[5:13]] == [counts[k][s.pos] for k in range(8)] and int(r[13]) == s.flags
    # contigs: a site's position counts from its contig's start
    formats.write_sites(path, ["a", "b"], [3000, 5000], np.asarray(sites, np.int32), np.asarray(counts, np.uint32), starts=[0, 3000])
    rows = [r.split("\t") for r in open(path).read().splitlines()][1:]
    assert [(r[0], int(r[1])) for r in rows] == [("a", s.pos + 1) if s.pos < 3000 else ("b", s.pos - 2999) for s in sites]
