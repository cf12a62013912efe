"""formats.sam_header, write_sam and write_paf over a reference of contigs, without a GPU: the textbook composition of the pipeline
test (tests/contig_cases.py) written with lists of names and lengths -- one @SQ per contig, RNAME and POS of the read's own contig, the
reference under a read rebuilt from SEQ + CIGAR + MD equal to that contig's slice, the PAF's target columns -- and the form with ONE
name, which writes what it wrote before."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contig_cases as cc  # noqa: E402
from mgl_amd import formats, synth  # noqa: E402
from mgl_amd import smithwaterman as sw  # noqa: E402


def _result(kind=None):
    cols = cc.pipeline_described(True)
    kind = kind or sw.ContigDescribedMapResult
    arr = lambda f: np.asarray(cols[f], np.int64 if f in ("ref_beg", "ref_end") else np.int32)  # noqa: E731
    return kind(*[cols[f] if f in ("cigars", "secondary", "md", "xcigars", "rname") else arr(f) for f in kind._fields])


def test_one_sq_line_per_contig_and_every_record_rebuilds_its_contig(tmp_path):
    contigs, reads, _ = cc.pipeline_set()
    names, lens = [n for n, _ in contigs], [len(s) for _, s in contigs]
    res = _result()
    assert res._fields == sw.DescribedMapResult._fields + ("rid", "rname")
    header = formats.sam_header(names, lens)
    assert header.splitlines() == ["@HD\tVN:1.6\tSO:unsorted"] + ["@SQ\tSN:%s\tLN:%d" % x for x in zip(names, lens)] + ["@PG\tID:mgl_amd\tPN:mgl_amd"]
    read_names = ["read%d" % p for p in range(len(reads))]
    for extended in (False, True):
        path = tmp_path / ("out%d.sam" % extended)
        formats.write_sam(path, names, lens, read_names, reads, None, res, extended=extended)
        text, refs, records = formats.read_sam(path)
        assert text == header and refs == list(zip(names, lens)) and len(records) == 11
        seen = set()
        for p, r in enumerate(records):
            if res.status[p]:
                assert p == cc.UNRELATED_AT and (r.flag, r.ref_id, r.pos, r.cigar, r.seq) == (4, -1, -1, [], reads[p])
                continue
            assert (r.ref_id, r.pos, r.mapq) == (res.rid[p], res.ref_beg[p], res.mapq[p]) and r.flag == (16 if res.strand[p] else 0)
            under, edits = formats.reference_under_read(r)
            span = sum(k for k, op in r.cigar if op in "M=XD")
            assert span == res.ref_end[p] - res.ref_beg[p]
            assert under == contigs[r.ref_id][1][r.pos:r.pos + span] and edits == r.tags["NM"] == res.nm[p]
            assert r.seq == (synth.revcomp(reads[p]) if res.strand[p] else reads[p])
            seen.add(r.ref_id)
        assert seen == {0, 1, 2, 3}
    lines = open(tmp_path / "out0.sam").read().splitlines()[6:]
    assert [x.split("\t")[2:4] for x in lines[:3]] == [["contig0", "3001"], ["contig1", "1500"], ["contig1", "6500"]]
    assert lines[cc.EDGE].split("\t")[1:4] == ["16", "contig1", "21"]  # 20 bases into its contig, counted from 1


def test_paf_target_columns(tmp_path):
    contigs, reads, _ = cc.pipeline_set()
    names, lens = [n for n, _ in contigs], [len(s) for _, s in contigs]
    res = _result()
    path = tmp_path / "out.paf"
    formats.write_paf(path, names, lens, ["read%d" % p for p in range(len(reads))], reads, res)
    lines = [x.split("\t") for x in open(path).read().splitlines()]
    assert len(lines) == 10
    for p, c in enumerate(lines):
        assert c[0] == "read%d" % p and c[5:9] == [names[res.rid[p]], str(lens[res.rid[p]]), str(res.ref_beg[p]), str(res.ref_end[p])]
        assert int(c[8]) <= int(c[6]) and c[4] == "+-"[res.strand[p]]
    assert lines[cc.CHIMERA][5:9] == ["contig1", "9999", "0", "600"] and lines[7][5:7] == ["contig3", "19499"]


def test_the_form_with_one_name_is_unchanged(tmp_path):
    contigs, reads, _ = cc.pipeline_set()
    res = _result(sw.DescribedMapResult)  # (no rid: the one-name form never asks for it)
    n = len(reads)
    read_names = ["read%d" % p for p in range(n)]
    assert formats.sam_header("ref1", 1234) == "@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:ref1\tLN:1234\n@PG\tID:mgl_amd\tPN:mgl_amd\n"
    assert formats.sam_header(["ref1"], [1234]) == formats.sam_header("ref1", 1234)
    sam, paf = tmp_path / "one.sam", tmp_path / "one.paf"
    formats.write_sam(sam, "ref1", 50000, read_names, reads, None, res)
    formats.write_paf(paf, "ref1", 50000, read_names, reads, res)
    _, refs, records = formats.read_sam(sam)
    assert refs == [("ref1", 50000)] and all(r.ref_id == (0 if not res.status[p] else -1) and (res.status[p] or r.pos == res.ref_beg[p]) for p, r in enumerate(records))
    for c, p in zip([x.split("\t") for x in open(paf).read().splitlines()], range(10)):
        assert c[5:9] == ["ref1", "50000", str(res.ref_beg[p]), str(res.ref_end[p])]
    # the contig form with a result that has no rid says so
    with pytest.raises(ValueError):
        formats.write_sam(tmp_path / "bad.sam", ["a", "b"], [10, 20], read_names, reads, None, res)
    with pytest.raises(ValueError):
        formats.sam_header(["a", "b"], [10])
