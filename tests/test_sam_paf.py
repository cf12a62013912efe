"""formats.write_sam / write_paf / read_sam without a GPU, on a DescribedMapResult made by hand from the textbooks
(tests/describe_map_cases.py): every mapped line's MD and CIGAR rebuild the reference under the read, NM is the edit count, SEQ and
QUAL are oriented, clips are written, an unmapped read is a flag-4 line, and PAF's columns hold.  The same file proves what the GPU
pipeline test (tests/test_gpu_map_reads_described.py) relies on: both strands, mismatches, insertions, deletions and clips occur."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import describe_map_cases as dmc  # noqa: E402
from mgl_amd import formats, synth  # noqa: E402

REF_NAME = "ref1"


def _quals(reads):
    return ["".join(chr(33 + (7 * k + p) % 40) for k in range(len(r))) for p, r in enumerate(reads)]


@pytest.mark.parametrize("extended", [False, True], ids=["MID", "=X"])
@pytest.mark.parametrize("to_query_end", [True, False])
@pytest.mark.parametrize("divergence", [0.0, 0.01])
def test_sam_round_trip(tmp_path, divergence, to_query_end, extended):
    ref, reads, names, res, _ = dmc.mapped(divergence, to_query_end)
    quals = _quals(reads)
    path = tmp_path / "out.sam"
    formats.write_sam(path, REF_NAME, len(ref), names, reads, quals, res, extended=extended)
    header, refs, records = formats.read_sam(path)
    assert header == formats.sam_header(REF_NAME, len(ref)) and refs == [(REF_NAME, len(ref))] and len(records) == len(reads)
    for p, (rec, read) in enumerate(zip(records, reads)):
        assert rec.name == names[p]
        if res.status[p]:
            assert (rec.flag, rec.ref_id, rec.pos, rec.mapq, rec.cigar, rec.seq, rec.tags) == (4, -1, -1, 0, [], read, {})
            assert rec.qual == bytes(ord(c) - 33 for c in quals[p])
            continue
        strand = int(res.strand[p])
        assert rec.flag == (16 if strand else 0) and rec.ref_id == 0 and rec.pos == res.ref_beg[p] and rec.mapq == res.mapq[p]
        assert rec.seq == (synth.revcomp(read) if strand else read)
        assert rec.qual == bytes(ord(c) - 33 for c in (quals[p][::-1] if strand else quals[p]))
        lead = rec.cigar[0][0] if rec.cigar[0][1] == "S" else 0
        trail = rec.cigar[-1][0] if rec.cigar[-1][1] == "S" else 0
        assert (lead, trail) == (res.q_beg[p], len(read) - res.q_end[p])
        assert all(n > 0 for n, _ in rec.cigar) and all(op != "S" for _, op in rec.cigar[1:-1])
        assert {op for _, op in rec.cigar} <= (set("=XIDS") if extended else set("MIDS"))
        assert sum(n for n, op in rec.cigar if op in "M=XIS") == len(read)
        under, edits = formats.reference_under_read(rec._replace(seq=rec.seq[lead:len(read) - trail], cigar=[e for e in rec.cigar if e[1] != "S"]))
        assert under == ref[rec.pos:rec.pos + (res.ref_end[p] - res.ref_beg[p])] and edits == rec.tags["NM"] == res.nm[p]
        assert formats.reference_under_read(rec) == (under, edits)  # the reader's own handling of clips
        assert rec.tags["AS"] == res.score[p] and set(rec.tags) == {"NM", "MD", "AS"}
    quiet = tmp_path / "noqual.sam"
    formats.write_sam(quiet, REF_NAME, len(ref), names, reads, None, res, extended=extended)
    assert all(r.qual == b"" for r in formats.read_sam(quiet)[2])


@pytest.mark.parametrize("extended", [False, True], ids=["MID", "=X"])
@pytest.mark.parametrize("to_query_end", [True, False])
def test_paf_columns(tmp_path, to_query_end, extended):
    ref, reads, names, res, descs = dmc.mapped(0.01, to_query_end)
    path = tmp_path / "out.paf"
    formats.write_paf(path, REF_NAME, len(ref), names, reads, res, extended=extended)
    lines = [ln.rstrip("\n").split("\t") for ln in open(path)]
    mapped = [p for p in range(len(reads)) if not res.status[p]]
    assert [c[0] for c in lines] == [names[p] for p in mapped]  # an unmapped read has no line
    for c, p in zip(lines, mapped):
        ql, strand = len(reads[p]), int(res.strand[p])
        assert len(c) == 15 and c[1] == str(ql) and c[4] == "-+"[strand == 0] and c[5] == REF_NAME and c[6] == str(len(ref))
        lo, hi = int(c[2]), int(c[3])
        oriented = synth.revcomp(reads[p]) if strand else reads[p]
        piece = reads[p][lo:hi]  # the interval is on the ORIGINAL strand
        assert (synth.revcomp(piece) if strand else piece) == oriented[res.q_beg[p]:res.q_end[p]] and 0 <= lo < hi <= ql
        assert (lo, hi) == ((ql - res.q_end[p], ql - res.q_beg[p]) if strand else (res.q_beg[p], res.q_end[p]))
        assert (int(c[7]), int(c[8])) == (res.ref_beg[p], res.ref_end[p])
        assert int(c[9]) == descs[p].n_match <= int(c[10]) == descs[p].n_match + res.nm[p] and int(c[11]) == res.mapq[p]
        assert c[12] == "NM:i:%d" % res.nm[p] and c[13] == "AS:i:%d" % res.score[p]
        assert c[14] == "cg:Z:" + (res.xcigars[p] if extended else res.cigars[p]) and "S" not in c[14][5:]
        els = formats.cigar_text_to_elements(c[14][5:])
        assert sum(n for n, op in els if op in "M=XD") == int(c[8]) - int(c[7]) and sum(n for n, op in els if op in "M=XI") == hi - lo
        assert sum(n for n, _ in els) == int(c[10])


@pytest.mark.parametrize("divergence", [0.0, 0.01])
def test_the_inputs_of_the_gpu_pipeline_test(divergence):
    for to_query_end in (True, False):
        ref, reads, names, res, descs = dmc.mapped(divergence, to_query_end)
        assert len(reads) == 11 and res.status.tolist() == [0] * 8 + [dmc.BAD_ARG, 0, 0] and reads[8] == dmc.UNRELATED
        good = [d for d in descs if d is not None]
        assert {int(s) for s, st in zip(res.strand, res.status) if not st} == {0, 1}
        assert any(d.n_mismatch for d in good) and any(d.n_ins for d in good) and any(d.n_del for d in good)
        clips = [(int(b), len(r) - int(e)) for b, e, r, st in zip(res.q_beg, res.q_end, reads, res.status) if not st]
        if to_query_end:
            assert clips == [(0, 0)] * 10
        else:  # the two reads with 30 bases of N cut onto their ends, strand 0 and strand 1; the others reach their ends here too
            assert clips == [(0, 0)] * 8 + [(0, 30), (30, 0)]


def test_an_extended_sam_needs_extended_cigars(tmp_path):
    ref, reads, names, res, _ = dmc.mapped(0.0, True)
    with pytest.raises(ValueError):
        formats.write_sam(tmp_path / "x.sam", REF_NAME, len(ref), names, reads, None, res._replace(xcigars=None), extended=True)
