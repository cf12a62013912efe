"""formats.write_sam_all / write_paf_all from a hand-built AllMapResult: FLAGs, soft clips and tp tags per line, SA exactly on the
non-secondary lines of reads with two or more of them and listing the others, reference_under_read rebuilding the reference under
EVERY line (secondaries included), PAF's columns per line; and write_sam on a DescribedMapResult still writes what it wrote, compared
with a string built here."""
from mgl_amd import formats, synth
from mgl_amd.smithwaterman import AllMapResult, DescribedMapResult, Line

REF = (b"TTGACCAGTACGGATCCATGCAAGTCTAGGCTAACGTTAGC" b"NNNN" b"GATTACAGATTACACCGGTTAACCGGTATGCATGCAAT")
CONTIG = [("c0", 0, 41), ("c1", 45, 38)]


def _line(contig, beg, end, strand, cigar, q_beg, q_end, flag, mapq, parent, nm, n_match, md, xcigar, score=100):
    return Line(beg, end, strand, score, cigar, q_beg, q_end, flag, mapq, parent, nm, n_match, n_match + nm, md, xcigar, contig, CONTIG[contig][0], 0)


def _case():
    c0, c1 = REF[0:41], REF[45:83]
    # read 0, a chimera: c0[2:14] then c1[5:17], with a mismatch in its second part (c1[9] T -> C)
    part2 = bytearray(c1[5:17])
    part2[4] = ord("C")
    r0 = c0[2:14] + bytes(part2)
    first = _line(0, 2, 14, 0, "12M", 0, 12, 0, 60, 0, 0, 12, b"12", "12=")
    second = _line(1, 5, 17, 0, "12M", 12, 24, 0x800, 47, 1, 1, 11, b"4" + c1[9:10] + b"7", "4=1X7=", score=80)
    # read 1, strand 1 with a deletion: the oriented read is c0[20:26] + c0[28:36]; and a secondary copy of its first six bases
    ori = c0[20:26] + c0[28:36]
    r1 = synth.revcomp(ori)
    prim = _line(0, 20, 36, 1, "6M2D8M", 0, 14, 0x10, 0, 0, 2, 14, b"6^" + c0[26:28] + b"8", "6=2D8=")
    sec = _line(0, 20, 26, 1, "6M", 0, 6, 0x110, 0, 0, 0, 6, b"6", "6=", score=30)
    # read 2: unmapped
    r2 = b"ACGTACGT"
    return [r0, r1, r2], AllMapResult([2, 2, 0], [[first, second], [prim, sec], []])


def test_sam_lines_flags_clips_tags_and_sa(tmp_path):
    reads, result = _case()
    names = ["r0", "r1", "r2"]
    path = str(tmp_path / "all.sam")
    formats.write_sam_all(path, [c[0] for c in CONTIG], [c[2] for c in CONTIG], names, reads, ["I" * 23 + "5", None, "#" * 8], result)
    text = open(path).read()
    assert text.startswith(formats.sam_header(["c0", "c1"], [41, 38]))
    rows = [x.split("\t") for x in text.splitlines() if not x.startswith("@")]
    assert [(r[0], int(r[1]), r[2], int(r[3]), int(r[4]), r[5]) for r in rows] == [
        ("r0", 0, "c0", 3, 60, "12M12S"), ("r0", 0x800, "c1", 6, 47, "12S12M"), ("r1", 0x10, "c0", 21, 0, "6M2D8M"), ("r1", 0x110, "c0", 21, 0, "6M8S"),
        ("r2", 4, "*", 0, 0, "*")]
    tags = [{t[:4]: t[5:] for t in r[11:]} for r in rows]
    assert [t.get("tp:A") for t in tags] == ["P", "P", "P", "S", None]
    # SA: on the two lines of the chimera, each naming the other; the read with one non-secondary line has none
    assert tags[0]["SA:Z"] == "c1,6,+,12S12M,47,1;" and tags[1]["SA:Z"] == "c0,3,+,12M12S,60,0;" and "SA:Z" not in tags[2] and "SA:Z" not in tags[3]
    assert [t.get("NM:i") for t in tags[:4]] == ["0", "1", "2", "0"] and [t.get("AS:i") for t in tags[:4]] == ["100", "80", "100", "30"]
    # SEQ and QUAL are oriented on every line
    assert rows[0][9] == rows[1][9] == reads[0].decode() and rows[0][10] == "I" * 23 + "5"
    assert rows[2][9] == rows[3][9] == synth.revcomp(reads[1]).decode() and rows[2][10] == "*"
    assert rows[4][9] == reads[2].decode() and rows[4][10] == "#" * 8 and len(rows[4]) == 11
    # the reference under EVERY line
    _, refs, recs = formats.read_sam(path)
    assert refs == [("c0", 41), ("c1", 38)] and len(recs) == 5
    for rec, (contig, beg, end) in zip(recs, [(0, 2, 14), (1, 5, 17), (0, 20, 36), (0, 20, 26)]):
        start = CONTIG[contig][1]
        assert formats.reference_under_read(rec)[0] == REF[start + beg:start + end] and rec.pos == beg
    # the = / X form
    formats.write_sam_all(path, ["c0", "c1"], [41, 38], names, reads, None, result, extended=True)
    rows = [x.split("\t") for x in open(path).read().splitlines() if not x.startswith("@")]
    assert [r[5] for r in rows] == ["12=12S", "12S4=1X7=", "6=2D8=", "6=8S", "*"] and "SA:Z:c1,6,+,12S4=1X7=,47,1;" in rows[0]


def test_a_reverse_strand_line_reverses_the_qualities(tmp_path):
    reads, result = _case()
    path = str(tmp_path / "q.sam")
    formats.write_sam_all(path, ["c0", "c1"], [41, 38], ["r0", "r1", "r2"], reads, [None, "ABCDEFGHIJKLMN", None], result)
    rows = [x.split("\t") for x in open(path).read().splitlines() if not x.startswith("@")]
    assert rows[2][10] == rows[3][10] == "NMLKJIHGFEDCBA"


def test_paf_columns_per_line(tmp_path):
    reads, result = _case()
    path = str(tmp_path / "all.paf")
    formats.write_paf_all(path, ["c0", "c1"], [41, 38], ["r0", "r1", "r2"], reads, result)
    rows = [x.split("\t") for x in open(path).read().splitlines()]
    assert [r[:12] for r in rows] == [
        ["r0", "24", "0", "12", "+", "c0", "41", "2", "14", "12", "12", "60"], ["r0", "24", "12", "24", "+", "c1", "38", "5", "17", "11", "12", "47"],
        ["r1", "14", "0", "14", "-", "c0", "41", "20", "36", "14", "16", "0"], ["r1", "14", "8", "14", "-", "c0", "41", "20", "26", "6", "6", "0"]]
    assert [r[12:] for r in rows] == [["NM:i:0", "AS:i:100", "tp:A:P", "cg:Z:12M"], ["NM:i:1", "AS:i:80", "tp:A:P", "cg:Z:12M"],
                                      ["NM:i:2", "AS:i:100", "tp:A:P", "cg:Z:6M2D8M"], ["NM:i:0", "AS:i:30", "tp:A:S", "cg:Z:6M"]]


def test_one_reference_sequence_needs_no_rid(tmp_path):
    line = Line(2, 14, 0, 100, "12M", 0, 12, 0, 60, 0, 0, 12, 12, b"12", None, None, None, 0)
    path = str(tmp_path / "one.sam")
    formats.write_sam_all(path, "ref", 83, ["r"], [REF[2:14]], None, AllMapResult([1], [[line]]))
    assert open(path).read().splitlines()[-1] == "\t".join(["r", "0", "ref", "3", "60", "12M", "*", "0", "0", REF[2:14].decode(), "*", "NM:i:0", "MD:Z:12", "AS:i:100",
                                                             "tp:A:P"])


def test_write_sam_of_a_described_result_is_what_it_was(tmp_path):
    import numpy as np

    a = lambda *v: np.asarray(v, np.int32)  # noqa: E731
    res = DescribedMapResult(a(2, 0), a(14, 0), a(1, 0), a(100, 0), ["12M", ""], a(0, 1), a(60, 0), a(1, 0), [[], []], a(2, 0), a(14, 0), a(1, 0), a(11, 0), a(12, 0),
                             [b"5A6", b""], None)
    read = synth.revcomp(b"AC" + REF[2:14])
    path = str(tmp_path / "d.sam")
    formats.write_sam(path, "ref", 83, ["x", "y"], [read, b"ACGT"], ["ABCDEFGHIJKLMN", None], res)
    want = ("@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:ref\tLN:83\n@PG\tID:mgl_amd\tPN:mgl_amd\n"
            "x\t16\tref\t3\t60\t2S12M\t*\t0\t0\t" + (b"AC" + REF[2:14]).decode() + "\tNMLKJIHGFEDCBA\tNM:i:1\tMD:Z:5A6\tAS:i:100\n"
            "y\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\t*\n")
    assert open(path).read() == want
