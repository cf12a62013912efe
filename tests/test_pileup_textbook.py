"""tests/pileup_textbook.py, the definition of mgl_sw_pileup_alignments_batch_device and mgl_sw_pileup_sites_device (DESIGN.md section
9o), pinned without a GPU: by an independent restatement on describe_cases' sets, by describe_textbook's counts per alignment, by the
NM tags of the reference's own BAM fixture, and by hand cases worked out by hand."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import describe_cases as dc  # noqa: E402
import describe_textbook as dtb  # noqa: E402
import pileup_cases as pc  # noqa: E402
import pileup_textbook as ptb  # noqa: E402
from mgl_amd import formats  # noqa: E402

BAM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "HiSeq.1mb.1RG.2k_lines.bam")


def _sets():
    """describe_cases' seam, indel, offset and mixed sets and this module's own -> [(cases, t_start)]"""
    out = []
    for cases, gaps in ((dc.seam_cases(np.random.default_rng(1)), None), (dc.indel_cases(np.random.default_rng(2)), None),
                        dc.offset_cases(np.random.default_rng(3)), (dc.mixed_batch(np.random.default_rng(9), 60), None),
                        (pc.leading_insertions(np.random.default_rng(12)), None)):
        out.append((cases, dc.pack(cases, False, None, gaps)["t_start"]))
    return out


def test_the_two_statements_agree():
    for cases, t_start in _sets():
        als = pc.alignments(cases, t_start)
        end = int(max(int(s) + len(c.t) for c, s in zip(cases, t_start)))
        for beg, length in ((0, end + 2), (end // 3, max(end // 3, 1)), (5, 1)):
            assert ptb.pileup(als, beg, length) == ptb.pileup_by_columns(als, beg, length)
    # and adding to what stands
    als = pc.alignments(*_sets()[2])
    once = ptb.pileup(als, 0, 500)
    twice = ptb.pileup_by_columns(als, 0, 500, [list(row) for row in once])
    assert twice == [[2 * v for v in row] for row in once]


def test_ties_to_the_describe_textbook_per_alignment():
    seen_dropped = 0
    for cases, t_start in _sets():
        for c, s, on in zip(cases, t_start, pc.counted(cases)):
            if not on:
                continue
            d, (al,) = dc.described(c), pc.alignments([c], [s])
            pos = al[0]
            counts = ptb.pileup([al], max(pos - 3, 0), len(c.t) + 8)       # the region covers it
            dropped = [n for k, (n, op) in enumerate(c.cigar) if op == "I" and pos == 0 and not any(o != "I" for _, o in c.cigar[:k])]
            seen_dropped += len(dropped)
            assert sum(sum(counts[k]) for k in range(5)) == d.n_match + d.n_mismatch
            assert sum(counts[ptb.DEL]) == d.n_del
            assert sum(counts[ptb.INS]) == d.n_ins_runs - len(dropped) and sum(counts[ptb.INS_BASES]) == d.n_ins - sum(dropped)
    assert seen_dropped >= 1


def _core(rec, cigar):
    """the read without its soft clips, and the CIGAR without them"""
    lead = sum(n for n, op in cigar[:1] if op == "S")
    core = [(n, "M" if op in "M=X" else op) for n, op in cigar if op not in "SH"]
    return rec.seq[lead:lead + sum(n for n, op in core if op in "MI")], core


def test_the_bam_fixtures_nm_tags_add_up():
    _, _, records = formats.read_bam(BAM)
    als, refs, nm, used = [], {}, 0, 0
    for rec in records:
        if rec.flag & 4:
            continue
        rebuilt = formats.reference_under_read(rec)
        if rebuilt is None:
            continue
        try:  # only the records whose own CIGAR rebuilt the reference: their NM tag is that alignment's
            formats._rebuild(rec)
        except (AssertionError, IndexError):
            continue
        if any(op not in "MIDS" for _, op in rec.cigar) or rec.tags.get("NM") is None:
            continue
        query, core = _core(rec, rec.cigar)
        als.append((rec.pos, query, core))
        for k, b in enumerate(rebuilt[0]):   # the reference under the reads, position by position
            assert refs.setdefault(rec.pos + k, b) == b
        nm += rec.tags["NM"]
        used += 1
    assert used >= 1648
    beg, end = min(refs), max(refs) + 1
    counts = ptb.pileup(als, beg, end - beg)
    got = sum(counts[ptb.DEL]) + sum(counts[ptb.INS_BASES])
    for pos, b in refs.items():
        r = ptb.channel(b)
        got += sum(counts[c][pos - beg] for c in range(5) if c != r)
    assert got == nm and nm > 0, (got, nm)


def test_hand_cases():
    # ACGT at position 10 against A-GTT with an insertion: 1M 1D 2M 1I ... the I stands behind position 13
    counts = ptb.pileup([(10, b"AGTT", [(1, "M"), (1, "D"), (2, "M"), (1, "I")])], 8, 8)
    col = lambda i: [counts[p][i - 8] for p in range(8)]  # noqa: E731
    assert col(10) == [1, 0, 0, 0, 0, 0, 0, 0] and col(11) == [0, 0, 0, 0, 0, 1, 0, 0] and col(12) == [0, 0, 1, 0, 0, 0, 0, 0]
    assert col(13) == [0, 0, 0, 1, 0, 0, 1, 1] and col(9) == [0] * 8 and col(14) == [0] * 8
    # a leading I: at position 9, in front of the alignment; at position 0 it is dropped; two I elements count twice
    assert ptb.pileup([(10, b"TTA", [(2, "I"), (1, "M")])], 9, 1) == [[0]] * 6 + [[1], [2]]
    assert ptb.pileup([(0, b"TTA", [(2, "I"), (1, "M")])], 0, 1) == [[1]] + [[0]] * 7
    assert ptb.pileup([(5, b"TTA", [(2, "I"), (1, "I")])], 4, 1) == [[0]] * 6 + [[2], [3]]
    # the counts wrap
    assert ptb.pileup([(0, b"n", [(1, "M")])], 0, 1, [[0], [0], [0], [0], [ptb.MASK], [0], [0], [0]])[4] == [0]
    # sites: depth 10 over a reference C: 6 C, 3 T, 1 deleted; an insertion in 4 of them
    table = [[0], [6], [0], [3], [0], [1], [4], [9]]
    call, flags, out = ptb.sites(table, b"xxC", 2, 4, 2, 64)
    assert (call, flags) == (b"C", [1 | 2 | 8]) and out == [ptb.Site(0, 11, 10, 1, 1, 6, 3, 3)]
    assert ptb.sites(table, b"C", 0, 11, 2, 64) == (b"N", [0], [])                       # not covered
    assert ptb.sites(table, b"C", 0, 4, 4, 64)[1] == [1 | 8] and ptb.sites(table, b"C", 0, 4, 2, 76)[1] == [1 | 2 | 8]
    assert ptb.sites(table, b"C", 0, 4, 2, 77)[1] == [1 | 8]                             # 3 * 256 = 768 < 77 * 10
    assert ptb.sites(table, b"T", 0, 4, 2, 64)[2][0][3:] == (3, 1, 6, 1, 6)              # the reference's own base is no alt
    assert ptb.sites([[2], [2], [0], [0], [0], [2], [0], [0]], b"G", 0, 1, 1, 1)[2][0][4:] == (0, 2, 0, 2)  # ties go to the lowest channel


def test_the_constructed_tables_hold_what_they_are_for():
    counts, ref = pc.tie_tables()
    _, flags, out = ptb.sites([list(map(int, r)) for r in counts], ref, 0, 1, 1, 1)
    assert {s.call for s in out} == set(range(5)) and {s.alt for s in out} == set(range(5)) and {s.ref for s in out} == set(range(5))
    counts, ref, params = pc.threshold_tables()
    _, flags, out = ptb.sites([list(map(int, r)) for r in counts], ref, 0, *params)
    for k, bit in enumerate((2, 4, 8)):
        assert [f & bit for f in flags[6 * k:6 * k + 6]] == [0, 0, 0, bit, bit, 0], (k, flags[6 * k:6 * k + 6])
        assert [f & 1 for f in flags[6 * k:6 * k + 6]] == [0, 0, 1, 1, 1, 1]
    assert max(s.depth for s in out) == ptb.CLIP == max(s.call_count for s in out) == max(s.alt_count for s in out)
