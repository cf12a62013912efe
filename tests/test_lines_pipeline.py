"""Proof, without a GPU, that the inputs of the map_reads_all pipeline tests are adversarial: the existing CPU textbooks composed
(tests/lines_cases.py: compose -- seeds, grouped chains, ranks, lines_textbook.expand_chains, the window per job, chain_textbook.
chain_align per job, lines_textbook.classify_alignments) give a supplementary line in another contig, a secondary of equal score with
mapq 0, secondaries of strictly lower score with 0 < mapq < 60, and one read with a line on each strand."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contig_cases as cc  # noqa: E402
import lines_cases as lc  # noqa: E402


def _lines(d, p):
    e, c = d["expanded"], d["classified"]
    jobs = [j for j in range(e.job_start[p], e.job_start[p + 1]) if c.lines[j].order >= 0]
    return sorted(jobs, key=lambda j: c.lines[j].order)


def test_the_chimera_gives_a_primary_and_a_supplementary_line_in_the_other_contig():
    _, _, _, _, _, _, d = lc.contig_composed(False)
    c, rid = d["classified"], d["located"][4]
    first, second = _lines(d, cc.CHIMERA)
    assert (c.lines[first].flag, c.lines[second].flag) == (0, 0x800) and {rid[first], rid[second]} == {0, 1}
    assert c.lines[second].parent == second and c.lines[first].n_sub == 0
    # their intervals on the forward read overlap below the mask: here not at all
    spans = sorted((c.lines[j].fwd_q_beg, c.lines[j].fwd_q_end) for j in (first, second))
    assert spans == [(0, 600), (600, 1200)]


def test_the_read_whose_window_two_contigs_hold_gives_a_secondary_of_equal_score_and_mapq_0():
    _, _, _, _, _, _, d = lc.contig_composed(False)
    c, rid = d["classified"], d["located"][4]
    first, second = _lines(d, 0)
    assert (c.lines[first].flag, c.lines[second].flag) == (0, 0x100) and c.lines[second].parent == first and (rid[first], rid[second]) == (0, 3)
    assert d["aln"][first][0] == d["aln"][second][0] == c.lines[first].subsc and c.lines[first].mapq == 0 and c.lines[first].n_sub == 1
    assert all(c.lines[_lines(d, p)[0]].mapq == 60 and len(_lines(d, p)) == 1 for p in range(1, 8)) and _lines(d, cc.UNRELATED_AT) == []


def test_a_split_read_with_an_inverted_part_gives_one_line_per_strand():
    _, _, _, _, reads, _, d = lc.contig_composed(False)
    _, truth = lc.contig_reads()
    c, e = d["classified"], d["expanded"]
    for k, parts in enumerate(truth):
        p = len(reads) - 2 + k
        lines = _lines(d, p)
        assert len(lines) == 2 and sorted(e.jobs[j].strand for j in lines) == sorted(part[2] for part in parts)
    assert [part[2] for part in truth[1]] == [0, 1]  # the inversion: ONE read, a job on each strand
    # (with GATK's gap extension of 11 and no Z-drop each part's job aligns on through the breakpoint, so the two lines cover the same
    # part of the read and the second is 0x100, not 0x800: DESIGN.md section 9n, Limits)
    assert [c.lines[j].flag & 0x10 for j in _lines(d, len(reads) - 1)] == [0, 0x10]


def test_repeat_copies_at_one_per_cent_give_lower_scores_and_a_mapq_between_0_and_60():
    _, _, _, d = lc.repeat_composed(0.01)
    e, c = d["expanded"], d["classified"]
    assert c.n_lines == [2] * 4 + [1] * 4
    for p in range(4):
        first, second = _lines(d, p)
        assert c.lines[second].flag & 0x100 and d["aln"][second][0] < d["aln"][first][0] and 0 < c.lines[first].mapq < 60
    # the values found (alignment scores of the read and its copy; the chain-level MAPQ of section 9k beside them is 19 .. 43)
    assert [c.lines[e.job_start[p]].mapq for p in range(8)] == [46, 25, 24, 52, 60, 60, 60, 60]
    assert [(d["aln"][e.job_start[p]][0], d["aln"][e.job_start[p] + 1][0]) for p in range(4)] == [(358858, 351037), (357599, 352706), (363401, 357801),
                                                                                                  (353582, 345142)]
    _, _, _, exact = lc.repeat_composed(0.0)
    assert [exact["classified"].lines[exact["expanded"].job_start[p]].mapq for p in range(8)] == [0] * 4 + [60] * 4
