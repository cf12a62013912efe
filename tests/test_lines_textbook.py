"""tests/lines_textbook.py against independent restatements of its two functions on random reads, and against cases worked out by hand:
the mask's edge, the strand-1 flip, re-ranking, ties, dead jobs, a parent that is not line 0, the MAPQ table and its 2^63 bound, the
capacity rule at its edges, and the empty tail."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lines_cases as lc  # noqa: E402
import lines_textbook as ltb  # noqa: E402
from rank_textbook import lg8  # noqa: E402


# ---------------------------------------------------------------------------------------------------------------- restatements

def restated_expand(b, keep_secondary, job_capacity):
    """expand_chains once more, array-wise: which chains give jobs first, then the greedy cut as a running sum, then everything by
    index arithmetic on the kept chains"""
    n = len(b["q_len"])
    status, cand = [], []
    for p in range(n):
        recs = b["records"][p][:max(b["n_chains"][p], 0)]
        a, e = b["ranked_start"][p], b["ranked_start"][p + 1]
        if b["rank_status"][p]:
            status.append(b["rank_status"][p])
        elif (b["q_len"][p] <= 0 or b["q_start"][p] < 0 or b["q_start"][p] + b["q_len"][p] > b["query_bytes"] or b["n_chains"][p] < 0 or
              b["n_chains"][p] > b["max_chains"] or a < 0 or e < a or e > b["total_anchors"] or any(r.strand not in (0, 1) for r in recs) or
              any(r.n_anchors <= 0 for r in recs) or e - a != sum(r.n_anchors for r in recs)):
            status.append(1)
        else:
            status.append(0)
        offs = np.concatenate([[0], np.cumsum([r.n_anchors for r in recs])]).astype(int) if status[-1] == 0 else []
        cand.append([(c, a + int(offs[c])) for c, r in enumerate(recs) if keep_secondary or r.parent == c] if status[-1] == 0 else [])
    used_j = used_a = 0
    job_start, rows, src = [0], [], []
    for p in range(n):
        k = sum(b["records"][p][c].n_anchors for c, _ in cand[p])
        if status[p] == 0 and (used_j + len(cand[p]) > job_capacity or used_a + k > b["total_anchors"]):
            status[p], cand[p] = 3, []
        used_j, used_a = used_j + len(cand[p]), used_a + (k if cand[p] else 0)
        for c, at in cand[p]:
            r = b["records"][p][c]
            rows.append((p, c, r.strand, r.n_anchors, r.score, r.parent, b["q_len"][p], 0))
            src.append(at)
        job_start.append(len(rows))
    idx = [i for (row, at) in zip(rows, src) for i in range(at, at + row[3])]
    astart = list(np.concatenate([[0], np.cumsum([row[3] for row in rows])]).astype(int)) + [sum(row[3] for row in rows)] * (job_capacity - len(rows))
    empty = job_capacity - len(rows)
    return (len(rows), job_start, rows + [(-1, 0, 0, 0, 0, 0, 0, 0)] * empty, [b["q_start"][r[0]] + r[2] * b["query_bytes"] for r in rows] + [0] * empty,
            [r[6] for r in rows] + [0] * empty, astart, [b["ranked_t"][i] for i in idx], [b["ranked_q"][i] for i in idx], [b["ranked_len"][i] for i in idx],
            status)


def restated_classify(job_start, jobs, cap, aln, st, match, min_score, mask_level):
    """classify_alignments once more: lines as sorted tuples, parents through a dict of the own-parent lines met so far"""
    lines, n_lines, primary, status = [None] * cap, [], [], []
    for p in range(len(job_start) - 1):
        a, b = job_start[p], job_start[p + 1]
        if not (0 <= a <= b <= cap and b - a <= 16 and all(jobs[j].read == p for j in range(a, b))):
            n_lines.append(0), primary.append(-1), status.append(1)
            continue
        rows = []
        for j in range(a, b):
            lines[j] = (-1, 0, 0, -1, 0, 0, 0, 0)
            if st[j] != 0 or aln[j][2] <= aln[j][1] or aln[j][0] < 1:
                continue
            s, qb, qe = aln[j]
            lo, hi = (jobs[j].q_len - qe, jobs[j].q_len - qb) if jobs[j].strand == 1 else (qb, qe)
            rows.append((-s, jobs[j].rank, j, lo, hi))
        rows.sort()
        heads = {}  # line -> [n_sub, subsc, csub]
        parent = {}
        for c, (ns, _, j, lo, hi) in enumerate(rows):
            for o in sorted(heads):
                _, _, _, olo, ohi = rows[o]
                if max(0, min(hi, ohi) - max(lo, olo)) * 256 >= mask_level * min(hi - lo, ohi - olo):
                    parent[c] = o
                    heads[o][0] += 1
                    if -ns > heads[o][1]:
                        heads[o][1:] = [-ns, jobs[j].chain_score]
                    break
            else:
                parent[c] = c
                heads[c] = [0, 0, 0]
        for c, (ns, _, j, lo, hi) in enumerate(rows):
            flag = 0x10 * jobs[j].strand
            if parent[c] != c:
                lines[j] = (c, flag | 0x100, 0, rows[parent[c]][2], 0, 0, lo, hi)
                continue
            n_sub, subsc, csub = heads[c]
            s, ch = -ns, max(1, jobs[j].chain_score)
            x = (((min(ch, max(csub, min_score)) * 65536) // ch) * (((subsc * 65536) // s) if n_sub else 65536)) // 65536
            raw = (40 * min(jobs[j].n_anchors, 10) * (65536 - x) * lg8(max(1, s // match)) * 177) // (10 * 65536 ** 2)
            lines[j] = (c, flag | (0x800 if c else 0), min(60, max(0, raw - (3 * lg8(n_sub + 1) + 128) // 256)), j, n_sub, subsc, lo, hi)
        n_lines.append(len(rows)), primary.append(rows[0][2] if rows else -1), status.append(0)
    return lines, n_lines, primary, status


# ---------------------------------------------------------------------------------------------------------------- random reads

@pytest.mark.parametrize("keep_secondary", [0, 1])
def test_expand_chains_against_its_restatement(keep_secondary):
    rng = np.random.default_rng(keep_secondary)
    reads = []
    for p in range(60):
        status = int(rng.choice([0, 0, 0, 0, 0, 1, 5]))
        reads.append((lc.random_read(rng, int(rng.integers(1, 80))), status, lc.random_records(rng, int(rng.integers(0, 17)))))
    b = lc.expand_batch(reads, 16, gap=1)
    for p in (7, 23):  # per-read refusals of several kinds among them
        b["q_len"][p] = 0
    b["n_chains"][31] = 17
    b["records"][40] = [b["records"][40][0]._replace(strand=3)] + b["records"][40][1:] if b["records"][40] else b["records"][40]
    total_jobs = ltb.expand_chains(b["q_start"], b["q_len"], b["query_bytes"], b["rank_status"], b["n_chains"], b["records"], 16, b["ranked_start"],
                                   b["ranked_t"], b["ranked_q"], b["ranked_len"], b["total_anchors"], keep_secondary, 60 * 16).n_jobs
    assert total_jobs > 100
    for cap in (60 * 16, total_jobs, total_jobs - 1, total_jobs // 2, 5, 0):
        e = lc.expand_textbook(b, keep_secondary, cap)
        assert tuple(e) == tuple(restated_expand(b, keep_secondary, cap))[:10] and list(map(tuple, e.jobs)) == restated_expand(b, keep_secondary, cap)[2]
        assert 3 in e.status or cap >= total_jobs


def test_classify_alignments_against_its_restatement():
    rng = np.random.default_rng(4)
    reads = lc.random_classify_reads(rng, [int(rng.integers(0, 17)) for _ in range(60)])
    for mask_level in (1, 64, 128, 256):
        for match in (1, 200):
            job_start, jobs, aln, st, cap = lc.classify_batch(reads)
            c = ltb.classify_alignments(job_start, jobs, cap, aln, st, match, 40, mask_level)
            lines, n_lines, primary, status = restated_classify(job_start, jobs, cap, aln, st, match, 40, mask_level)
            assert [None if l is None else tuple(l) for l in c.lines] == lines and c.n_lines == n_lines and c.primary_job == primary and c.status == status
    flags = {l.flag for l in c.lines if l is not None and l.order >= 0}
    assert flags >= {0, 0x10, 0x100, 0x110} and any(l.mapq > 0 for l in c.lines if l is not None)
    # per-read refusals
    job_start, jobs, aln, st, cap = lc.classify_batch(reads, tail=20)
    for edit in (lambda s, j: s.__setitem__(5, s[4] - 1), lambda s, j: s.__setitem__(60, cap + 1), lambda s, j: s.__setitem__(60, s[59] + 17),
                 lambda s, j: j.__setitem__(s[10], j[s[10]]._replace(read=99))):
        s2, j2 = list(job_start), list(jobs)
        edit(s2, j2)
        c = ltb.classify_alignments(s2, j2, cap, aln, st, 1, 40, 128)
        assert ([None if l is None else tuple(l) for l in c.lines], c.n_lines, c.primary_job, c.status) == restated_classify(s2, j2, cap, aln, st, 1, 40, 128)
        assert 1 in c.status


# ---------------------------------------------------------------------------------------------------------------- by hand

@pytest.mark.parametrize("case", lc.HAND, ids=[c[0] for c in lc.HAND])
def test_hand_cases(case):
    name, mine, params, want, n_lines, primary = case
    job_start, jobs, aln, st, cap = lc.hand_batch(case)
    c = ltb.classify_alignments(job_start, jobs, cap, aln, st, *params)
    assert [(l.order, l.flag, l.parent) for l in c.lines[:len(mine)]] == want and c.n_lines == [n_lines] and c.primary_job == [primary]
    assert c.lines[len(mine):] == [None] * 3 and c.status == [0]


def test_the_strand_flip_changes_the_interval():
    job_start, jobs, aln, st, cap = lc.hand_batch(lc.HAND[2])
    c = ltb.classify_alignments(job_start, jobs, cap, aln, st, 1, 40, 128)
    assert (c.lines[1].fwd_q_beg, c.lines[1].fwd_q_end) == (0, 100) and (c.lines[0].fwd_q_beg, c.lines[0].fwd_q_end) == (0, 100)


@pytest.mark.parametrize("args,want", lc.MAPQ)
def test_the_mapq_table(args, want):
    assert ltb.line_mapq(*args) == want  # (line_mapq asserts every intermediate below 2^63)


def test_mapq_through_classify_with_n_sub_0_1_3():
    got = []
    for n_sub in (0, 1, 3):
        mine = [(lc.J(0, chain_score=1000), (1000, 0, 100), 0)] + [(lc.J(1 + x, chain_score=900 - x), (950 - x, 10, 60), 0) for x in range(n_sub)]
        job_start, jobs, aln, st, cap = lc.classify_batch([mine])
        c = ltb.classify_alignments(job_start, jobs, cap, aln, st, 1, 40, 128)
        assert (c.lines[0].n_sub, c.lines[0].subsc) == (n_sub, 950 if n_sub else 0) and all(l.mapq == 0 and l.n_sub == 0 and l.subsc == 0 for l in c.lines[1:1 + n_sub])
        got.append(c.lines[0].mapq)
    # n_sub = 1: x = 56032 as in the table, raw = 39, minus (3 * 256 + 128) >> 8 = 3
    assert got == [60, 36, 33]


def test_the_capacity_rule_and_the_empty_tail():
    rng = np.random.default_rng(6)
    reads = [(lc.random_read(rng, 20), 0, lc.random_records(rng, m)) for m in (3, 4, 2, 1, 4, 1)]
    b = lc.expand_batch(reads, 4)
    assert lc.expand_textbook(b, 1, 15).status == [0] * 6  # exactly fitting
    assert lc.expand_textbook(b, 1, 14).status == [0] * 5 + [3]  # one short
    e = lc.expand_textbook(b, 1, 8)  # the read of 2 does not fit behind 3 + 4; the later, smaller read of 1 still does
    assert e.status == [0, 0, 3, 0, 3, 3] and e.job_start == [0, 3, 7, 7, 8, 8, 8] and e.n_jobs == 8
    assert [j.read for j in e.jobs] == [0, 0, 0, 1, 1, 1, 1, 3]
    e = lc.expand_textbook(b, 1, 13)  # 3 + 4 + 2 + 1, not 4, then 1: eleven jobs and a tail of two empty ones without anchors
    assert e.n_jobs == 11 and e.jobs[11:] == [ltb.EMPTY_JOB] * 2 and e.job_q_len[11:] == [0, 0] and e.job_q_start[11:] == [0, 0]
    assert e.job_anchor_start[11:] == [len(e.job_anchor_t)] * 3 and len(e.job_anchor_start) == 14 and e.status == [0, 0, 0, 0, 3, 0]
    assert lc.expand_textbook(b, 1, 0).status == [3] * 6


def test_the_oriented_buffer():
    reads = [(b"ACGTNNAC", 0, [lc.ranked(50, 0, 1, 0)]), (b"AACCGGTTNx", 0, [lc.ranked(50, 1, 1, 0)]), (b"ACG", 0, [lc.ranked(9, 0, 1, 0), lc.ranked(8, 1, 2, 1)]),
             (b"TTTT", 0, [])]
    b = lc.expand_batch(reads, 2, gap=1, first=2)
    e = lc.expand_textbook(b, 1, 8)
    got = ltb.oriented(b["queries"], b["q_start"], b["q_len"], b["query_bytes"], e, before=b"." * (2 * b["query_bytes"]))
    n = b["query_bytes"]
    assert got[:n] == b"..ACGTNNAC............ACG......" and got[n:] == b"...........xNAACCGGTT.CGT......"
    assert e.job_q_start == [2, n + 11, 22, n + 22] + [0] * 4
