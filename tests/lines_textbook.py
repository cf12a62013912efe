"""The functions of mgl_sw_expand_chains_batch_device and mgl_sw_classify_alignments_batch_device (include/mgl_sw.h, DESIGN.md section
9n), stated once in plain Python on top of rank_textbook.py: every ranked chain of a read becomes one alignment job, and the jobs'
alignments become the lines of the read -- primary, supplementary, secondary -- with a mapping quality that uses the alignment scores.
Integers only.

expand_chains.  Read p has q_start[p], q_len[p], the rank stage's status, n_chains[p], its records (rank_textbook.Ranked) and its ranked
anchors: ranked_start[p] .. ranked_start[p + 1] of the rank stage's ranked_t / _q / _len, the chains one behind the other in rank order,
n_anchors each.  Statuses per read (mgl_sw_status), the first that applies: the rank stage's own where that is not 0 (nothing else of
the read is looked at); 1 (BAD_ARG) for q_len < 1, a read that leaves [0, query_bytes), n_chains outside 0 .. max_chains, a record with
strand outside 0 / 1 or n_anchors < 1, a ranked_start range that descends, leaves [0, total_anchors] or is not the sum of the read's
n_anchors; 3 (NOMEM) by the capacity rule.  A read with a status has no jobs.  Otherwise every ranked chain c gives one job, in rank
order; with keep_secondary = 0 only the chains with parent == c do.
The capacity rule is per read and greedy: reads are visited in index order with S the jobs kept so far; a read with J jobs is kept iff
S + J <= job_capacity, and a read that is not kept is NOMEM and leaves S as it was, so a later, smaller read still fits.  (The seed
stage cuts EVERY pair from the first that does not fit; that would refuse reads that fit, so it is not taken over.)  The jobs' anchor
arrays have total_anchors entries, which the jobs of reads whose ranges are disjoint cannot exceed; ranges that overlap can, so the
rule holds for the anchors too: with A the anchors kept so far and a those of the read's jobs, the read is kept iff also
A + a <= total_anchors.
Jobs are numbered densely over the batch in read order: job_start[p] .. job_start[p + 1], n_jobs = job_start[n].  A job record is eight
int32: read, rank, strand, n_anchors, chain_score, chain_parent, q_len, 0.  job_q_len[j] = q_len[read], job_q_start[j] = q_start[read]
+ strand * query_bytes: an offset into the oriented buffer of 2 * query_bytes.
The jobs' anchors: job_anchor_start (job_capacity + 1 entries) is the prefix sum of the jobs' n_anchors, and job_anchor_t / _q / _len
hold the jobs' anchors one behind the other, COPIED from the ranked arrays.  (A CSR start array has no gaps: job j's anchors end where
job j + 1's begin.  The ranked arrays do have gaps between jobs -- the anchors of a chain that keep_secondary = 0 skips, those of a read
that is refused or cut -- so the ranked arrays cannot serve the jobs as they are; with every chain kept the copy is the identity.)
Jobs at or beyond n_jobs and below job_capacity are EMPTY: read -1, the other fields 0, q_start 0, q_len 0, no anchors
(job_anchor_start = its last value).  locate_window (ql < 1) and align_chain (a length below 1) refuse such a job with BAD_ARG.

oriented.  The first half of the buffer holds Q_p at q_start[p] for every read with a strand-0 job, the second half rc(Q_p) at
query_bytes + q_start[p] for every read with a strand-1 job; A <-> T and C <-> G, every other byte as it is (select_strand's rule).  No
other byte is written.

classify_alignments.  Per job: its record, the alignment's (score, q_beg, q_end) and its status; job_start [n + 1]; match, min_score,
mask_level.  Statuses per read: 1 (BAD_ARG) for a job_start range that descends, leaves [0, job_capacity] or is longer than 16, and for
a job in it whose `read` is not p; such a read has n_lines 0, primary_job -1 and no line record written.
A job is LIVE iff its status is 0, q_end > q_beg and score >= 1; nothing of the alignment record of a job with a non-zero status is
looked at.  A read's live jobs in the order (alignment score descending, rank ascending, job index ascending) are its LINES.  A line's
interval on the forward read is [q_beg, q_end) on strand 0 and [ql - q_end, ql - q_beg) on strand 1, ql the job's q_len.  Parents:
rank_textbook's rule on these intervals in line order -- line c looks at the earlier lines o that are their own parent, in order; with
ov = max(0, min(ends) - max(begins)), if ov * 256 >= mask_level * min(len_c, len_o) then parent(c) = o, n_sub(o) += 1, and where
score(c) > subsc(o): subsc(o) = score(c) and csub(o) = chain_score(c) (the first secondary of a line is its best aligned: the lines
descend).  Flags: 0x10 on strand 1; the first line is the primary and gets nothing more; another own-parent line gets 0x800
(supplementary); a line with a parent gets 0x100 (secondary).
Mapping quality of an own-parent line with alignment score s, chain score c (taken as at least 1) and K anchors -- minimap2's DP branch
in integers, no parity claimed:
    r_chain = (min(c, max(csub, min_score)) << 16) // c
    r_aln   = (subsc << 16) // s if n_sub > 0 else 65536
    x       = (r_chain * r_aln) >> 16
    raw     = (40 * min(K, 10) * (65536 - x) * lg8(max(1, s // match)) * 177) // (10 * 65536 * 65536)
    mapq    = clamp(raw - ((3 * lg8(n_sub + 1) + 128) >> 8), 0, 60)
Below 2^63: min(c, .) <= c < 2^31, so r_chain <= 65536 and its numerator is below 2^47; subsc <= s (a secondary stands behind its
parent), so r_aln <= 65536 with a numerator below 2^47; r_chain * r_aln <= 2^32 and 0 <= x <= 65536; lg8 of a value below 2^31 is below
31 * 256 + 256 = 2^13, so raw's numerator is at most 400 * 2^16 * 2^13 * 177 < 2^46.  A secondary line has mapq, n_sub and subsc 0.
Output per JOB index, eight int32: order (the line's place among the read's lines; -1 for a job that is not live), flag, mapq, parent
(a JOB index: the line's own where it is its own parent; -1 for a job that is not live), n_sub, subsc, fwd_q_beg, fwd_q_end; a job
that is not live has (-1, 0, 0, -1, 0, 0, 0, 0).  The lines of the jobs of every accepted read are written and no others: a job
that no read's range holds (the empty tail) has no line.  Per read: n_lines[p] and primary_job[p] (-1: unmapped).
"""
from collections import namedtuple

from rank_textbook import lg8

BAD_ARG, NOMEM = 1, 3
MAX_JOBS = 16  # per read

Job = namedtuple("Job", "read rank strand n_anchors chain_score chain_parent q_len reserved")
Line = namedtuple("Line", "order flag mapq parent n_sub subsc fwd_q_beg fwd_q_end")
EMPTY_JOB = Job(-1, 0, 0, 0, 0, 0, 0, 0)
DEAD_LINE = Line(-1, 0, 0, -1, 0, 0, 0, 0)

Expanded = namedtuple("Expanded", "n_jobs job_start jobs job_q_start job_q_len job_anchor_start job_anchor_t job_anchor_q job_anchor_len status")
Classified = namedtuple("Classified", "lines n_lines primary_job status")

_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(q):
    return bytes(q).translate(_COMP)[::-1]


def read_jobs(p, q_start, q_len, query_bytes, rank_status, n_chains, records, a, b, total_anchors, max_chains, keep_secondary):
    """one read, before the capacity rule -> (status, [(Job, its anchors' offset from the read's first, relative)])"""
    if rank_status:
        return rank_status, []
    if q_len < 1 or q_start < 0 or q_start + q_len > query_bytes or not 0 <= n_chains <= max_chains:
        return BAD_ARG, []
    if a < 0 or b < a or b > total_anchors:
        return BAD_ARG, []
    recs = records[:n_chains]
    if any(r.strand not in (0, 1) or r.n_anchors < 1 for r in recs) or sum(r.n_anchors for r in recs) != b - a:
        return BAD_ARG, []
    out, off = [], 0
    for c, r in enumerate(recs):
        if keep_secondary or r.parent == c:
            out.append((Job(p, c, r.strand, r.n_anchors, r.score, r.parent, q_len, 0), a + off))
        off += r.n_anchors
    return 0, out


def expand_chains(q_start, q_len, query_bytes, rank_status, n_chains, records, max_chains, ranked_start, ranked_t, ranked_q, ranked_len,
                  total_anchors, keep_secondary, job_capacity):
    """The batch as the entry sees it -> Expanded; ``records[p]``: the read's [Ranked]; ``rank_status``: None for all 0."""
    assert 1 <= max_chains <= MAX_JOBS and keep_secondary in (0, 1) and 0 <= job_capacity <= 1 << 30
    n = len(q_len)
    job_start, jobs, at, aq, al, astart, status = [0], [], [], [], [], [0], []
    for p in range(n):
        st, mine = read_jobs(p, int(q_start[p]), int(q_len[p]), query_bytes, 0 if rank_status is None else int(rank_status[p]), int(n_chains[p]),
                             records[p], int(ranked_start[p]), int(ranked_start[p + 1]), total_anchors, max_chains, keep_secondary)
        if st == 0 and (len(jobs) + len(mine) > job_capacity or len(at) + sum(j.n_anchors for j, _ in mine) > total_anchors):
            st, mine = NOMEM, []
        for job, src in mine:
            jobs.append(job)
            for i in range(src, src + job.n_anchors):
                at.append(int(ranked_t[i])), aq.append(int(ranked_q[i])), al.append(int(ranked_len[i]))
            astart.append(len(at))
        job_start.append(len(jobs))
        status.append(st)
    n_jobs = len(jobs)
    jq_start = [int(q_start[j.read]) + j.strand * query_bytes for j in jobs] + [0] * (job_capacity - n_jobs)
    jq_len = [j.q_len for j in jobs] + [0] * (job_capacity - n_jobs)
    jobs = jobs + [EMPTY_JOB] * (job_capacity - n_jobs)
    astart = astart + [astart[-1]] * (job_capacity - n_jobs)
    return Expanded(n_jobs, job_start, jobs, jq_start, jq_len, astart, at, aq, al, status)


def oriented(queries, q_start, q_len, query_bytes, exp, before=None):
    """The oriented buffer behind expand_chains: ``before`` (2 * query_bytes, zeros by default) with the bytes the stage writes."""
    buf = bytearray(before if before is not None else bytes(2 * query_bytes))
    assert len(buf) == 2 * query_bytes
    for j in exp.jobs[:exp.n_jobs]:
        a, l = int(q_start[j.read]), int(q_len[j.read])
        q = bytes(queries[a:a + l])
        buf[j.strand * query_bytes + a:j.strand * query_bytes + a + l] = revcomp(q) if j.strand else q
    return bytes(buf)


def line_mapq(s, c, k, n_sub, subsc, csub, match, min_score):
    c = max(c, 1)
    r_chain = (min(c, max(csub, min_score)) << 16) // c
    r_aln = (subsc << 16) // s if n_sub > 0 else 65536
    x = (r_chain * r_aln) >> 16
    num = 40 * min(k, 10) * (65536 - x) * lg8(max(1, s // match)) * 177
    assert 0 <= r_chain <= 65536 and 0 <= r_aln <= 65536 and 0 <= num < 1 << 63
    raw = num // (10 * 65536 * 65536)
    return max(0, min(60, raw - ((3 * lg8(n_sub + 1) + 128) >> 8)))


def classify_read(jobs, aln, aln_status, first, match, min_score, mask_level):
    """One accepted read: its jobs, their (score, q_beg, q_end) and statuses, the index of its first job -> ([Line] per job, n_lines,
    primary_job)"""
    m = len(jobs)
    live = [aln_status[j] == 0 and aln[j][2] > aln[j][1] and aln[j][0] >= 1 for j in range(m)]
    order = sorted((j for j in range(m) if live[j]), key=lambda j: (-aln[j][0], jobs[j].rank, j))
    L = len(order)
    span = []
    for j in order:
        ql, (_, qb, qe) = jobs[j].q_len, aln[j]
        span.append((ql - qe, ql - qb) if jobs[j].strand else (qb, qe))
    score = [aln[j][0] for j in order]
    parent, n_sub, subsc, csub = list(range(L)), [0] * L, [0] * L, [0] * L
    for c in range(L):
        for o in range(c):
            if parent[o] != o:
                continue
            ov = max(0, min(span[c][1], span[o][1]) - max(span[c][0], span[o][0]))
            if ov * 256 >= mask_level * min(span[c][1] - span[c][0], span[o][1] - span[o][0]):
                parent[c] = o
                n_sub[o] += 1
                if score[c] > subsc[o]:
                    subsc[o], csub[o] = score[c], jobs[order[c]].chain_score
                break
    lines = [DEAD_LINE] * m
    for c, j in enumerate(order):
        own = parent[c] == c
        flag = (0x10 if jobs[j].strand else 0) | (0x100 if not own else 0x800 if c > 0 else 0)
        q = line_mapq(score[c], jobs[j].chain_score, jobs[j].n_anchors, n_sub[c], subsc[c], csub[c], match, min_score) if own else 0
        lines[j] = Line(c, flag, q, first + order[parent[c]], n_sub[c] if own else 0, subsc[c] if own else 0, span[c][0], span[c][1])
    return lines, L, first + order[0] if L else -1


def classify_alignments(job_start, jobs, job_capacity, aln, aln_status, match, min_score, mask_level):
    """The batch as the entry sees it: ``jobs`` [job_capacity] Job, ``aln`` [job_capacity] (score, q_beg, q_end), ``aln_status``
    [job_capacity] -> Classified; ``lines[j]`` is None where the entry writes nothing."""
    assert match >= 1 and min_score >= 1 and 1 <= mask_level <= 256
    n = len(job_start) - 1
    lines, n_lines, primary, status = [None] * job_capacity, [], [], []
    for p in range(n):
        a, b = int(job_start[p]), int(job_start[p + 1])
        if a < 0 or b < a or b > job_capacity or b - a > MAX_JOBS or any(jobs[j].read != p for j in range(a, b)):
            n_lines.append(0), primary.append(-1), status.append(BAD_ARG)
            continue
        mine, L, prim = classify_read(jobs[a:b], aln[a:b], aln_status[a:b], a, match, min_score, mask_level)
        lines[a:b] = mine
        n_lines.append(L), primary.append(prim), status.append(0)
    return Classified(lines, n_lines, primary, status)
