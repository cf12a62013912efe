"""Inputs for the tests of the expand and classify stages (tests/lines_textbook.py is the definition): batches of reads with made-up
rank records for expand_chains, batches of jobs with made-up alignments for classify_alignments, the hand cases of the latter worked
out by hand, and the expected output arrays -- canaries where nothing is written -- as the GPU tests compare them."""
import numpy as np

import lines_textbook as ltb
from rank_textbook import Ranked

CANARY = -0x5A5A5A5B
CANARY_BYTE = 0xA5
PAD = 16


# ---------------------------------------------------------------------------------------------------------------- expand_chains

def ranked(score, strand, k, parent):
    """a rank record of which the expand stage reads score, strand, n_anchors and parent"""
    return Ranked(score, strand, k, 0, 0, 0, 0, parent, 0, 0, 0, 0)


def expand_batch(reads, max_chains, gap=0, first=0, residues=None):
    """``reads``: per read (the read's bytes, rank_status, [Ranked]) -> the stage's inputs as a dict.  The reads lie ``gap`` bytes apart
    from offset ``first`` on -- with ``residues`` read p begins at the first offset behind that which is residues[p] mod 16 --; the
    anchors are numbered so that every copy shows."""
    q_start, q_len, buf = [], [], bytearray(b"N" * first)
    start, t, q, l = [0], [], [], []
    for p, (seq, _, recs) in enumerate(reads):
        if residues is not None:
            buf += b"N" * ((residues[p] - len(buf)) % 16)
        q_start.append(len(buf)), q_len.append(len(seq))
        buf += bytes(seq) + b"N" * gap
        for c, r in enumerate(recs):
            for x in range(r.n_anchors):
                t.append(1000 * len(start) + 100 * c + x), q.append(7 * len(t)), l.append(1 + (len(t) % 5))
        start.append(len(t))
    return dict(queries=bytes(buf), q_start=q_start, q_len=q_len, query_bytes=len(buf), rank_status=[s for _, s, _ in reads],
                n_chains=[len(r) for _, _, r in reads], records=[r for _, _, r in reads], max_chains=max_chains, ranked_start=start, ranked_t=t,
                ranked_q=q, ranked_len=l, total_anchors=len(t))


def expand_textbook(b, keep_secondary, job_capacity, rank_status=True):
    return ltb.expand_chains(b["q_start"], b["q_len"], b["query_bytes"], b["rank_status"] if rank_status else None, b["n_chains"], b["records"],
                             b["max_chains"], b["ranked_start"], b["ranked_t"], b["ranked_q"], b["ranked_len"], b["total_anchors"], keep_secondary,
                             job_capacity)


EXPAND_NAMES = ("n_jobs", "job_start", "jobs", "job_q_start", "job_q_len", "job_anchor_start", "job_anchor_t", "job_anchor_q", "job_anchor_len",
                "oriented", "status")


def expand_sizes(b, job_capacity):
    n, total = len(b["q_len"]), b["total_anchors"]
    return (1, n + 1, 8 * job_capacity, job_capacity, job_capacity, job_capacity + 1, total, total, total, 2 * b["query_bytes"], n)


def expand_dtypes():
    return (np.int64, np.int64, np.int32, np.int64, np.int32, np.int64, np.int32, np.int32, np.int32, np.uint8, np.int32)


def expand_expected(b, keep_secondary, job_capacity, rank_status=True):
    """-> (Expanded, the eleven output arrays with PAD canaries behind each (8 * PAD behind the jobs); the oriented buffer starts as
    canary bytes, so every byte the stage must not write shows)"""
    e = expand_textbook(b, keep_secondary, job_capacity, rank_status)
    ori = ltb.oriented(b["queries"], b["q_start"], b["q_len"], b["query_bytes"], e, before=bytes([CANARY_BYTE]) * (2 * b["query_bytes"]))
    kept = len(e.job_anchor_t)
    tail = [CANARY] * (b["total_anchors"] - kept)
    vals = ([e.n_jobs], e.job_start, [v for j in e.jobs for v in j], e.job_q_start, e.job_q_len, e.job_anchor_start, e.job_anchor_t + tail,
            e.job_anchor_q + tail, e.job_anchor_len + tail, np.frombuffer(ori, np.uint8), e.status)
    out = []
    for k, (v, dt) in enumerate(zip(vals, expand_dtypes())):
        pad = PAD * 8 if k == 2 else PAD
        can = CANARY_BYTE if dt == np.uint8 else CANARY
        out.append(np.concatenate([np.asarray(v, dtype=dt).reshape(-1), np.full(pad, can, dtype=dt)]))
    return e, out


def random_read(rng, length):
    seq = np.frombuffer(b"ACGTNacgtRY", np.uint8)[rng.integers(0, 11 if rng.random() < 0.3 else 4, length)].tobytes()
    return seq


def random_records(rng, n_chains, sizes=(1, 2, 3, 5)):
    recs = []
    for c in range(n_chains):
        own = [o for o in range(c) if recs[o].parent == o]
        parent = int(rng.choice(own)) if own and rng.random() < 0.5 else c
        recs.append(ranked(int(rng.integers(40, 5000)), int(rng.integers(0, 2)), int(rng.choice(sizes)), parent))
    return recs


# ---------------------------------------------------------------------------------------------------------------- classify_alignments

def job(read, rank, strand=0, k=10, chain_score=100, q_len=1000, parent=None):
    return ltb.Job(read, rank, strand, k, chain_score, rank if parent is None else parent, q_len, 0)


def classify_batch(reads, job_capacity=None, tail=3):
    """``reads``: per read a list of (Job fields without `read` as a dict or Job, (score, q_beg, q_end), status) -> (job_start, jobs,
    aln, aln_status, job_capacity); ``tail`` empty jobs follow"""
    job_start, jobs, aln, st = [0], [], [], []
    for p, mine in enumerate(reads):
        for j, a, s in mine:
            jobs.append(j._replace(read=p) if j.read is None else j)
            aln.append(tuple(a)), st.append(s)
        job_start.append(len(jobs))
    cap = len(jobs) + tail if job_capacity is None else job_capacity
    jobs += [ltb.EMPTY_JOB] * (cap - len(jobs))
    aln += [(0, 0, 0)] * (cap - len(aln))
    st += [ltb.BAD_ARG] * (cap - len(st))
    return job_start, jobs, aln, st, cap


def J(rank, strand=0, k=10, chain_score=100, q_len=1000):
    return ltb.Job(None, rank, strand, k, chain_score, rank, q_len, 0)


# (name, the read's jobs, (match, min_score, mask_level), the expected (order, flag, parent) per job, n_lines, primary)
HAND = [
    # two lines of 100 bases that share 50: ov * 256 = 12800 = 128 * 100 -> secondary
    ("overlap exactly at the mask", [(J(0), (500, 0, 100), 0), (J(1), (400, 50, 150), 0)], (1, 40, 128), [(0, 0, 0), (1, 0x100, 0)], 2, 0),
    # one base less: 49 * 256 = 12544 < 12800 -> supplementary
    ("overlap one below the mask", [(J(0), (500, 0, 100), 0), (J(1), (400, 51, 151), 0)], (1, 40, 128), [(0, 0, 0), (1, 0x800, 1)], 2, 0),
    # [0, 100) on strand 0 and [900, 1000) on strand 1 of a read of 1000: the latter is [0, 100) of the forward read
    ("overlap only after the strand-1 flip", [(J(0), (500, 0, 100), 0), (J(1, strand=1), (400, 900, 1000), 0)], (1, 40, 128),
     [(0, 0, 0), (1, 0x110, 0)], 2, 0),
    ("no overlap without the flip", [(J(0), (500, 0, 100), 0), (J(1), (400, 900, 1000), 0)], (1, 40, 128), [(0, 0, 0), (1, 0x800, 1)], 2, 0),
    # rank 1 aligns better than rank 0 and becomes the primary line
    ("re-ranking", [(J(0), (300, 0, 100), 0), (J(1), (700, 200, 300), 0)], (1, 40, 128), [(1, 0x800, 0), (0, 0, 1)], 2, 1),
    ("equal scores go to the lower rank", [(J(0), (500, 0, 100), 0), (J(1), (500, 0, 100), 0)], (1, 40, 128), [(0, 0, 0), (1, 0x100, 0)], 2, 0),
    ("all jobs dead", [(J(0), (500, 0, 100), 1), (J(1), (0, 0, 100), 0), (J(2), (50, 10, 10), 0)], (1, 40, 128),
     [(-1, 0, -1), (-1, 0, -1), (-1, 0, -1)], 0, -1),
    # line 2 does not overlap line 0, does overlap line 1, which is its own parent: its parent is line 1, not line 0
    ("first fitting parent is not line 0", [(J(0), (900, 0, 100), 0), (J(1), (800, 500, 600), 0), (J(2), (700, 520, 600), 0)], (1, 40, 128),
     [(0, 0, 0), (1, 0x800, 1), (2, 0x100, 1)], 3, 0),
    # a secondary is no parent: line 2 lies inside line 1, which is line 0's secondary, and outside line 0's first half
    ("a secondary is nobody's parent", [(J(0), (900, 0, 200), 0), (J(1), (800, 100, 300), 0), (J(2), (700, 250, 300), 0)], (1, 40, 128),
     [(0, 0, 0), (1, 0x100, 0), (2, 0x800, 2)], 3, 0),
    ("no jobs", [], (1, 40, 128), [], 0, -1),
]


def hand_batch(case):
    name, mine, params, want, n_lines, primary = case
    return classify_batch([mine])


# (s, c, K, n_sub, subsc, csub, match, min_score) -> mapq, each worked out by hand from the formula in lines_textbook's docstring
MAPQ = [
    # no secondary: r_chain = (40 << 16) // 1000 = 2621, r_aln = 65536, x = 2621; lg8(1000 // 1) = (9 << 8) + ((1000 << 8 >> 9) - 256) =
    # 2304 + 244 = 2548; raw = 400 * 62915 * 2548 * 177 // 42949672960 = 264; the clamp to 60
    ((1000, 1000, 10, 0, 0, 0, 1, 40), 60),
    # s < match: lg8(max(1, 0)) = 0 -> raw 0 -> 0
    ((150, 1000, 10, 0, 0, 0, 200, 40), 0),
    # subsc == s: r_aln = 65536; csub == c: r_chain = 65536; x = 65536 -> raw 0; minus (3 * lg8(2) + 128) >> 8 = (768 + 128) >> 8 = 3 -> 0
    ((1000, 1000, 10, 1, 1000, 1000, 1, 40), 0),
    # three secondaries, a near one: r_chain = (900 << 16) // 1000 = 58982, r_aln = (950 << 16) // 1000 = 62259, x = (58982 * 62259) >> 16
    # = 56032; raw = 400 * 9504 * 2548 * 177 // 42949672960 = 39; minus (3 * lg8(4) + 128) >> 8 = (1536 + 128) >> 8 = 6 -> 33
    ((1000, 1000, 10, 3, 950, 900, 1, 40), 33),
    # few anchors scale it down: K = 3: raw = 120 * 9504 * 2548 * 177 // 42949672960 = 11; minus 6 -> 5
    ((1000, 1000, 3, 3, 950, 900, 1, 40), 5),
    # the clamp at 0: K = 1: raw = 40 * 9504 * 2548 * 177 // 42949672960 = 3; minus 6 -> -3 -> 0
    ((1000, 1000, 1, 3, 950, 900, 1, 40), 0),
    # the largest values: every intermediate asserted below 2^63 inside line_mapq
    ((2**31 - 1, 2**31 - 1, 10, 0, 0, 0, 1, 40), 60),
    ((2**31 - 1, 2**31 - 1, 2**31 - 1, 1, 2**31 - 1, 2**31 - 1, 1, 2**31 - 1), 0),
]


def random_classify_reads(rng, sizes):
    """reads of the given job counts with alignment scores that tie, dead jobs of every kind, both strands and poison under statuses"""
    reads = []
    for m in sizes:
        ql = int(rng.integers(50, 3000))
        mine = []
        for r in range(m):
            b = int(rng.integers(0, ql - 1))
            e = int(rng.integers(b + 1, ql + 1))
            score = int(rng.choice([0, 1, 77, 500, 500, 501, 1500, 40000]))
            st = int(rng.choice([0, 0, 0, 0, 1, 2, 5]))
            if rng.random() < 0.1:
                e = b  # an empty alignment
            a = (score, b, e) if st == 0 else (CANARY, CANARY, CANARY)
            mine.append((ltb.Job(None, r if rng.random() < 0.9 else max(r - 1, 0), int(rng.integers(0, 2)), int(rng.integers(1, 30)),
                                 int(rng.integers(1, 3000)), r, ql, 0), a, st))
        reads.append(mine)
    return reads


CLASSIFY_NAMES = ("lines", "n_lines", "primary_job", "status")


def classify_expected(batch, params):
    """-> (Classified, the four output arrays with PAD canaries behind each (8 * PAD behind the lines); canaries where no line is written)"""
    job_start, jobs, aln, st, cap = batch
    c = ltb.classify_alignments(job_start, jobs, cap, aln, st, *params)
    lines = np.full((cap + PAD, 8), CANARY, np.int32)
    for j, line in enumerate(c.lines):
        if line is not None:
            lines[j] = line
    pad = np.full(PAD, CANARY, np.int32)
    return c, [lines.reshape(-1)] + [np.concatenate([np.asarray(v, np.int32).reshape(-1), pad]) for v in (c.n_lines, c.primary_job, c.status)]


# ---------------------------------------------------------------------------------------------------------------- the pipeline's inputs

def compose(ranked, reads, window, buffer, parameters, band, zdrop, to_query_end, max_chains, keep_secondary=1, min_score=40, mask_level=128, query_pad=0):
    """The stages behind the rank stage, composed from the CPU textbooks: ``ranked`` = rank_textbook.rank_batch's tuple over the reads,
    ``window(q_len, anchor_start, anchor_t, anchor_q, anchor_len)`` = the window textbook over the jobs -> (t_start, t_len, rebased t,
    status[, rid]); the reads lie one behind the other in a buffer with ``query_pad`` spare bytes behind the last.  -> dict(expanded, located, aln [(score, q_beg, q_end)], full [ChainAln or None], cigars, aln_status, classified)"""
    import chain_textbook as atb
    import index_textbook as itb

    nc, recs, rs, rt, rq, rl, rst = ranked
    queries, q_start, q_len = itb.concat(reads)
    total = len(rt)
    cap = len(reads) * max_chains
    e = ltb.expand_chains(q_start, q_len, len(queries) + query_pad, rst, nc, recs, max_chains, rs, rt, rq, rl, total, keep_secondary, cap)
    pad = [0] * (total - len(e.job_anchor_t))
    located = window(e.job_q_len, e.job_anchor_start, e.job_anchor_t + pad, e.job_anchor_q + pad, e.job_anchor_len + pad)
    aln, full, cigars, status = [], [], [], []
    for j, job in enumerate(e.jobs):
        a, b = e.job_anchor_start[j], e.job_anchor_start[j + 1]
        if job.read < 0 or located[3][j] or a == b:
            aln.append((0, 0, 0)), full.append(None), cigars.append(""), status.append(located[3][j] or ltb.BAD_ARG)
            continue
        Q = bytes(reads[job.read])
        Q = ltb.revcomp(Q) if job.strand else Q
        T = buffer[located[0][j]:located[0][j] + located[1][j]]
        r, cigar, *_ = atb.chain_align(T, Q, [(located[2][i], e.job_anchor_q[i], e.job_anchor_len[i]) for i in range(a, b)], *parameters, band, zdrop, to_query_end)
        aln.append((r.score, r.q_beg, r.q_end)), full.append(r), cigars.append(cigar), status.append(0)
    c = ltb.classify_alignments(e.job_start, e.jobs, cap, aln, status, parameters[0], min_score, mask_level)
    return dict(expanded=e, located=located, aln=aln, full=full, cigars=cigars, aln_status=status, classified=c, q_start=q_start, q_len=q_len)


SPLIT = (1, 2)  # the reads of split_mapping_set(11, 8, 2000, 3000) behind contig_cases' reads: a plain chimera and one with its second part inverted


def contig_reads():
    """contig_cases' eleven reads and two split reads on the same reference (contig_mapping_set and split_mapping_set share
    mapping_set(11, 8, 2000, 3000)) -> (reads, the split reads' truth)"""
    import contig_cases as cc
    from mgl_amd import synth

    _, reads, _ = cc.pipeline_set()
    _, split, truth = synth.split_mapping_set(11, 8, length=2000, spacer=3000)
    return list(reads) + [split[p] for p in SPLIT], [truth[p] for p in SPLIT]


_CACHE = {}


def contig_composed(to_query_end, query_pad=0):
    """-> (buffer, start, length, names, reads, map_reads_contigs' tuple, compose's dict) over contig_reads()"""
    if (to_query_end, query_pad) in _CACHE:
        return _CACHE[(to_query_end, query_pad)]
    import contig_cases as cc
    import contig_textbook as gtb
    import index_cases as ic

    buffer, start, length, names, _, index, _ = cc.pipeline_textbook()
    reads, _ = contig_reads()
    seeding, chaining = cc.stage_args()
    ranking = tuple(cc.RANKING[f] for f in ("max_chains", "min_score", "min_cnt", "mask_level"))
    got = gtb.map_reads_contigs(index, len(buffer), start, length, reads, cc.K, cc.W, 2, *seeding, 2 * len(reads) * seeding[3], *chaining, ic.SLACK, ic.MAX_TL,
                                ranking=ranking)
    window = lambda *a: gtb.locate_window_contigs(start, length, *a, ic.SLACK, ic.MAX_TL)  # noqa: E731
    out = (buffer, start, length, names, reads, got, compose(got[6], reads, window, buffer, cc.GATK, cc.BAND, cc.ZDROP, to_query_end, ranking[0], query_pad=query_pad))
    _CACHE[(to_query_end, query_pad)] = out
    return out


def repeat_composed(divergence):
    """-> (ref, reads, copy, compose's dict) over rank_cases' repeat reads against a plain index, extension to the query's end"""
    key = ("repeat", divergence)
    if key not in _CACHE:
        import index_cases as ic
        import index_textbook as itb
        import rank_cases as rc

        ref, reads, _, copy, _, ranked = rc.repeat_mapped(divergence)
        window = lambda *a: itb.locate_window(len(ref), *a, ic.SLACK, ic.MAX_TL)  # noqa: E731
        _CACHE[key] = (ref, reads, copy, compose(ranked, reads, window, ref, (200, -150, 260, 11), 64, -1, True, rc.RANKING["max_chains"]))
    return _CACHE[key]
