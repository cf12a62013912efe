"""The function of mgl_sw_rank_chains_batch_device (include/mgl_sw.h), stated once in plain Python on top of
chain_dp_textbook.py, which says what f and pred are: the best ``max_chains`` chains of every read, ranked, marked primary or secondary
and given a mapping quality, in integers only.

Rows and reads.  Read p has ``strands`` rows (1 or 2), rows strands * p .. strands * p + strands - 1.  Row r has its candidates (t, q, l)
at cand_start[r] .. cand_start[r + 1], the chain stage's f and pred for them (pred relative to the row's first candidate, -1: none),
row_q_len[r] and, optionally, the chain stage's status row_status[r].

The chains of a row (row_chains).  The candidates are visited by (f descending, index ascending).  An unused candidate e with
f(e) >= min_score starts a walk: i = e; while i >= 0 and i is unused, i is marked used, counted, remembered as `first`, and i = pred(i).
The chain's score is f(e) where the walk reached -1 and f(e) - f(i) where the used candidate i stopped it.  The chain is kept iff
score >= min_score and its anchor count K >= min_cnt; a dropped chain's candidates stay used.  The visit ends at the first unused candidate
with f < min_score.  A chain: strand (its row minus strands * p), end_index e, K, t_beg = t_first, t_end = t_e + l_e, q_beg = q_first,
q_end = q_e + l_e, in the row's own oriented coordinates.

Ranking.  The kept chains of a read's rows by (score descending, strand ascending, end_index ascending), cut to max_chains.

Primary and secondary.  A chain's interval on the FORWARD read is [q_beg, q_end) for strand 0 and [ql - q_end, ql - q_beg) for strand 1.
In rank order, chain c looks at the earlier chains p that are their own parent, in rank order: ov = max(0, min(ends) - max(begins)); if
ov * 256 >= mask_level * min(len_c, len_p) then parent(c) = p, n_sub(p) += 1, subsc(p) = max(subsc(p), score(c)) and the search stops.
Otherwise c is its own parent: primary.  Parents are computed over the cut list only.

Mapping quality (mapq): minimap2's chain-only formula in integers.  lg8(x) = (e << 8) + (((x << 8) >> e) - 256) with e = ilog2(x) is
log2 in 1/256 units with a linear mantissa.  For a primary chain sub = min(score, max(subsc, min_score)),
raw = (40 * min(K, 10) * (score - sub) * lg8(score) * 177) // (10 * score * 65536) and
mapq = clamp(raw - ((3 * lg8(n_sub + 1) + 128) >> 8), 0, 60).  A secondary chain has mapq 0, n_sub 0 and subsc 0.

Statuses per read (mgl_sw_status): 1 (BAD_ARG) for a row with row_q_len < 1 or a range of cand_start that descends or leaves
[0, total_cand], or a pred(i) outside [-1, i) or more than 64 behind i; then 5 (UNSUPPORTED) for a row with more than max_cand
candidates.  A refused read has no chains.  A row whose row_status is not 0 contributes no chains and its f / pred are never looked at
(the chain stage left them unwritten); its length, range and candidate count are still checked.  A read with no kept chain is status 0
with no chains.

The candidates themselves are the chain stage's: those it accepted (l >= 1, t, q >= 0, q + l <= ql), and f its scores (1 <= f < 2^31).
"""
from collections import namedtuple

from chain_dp_textbook import ilog2

BAD_ARG, UNSUPPORTED = 1, 5
MAX_PRED = 64

FIELDS = "score strand n_anchors t_beg t_end q_beg q_end parent n_sub subsc mapq end_index"
Ranked = namedtuple("Ranked", FIELDS)  # the twelve int32 of mgl_sw_ranked_chain, in its order


def lg8(x):
    """log2(x) in 1/256 units with a linear mantissa, x >= 1"""
    e = ilog2(x)
    return (e << 8) + (((x << 8) >> e) - 256)


def mapq(score, sub, k, n_sub):
    raw = (40 * min(k, 10) * (score - sub) * lg8(score) * 177) // (10 * score * 65536)
    return max(0, min(60, raw - ((3 * lg8(n_sub + 1) + 128) >> 8)))


def pred_ok(pred):
    return all(p == -1 or (0 <= p < i and i - p <= MAX_PRED) for i, p in enumerate(pred))


def row_chains(cands, f, pred, min_score, min_cnt):
    """one row -> its kept chains [(score, end_index, K, first)] in the order of the visit"""
    n = len(cands)
    used = [False] * n
    out = []
    for e in sorted(range(n), key=lambda i: (-f[i], i)):
        if used[e]:
            continue
        if f[e] < min_score:
            break
        i, k, first = e, 0, e
        while i >= 0 and not used[i]:
            used[i] = True
            k += 1
            first = i
            i = pred[i]
        score = f[e] if i < 0 else f[e] - f[i]
        if score >= min_score and k >= min_cnt:
            out.append((score, e, k, first))
    return out


def chain_anchors(pred, e, k):
    """the K candidates of a kept chain, ascending"""
    idx = []
    for _ in range(k):
        idx.append(e)
        e = pred[e]
    return idx[::-1]


def rank_read(rows, max_cand, max_chains, min_score, min_cnt, mask_level):
    """One read: ``rows`` = per strand (ql, cands, f, pred, row_status), ranges already cut.  -> (status, [Ranked], anchors: per ranked
    chain its [(t, q, l)] ascending)"""
    assert 1 <= max_chains <= 16 and min_score >= 1 and min_cnt >= 1 and 1 <= mask_level <= 256
    if any(ql < 1 for ql, *_ in rows) or any(st == 0 and not pred_ok(pred) for _, _, _, pred, st in rows):
        return BAD_ARG, [], []
    if any(len(cands) > max_cand for _, cands, *_ in rows):
        return UNSUPPORTED, [], []
    kept = []
    for strand, (ql, cands, f, pred, st) in enumerate(rows):
        if st == 0:
            kept += [(-score, strand, e, k, first) for score, e, k, first in row_chains(cands, f, pred, min_score, min_cnt)]
    kept = sorted(kept)[:max_chains]
    m = len(kept)
    score = [-c[0] for c in kept]
    span, recs = [], []
    for _, strand, e, k, first in kept:
        ql, cands = rows[strand][0], rows[strand][1]
        qb, qe = cands[first][1], cands[e][1] + cands[e][2]
        span.append((ql - qe, ql - qb) if strand else (qb, qe))
    parent, n_sub, subsc = list(range(m)), [0] * m, [0] * m
    for c in range(m):
        for p in range(c):
            if parent[p] != p:
                continue
            ov = max(0, min(span[c][1], span[p][1]) - max(span[c][0], span[p][0]))
            if ov * 256 >= mask_level * min(span[c][1] - span[c][0], span[p][1] - span[p][0]):
                parent[c] = p
                n_sub[p] += 1
                subsc[p] = max(subsc[p], score[c])
                break
    anchors = []
    for c, (_, strand, e, k, first) in enumerate(kept):
        cands, pred = rows[strand][1], rows[strand][3]
        prim = parent[c] == c
        q = mapq(score[c], min(score[c], max(subsc[c], min_score)), k, n_sub[c]) if prim else 0
        recs.append(Ranked(score[c], strand, k, cands[first][0], cands[e][0] + cands[e][2], cands[first][1], cands[e][1] + cands[e][2], parent[c],
                           n_sub[c] if prim else 0, subsc[c] if prim else 0, q, e))
        anchors.append([cands[i] for i in chain_anchors(pred, e, k)])
    return 0, recs, anchors


def rank_batch(strands, row_q_len, cand_start, cand_t, cand_q, cand_len, f, pred, row_status, max_cand, max_chains, min_score, min_cnt, mask_level,
               total_cand=None):
    """The batch as the entry sees it: -> (n_chains [n], records: per read its [Ranked], ranked_start [n + 1], ranked_t, ranked_q,
    ranked_len (the kept chains' anchors, read after read in rank order), status [n])."""
    rows_n = len(row_q_len)
    assert strands in (1, 2) and rows_n % strands == 0
    total = len(cand_t) if total_cand is None else total_cand
    n_chains, records, start, rt, rq, rl, status = [], [], [0], [], [], [], []
    for p in range(rows_n // strands):
        rows, bad = [], False
        for r in range(strands * p, strands * p + strands):
            a, b = int(cand_start[r]), int(cand_start[r + 1])
            st = 0 if row_status is None else int(row_status[r])
            if a < 0 or b < a or b > total:
                bad = True
                continue
            cands = [(int(cand_t[i]), int(cand_q[i]), int(cand_len[i])) for i in range(a, b)]
            rows.append((int(row_q_len[r]), cands, [int(x) for x in f[a:b]] if st == 0 else None, [int(x) for x in pred[a:b]] if st == 0 else None, st))
        s, recs, anchors = (BAD_ARG, [], []) if bad else rank_read(rows, max_cand, max_chains, min_score, min_cnt, mask_level)
        for chain in anchors:
            for t, q, l in chain:
                rt.append(t), rq.append(q), rl.append(l)
        n_chains.append(len(recs)), records.append(recs), start.append(len(rt)), status.append(s)
    return n_chains, records, start, rt, rq, rl, status
