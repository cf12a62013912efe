"""The function of mgl_sw_chain_anchors_batch_device (include/mgl_sw.h), stated once in plain Python: a colinear
chaining DP over one read's candidate anchors, in integers only, and the best chain traced back.

A read is a window of tl and a query of ql bases and N >= 0 candidates (t, q, l): T[t .. t + l) lies against Q[q .. q + l).  The DP is
defined on index order alone.  j may precede i iff

    i - max_pred <= j < i,   dt = t_i - (t_j + l_j) >= 0,   dq = q_i - (q_j + l_j) >= 0,
    dt <= max_dist_t,   dq <= max_dist_q,   dd = |dt - dq| <= bw

    f(i)   = max( l_i , max_j f(j) + l_i - pen(j, i) )
    pen    = ((pen_gap * dd + pen_skip * min(dt, dq)) >> 8) + (ilog2(dd + 1) >> 1)

Ties go to the largest j, "no predecessor" counting as j = -1: a predecessor that only equals the current best replaces it.  pred(i)
is that j, relative to the read's first candidate.  The chain ends in the i with the largest f(i), ties to the smallest i, follows pred
to -1 and is emitted in ascending order; its score is f(end).  N = 0: an empty chain of score 0.

Statuses (mgl_sw_status): 1 (BAD_ARG) for tl or ql below 1 or a candidate with l < 1, t < 0, q < 0, t + l > tl or q + l > ql;
5 (UNSUPPORTED) for N > max_cand.  A refused read has an empty chain, score 0 and no f / pred.
"""
from collections import namedtuple

BAD_ARG, UNSUPPORTED = 1, 5

Chained = namedtuple("Chained", "status chain score f pred")  # chain: [(t, q, l)]; f, pred: lists of N ints (empty when refused)


def ilog2(x):
    """floor(log2(x)) for x >= 1"""
    return x.bit_length() - 1


def pen(dt, dq, pen_gap, pen_skip):
    dd = abs(dt - dq)
    return ((pen_gap * dd + pen_skip * min(dt, dq)) >> 8) + (ilog2(dd + 1) >> 1)


def guard_ok(max_dist_t, max_dist_q, bw, pen_gap, pen_skip):
    """the call's int32 guard of pen"""
    return pen_gap * bw + pen_skip * min(max_dist_t, max_dist_q) < 1 << 31


def chain_dp(tl, ql, cands, max_pred, max_dist_t, max_dist_q, bw, pen_gap, pen_skip, max_cand=None):
    """one read -> Chained"""
    assert 1 <= max_pred <= 64 and min(max_dist_t, max_dist_q, bw, pen_gap, pen_skip) >= 0
    assert guard_ok(max_dist_t, max_dist_q, bw, pen_gap, pen_skip)
    cands = [tuple(int(x) for x in c) for c in cands]
    n = len(cands)
    if tl < 1 or ql < 1 or any(l < 1 or t < 0 or q < 0 or t + l > tl or q + l > ql for t, q, l in cands):
        return Chained(BAD_ARG, [], 0, [], [])
    if max_cand is not None and n > max_cand:
        return Chained(UNSUPPORTED, [], 0, [], [])
    f, pred = [0] * n, [-1] * n
    for i, (ti, qi, li) in enumerate(cands):
        best, arg = li, -1
        for j in range(max(0, i - max_pred), i):
            tj, qj, lj = cands[j]
            dt, dq = ti - (tj + lj), qi - (qj + lj)
            if dt < 0 or dq < 0 or dt > max_dist_t or dq > max_dist_q or abs(dt - dq) > bw:
                continue
            s = f[j] + li - pen(dt, dq, pen_gap, pen_skip)
            if s >= best:
                best, arg = s, j
        f[i], pred[i] = best, arg
    if n == 0:
        return Chained(0, [], 0, [], [])
    end = max(range(n), key=lambda i: (f[i], -i))
    chain, i = [], end
    while i >= 0:
        chain.append(cands[i])
        i = pred[i]
    return Chained(0, chain[::-1], f[end], f, pred)


def chain_batch(t_lens, q_lens, cand_start, cand_t, cand_q, cand_len, max_cand, max_pred, max_dist_t, max_dist_q, bw, pen_gap, pen_skip):
    """The batch as the entry sees it: CSR arrays in, -> (chain_start [n + 1], chain_t, chain_q, chain_len (each chain_start[n] long),
    score [n], f, pred (one per candidate, None where no read wrote it), status [n]).  A range of cand_start that descends or leaves
    [0, total) is status 1."""
    n, total = len(t_lens), len(cand_t)
    start, ct, cq, cl, score, status = [0], [], [], [], [], []
    f, pred = [None] * total, [None] * total
    for p in range(n):
        a, b = int(cand_start[p]), int(cand_start[p + 1])
        if a < 0 or b < a or b > total:
            r = Chained(BAD_ARG, [], 0, [], [])
        else:
            r = chain_dp(int(t_lens[p]), int(q_lens[p]), list(zip(cand_t[a:b], cand_q[a:b], cand_len[a:b])), max_pred, max_dist_t, max_dist_q, bw, pen_gap,
                         pen_skip, max_cand)
        if r.f:
            f[a:b], pred[a:b] = r.f, r.pred
        for t, q, l in r.chain:
            ct.append(t), cq.append(q), cl.append(l)
        start.append(len(ct))
        score.append(r.score)
        status.append(r.status)
    return start, ct, cq, cl, score, f, pred, status
