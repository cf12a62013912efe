"""The chain alignment of mgl_sw_align_chain_batch_device, written from its definition (include/mgl_sw.h) and nothing
else: the checker the GPU entry is compared against.  A composition of tests/seed_extend_textbook.py (section 9e: the two sides, the
records of an empty flank, cigar_from, what a side contributes -- none of it restated here) and tests/banded_textbook.py (section 9b:
the gap's band rule, recurrence, priorities, run lengths, minus infinity and walk).

A target window T (tl >= 1), a query Q (ql >= 1) and K >= 1 anchors (st_k, sq_k, sl_k), sl_k >= 1: T[st_k : st_k + sl_k] lies against
Q[sq_k : sq_k + sl_k];  0 <= st_0, 0 <= sq_0;  st_k + sl_k <= st_(k+1) and sq_k + sl_k <= sq_(k+1);  the last anchor ends inside T and Q.

  Anchors   one `sl_k M` element each; anchor_score is the sum of match / mismatch over all anchors' columns (anchors need not be exact).
  Sides     the LEFT side of anchor 0 (on the reversed flanks) and the RIGHT side of anchor K - 1 are seed_extend_textbook.side()'s,
            with the call's band, zdrop, to-query-end request and adaptive flag.
  Gap k     T[st_k + sl_k : st_(k+1)] against Q[sq_k + sl_k : sq_(k+1)], gt and gq bases.  gt = gq = 0: no element, score 0.
            gt = 0 < gq: `gq I`, score -(o + (gq - 1) e).  gq = 0 < gt: `gt D`, likewise.  Otherwise the GLOBAL FILL: the banded
            function under INDEL -- lo = min(0, gq - gt) - band, hi = max(0, gq - gt) + band, so both corners are in the band;
            gap-penalty borders on both axes -- whose CIGAR is the banded walk from (gt, gq) back to (0, 0) and whose score is
            H(gt, gq), the corner, which banded_textbook does not return: gap_corner() below computes it, values only.  Always the
            plain band rule: the adaptive flag is the sides'.  LIMIT: no Z-drop inside a gap; it is aligned end to end at any cost.
            With gopen >= gext the gap's CIGAR re-scored with affine costs is H(gt, gq), and so the joined CIGAR's is `score`.
  Record    score = left + anchors + gaps + right; the spans half open; anchor_score; dropped and cigar_from as in section 9e.  For
            K = 1 it is seed_extend_textbook's record.
  CIGAR     reversed left elements, anchor 0, gap 0, anchor 1, ..., anchor K - 1, right elements, adjacent equal operations merged
            (only an M next to an anchor can be; two anchors merge across an empty gap).

chain_align() returns (ChainAln, cigar text, left Ext, right Ext, gap scores): one gap score per anchor, 0 for the last.  The last part
mirrors mgl_amd/csrc/sw_chain.h: the sum guard."""
import functools
from collections import namedtuple

import numpy as np

import banded_textbook as bt
import extend_textbook as et
import seed_extend_textbook as stb

ChainAln = namedtuple("ChainAln", "score t_beg t_end q_beg q_end anchor_score dropped cigar_from")


def chain_ok(tl, ql, anchors):
    """the inequalities a chain must satisfy"""
    if tl < 1 or ql < 1 or len(anchors) < 1:
        return False
    for k, (st, sq, sl) in enumerate(anchors):
        nt, nq = (anchors[k + 1][0], anchors[k + 1][1]) if k + 1 < len(anchors) else (tl, ql)
        if not (sl >= 1 and st >= 0 and sq >= 0 and st + sl <= nt and sq + sl <= nq):
            return False
    return True


def gap_corner(t, q, match, mismatch, gopen, gext, band):
    """H(gt, gq) of the banded fill with gap-penalty borders: the values only, one row at a time.  A value read from an out-of-band
    cell is minus infinity."""
    match, mismatch, o, e = bt.normalize(match, mismatch, gopen, gext)
    gt, gq = len(t), len(q)
    assert gt >= 1 and gq >= 1 and band >= 0
    lo, hi = bt.band_limits(gt, gq, band)
    NEG, LIM = bt.NEG, bt.NEG_LIMIT
    ta, qa = np.frombuffer(bytes(t), np.uint8), np.frombuffer(bytes(q), np.uint8)
    cols = np.arange(gq + 1, dtype=np.int64)
    H = np.where(cols <= hi, np.where(cols > 0, -o - (cols - 1) * e, 0), NEG)  # row 0
    E = np.where(H > LIM, H - o, NEG)                                          # E entering the next row, per column
    for i in range(1, gt + 1):
        a, b = max(1, i + lo), min(gq, i + hi)
        h0 = -o - (i - 1) * e if -i >= lo else NEG                             # H[i][0]
        diag = H[a - 1:b] + np.where(qa[a - 1:b] == ta[i - 1], match, mismatch)
        assert (H[a - 1:b] > LIM).all()                                        # the diagonal predecessor of an in-band cell is in the band
        down = E[a:b + 1].copy()
        if b == i + hi:
            down[-1] = NEG                                                     # (i - 1, b) is above the band
        hv = np.maximum(diag, down)
        f = h0 - o if (a == 1 and h0 > LIM) else NEG                           # F entering column a
        row = np.empty(b - a + 1, np.int64)
        for x in range(b - a + 1):
            h = max(int(hv[x]), f)
            row[x] = h
            f = max(h - o, f - e if f > LIM else NEG)
        E[a:b + 1] = np.maximum(row - o, np.where(down > LIM, down - e, NEG))
        H = np.full(gq + 1, NEG, np.int64)
        H[0] = h0
        H[a:b + 1] = row
    assert H[gq] > LIM
    return int(H[gq])


@functools.lru_cache(maxsize=None)
def gap_fill(t, q, match, mismatch, gopen, gext, band):
    """one gap: (score, cigar text); remembered, since the sweeps of the tests meet the same gap under many flags"""
    _, _, o, e = bt.normalize(match, mismatch, gopen, gext)
    gt, gq = len(t), len(q)
    if gt == 0 or gq == 0:
        g = gt + gq
        return (-(o + (g - 1) * e), f"{g}{'I' if gq else 'D'}") if g else (0, "")
    f = bt.banded_align if gt * min(gq, 2 * band + abs(gq - gt) + 1) <= 4000 else bt.banded_align_np
    off, _, cigar = f(t, q, match, mismatch, gopen, gext, bt.INDEL, band)
    assert off == 0 and et.cigar_spans(cigar) == (gt, gq)
    score = gap_corner(t, q, match, mismatch, gopen, gext, band)
    # the walk follows the decisions that made the corner.  (With gopen < gext the recurrence may open a gap right behind a gap, the
    # walk writes the two runs as one element, and the CIGAR re-scored is not H any more: the score stays H(gt, gq))
    assert o < e or et.cigar_score(cigar, t, q, match, mismatch, gopen, gext) == score
    return score, cigar


def chain_align(T, Q, anchors, match, mismatch, gopen, gext, band, zdrop, to_query_end=False, adaptive=False):
    T, Q = bytes(T), bytes(Q)
    anchors = [tuple(int(x) for x in a) for a in anchors]
    tl, ql = len(T), len(Q)
    assert chain_ok(tl, ql, anchors) and band >= 0
    params = (match, mismatch, gopen, gext)
    st0, sq0, _ = anchors[0]
    tend, qend = anchors[-1][0] + anchors[-1][2], anchors[-1][1] + anchors[-1][2]
    right, rc = stb.side(T[tend:], Q[qend:], params, band, zdrop, to_query_end, adaptive)
    left, lc = stb.side(T[:st0][::-1], Q[:sq0][::-1], params, band, zdrop, to_query_end, adaptive)
    li, lj, lh = stb.walk_start(left, sq0)
    ri, rj, rh = stb.walk_start(right, ql - qend)
    els = stb.elements(lc)[::-1]
    ascore, gaps = 0, []
    for k, (st, sq, sl) in enumerate(anchors):
        ascore += stb.seed_score(T, Q, st, sq, sl, match, mismatch)
        els.append((sl, "M"))
        if k + 1 < len(anchors):
            nt, nq, _ = anchors[k + 1]
            gs, gc = gap_fill(T[st + sl:nt], Q[sq + sl:nq], *params, band)
            gaps.append(gs)
            els += stb.elements(gc)
    gaps.append(0)
    els += stb.elements(rc)
    aln = ChainAln(lh + ascore + sum(gaps) + rh, st0 - li, tend + ri, sq0 - lj, qend + rj, ascore, left.dropped | right.dropped << 1,
                   left.cigar_from | right.cigar_from << 1)
    cigar = stb.text(stb.merged(els))
    assert et.cigar_spans(cigar) == (aln.t_end - aln.t_beg, aln.q_end - aln.q_beg)
    return aln, cigar, left, right, gaps


def mirror_anchors(tl, ql, anchors):
    """the chain as the reversed sequences see it"""
    return [(tl - st - sl, ql - sq - sl, sl) for st, sq, sl in reversed(anchors)]


# ---- mirror of mgl_amd/csrc/sw_chain.h: the sum guard, on the normalised parameters
CHAIN_MAX_SUM = 1 << 30


def chain_sum_ok(tl, ql, k, match, mismatch, gopen, gext):
    return max(match, -mismatch) * min(tl, ql) + 2 * gopen * (k + 1) + gext * (tl + ql) <= CHAIN_MAX_SUM
