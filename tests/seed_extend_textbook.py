"""The two-sided seed extension of mgl_sw_extend_seed_batch_device, written from its definition (include/mgl_sw.h)
and nothing else: the checker the GPU entry is compared against.  A composition of tests/extend_textbook.py (section 9c) and
tests/extend_adaptive_textbook.py (section 9d); nothing of either is restated here.

A target window T (tl >= 1), a query Q (ql >= 1) and a seed (st, sq, sl): T[st : st + sl] lies against Q[sq : sq + sl], sl >= 1, inside
both.  The seed is one `sl M` element, seed_score the sum of match / mismatch over its columns (seeds need not be exact).  The RIGHT side
is the extension of Q[sq + sl:] along T[st + sl:], the LEFT side the same function on reverse(T[:st]), reverse(Q[:sq]); band, zdrop and
the to-query-end request are the call's, on each side.  A side whose query flank is empty is the empty extension with score_qend 0 at
row 0; one whose target flank alone is empty has no cell in column ql: score_qend NO_QEND, t_end_qend -1.  Neither reaches the
extension function.

A side contributes the H of the cell its CIGAR starts from: score_qend where its cigar_from is 1, otherwise score.  The joined CIGAR is
reversed(left elements) + [sl M] + right elements with adjacent equal operations merged (only the seed's two neighbours can be).

seed_extend() returns (SeedAln, cigar text, left Ext, right Ext); the two Ext are in flank coordinates."""
import re
from collections import namedtuple

import extend_adaptive_textbook as eat
import extend_textbook as et

SeedAln = namedtuple("SeedAln", "score t_beg t_end q_beg q_end seed_score dropped cigar_from")

EMPTY_QUERY_FLANK = et.Ext(0, 0, 0, 0, 0, 0, 0, 0)
EMPTY_TARGET_FLANK = et.Ext(0, 0, 0, et.NO_QEND, -1, 0, 0, 0)


def elements(cigar):
    """CIGAR text -> [(length, op)]"""
    els = [(int(n), op) for n, op in re.findall(r"(\d+)([MID])", cigar)]
    assert "".join(f"{n}{op}" for n, op in els) == cigar
    return els


def text(els):
    return "".join(f"{n}{op}" for n, op in els)


def merged(els):
    out = []
    for n, op in els:
        if out and out[-1][1] == op:
            out[-1] = (out[-1][0] + n, op)
        else:
            out.append((n, op))
    return out


def side(t, q, params, band, zdrop, to_query_end, adaptive):
    """one side: (Ext, cigar text) of the extension of q along t, or the record of an empty flank"""
    if len(q) == 0:
        return EMPTY_QUERY_FLANK, ""
    if len(t) == 0:
        return EMPTY_TARGET_FLANK, ""
    small = len(t) * min(len(q), 2 * band + 1) <= 4000
    if adaptive:
        f = eat.extend_adaptive_align if small else eat.extend_adaptive_align_np
    else:
        f = et.extend_align if small else et.extend_align_np
    return f(t, q, *params, band, zdrop, to_query_end)


def walk_start(ext, ql):
    """the cell a side's CIGAR starts from and its H"""
    return (ext.t_end_qend, ql, ext.score_qend) if ext.cigar_from else (ext.t_end, ext.q_end, ext.score)


def seed_score(T, Q, st, sq, sl, match, mismatch):
    match, mismatch, _, _ = et.normalize(match, mismatch, 0, 0)
    return sum(match if T[st + k] == Q[sq + k] else mismatch for k in range(sl))


def seed_extend(T, Q, seed, match, mismatch, gopen, gext, band, zdrop, to_query_end=False, adaptive=False):
    T, Q = bytes(T), bytes(Q)
    st, sq, sl = seed
    tl, ql = len(T), len(Q)
    assert tl >= 1 and ql >= 1 and sl >= 1 and 0 <= st and st + sl <= tl and 0 <= sq and sq + sl <= ql and band >= 0
    params = (match, mismatch, gopen, gext)
    right, rc = side(T[st + sl:], Q[sq + sl:], params, band, zdrop, to_query_end, adaptive)
    left, lc = side(T[:st][::-1], Q[:sq][::-1], params, band, zdrop, to_query_end, adaptive)
    li, lj, lh = walk_start(left, sq)
    ri, rj, rh = walk_start(right, ql - sq - sl)
    ss = seed_score(T, Q, st, sq, sl, match, mismatch)
    aln = SeedAln(lh + ss + rh, st - li, st + sl + ri, sq - lj, sq + sl + rj, ss, left.dropped | right.dropped << 1,
                  left.cigar_from | right.cigar_from << 1)
    cigar = text(merged(elements(lc)[::-1] + [(sl, "M")] + elements(rc)))
    assert et.cigar_spans(cigar) == (aln.t_end - aln.t_beg, aln.q_end - aln.q_beg)
    return aln, cigar, left, right
