"""The anchored extension of mgl_sw_extend_batch_device, written from its definition (include/mgl_sw.h) and nothing
else: the checker the GPU kernel is compared against.

A target t (tl >= 1), a query q (ql >= 1), match / mismatch / gopen / gext normalised as everywhere (a gap of k costs o + (k - 1) e),
band >= 0 and zdrop (< 0: off).  A cell (i, j), border row and column included, is in the band iff -band <= j - i <= band.  The start
is anchored: H(0, 0) = 0 and the in-band border cells are gap penalties, H(0, j) = -(o + (j - 1) e), H(i, 0) = -(o + (i - 1) e).  The
interior is the affine recurrence with the library's priorities: the diagonal wins ties, then the horizontal gap; a gap opens only
where that is strictly better than extending; a value read from an out-of-band cell is minus infinity.

Per row i: rowmax(i) the largest H over the row's in-band cells (the border column while i <= band, the border row for i = 0), rj(i)
the smallest column that holds it; best(i) the largest H over rows 0 .. i, at the smallest row, then the smallest column.  A row
without in-band cells (i > ql + band) has rowmax = minus infinity.  Row i >= 1 DROPS iff zdrop >= 0 and

    best(i - 1).H - rowmax(i) > zdrop + e * |(i - best(i - 1).i) - (rj(i) - best(i - 1).j)|

(so an empty row drops whenever the rule is on).  rows_done = (first dropping row) - 1, or tl; no later row exists for any output.

extend_align() is the plain form, one cell at a time; extend_align_np() the same function one row at a time for long pairs (the two
agree on every output: tests/test_extend_textbook.py).  Both return (Ext, cigar text).  The last part mirrors
mgl_amd/csrc/sw_extend.h: one pair's workspace slot."""
from collections import namedtuple

import numpy as np

NEG = -(1 << 60)      # minus infinity: anything at or below NEG_LIMIT is it
NEG_LIMIT = -(1 << 59)
NO_QEND = -0x40000000

Ext = namedtuple("Ext", "score t_end q_end score_qend t_end_qend rows_done dropped cigar_from")


def normalize(match, mismatch, gopen, gext):
    return abs(match), -abs(mismatch), abs(gopen), abs(gext)


def _minus(v, k):
    return NEG if v <= NEG_LIMIT else v - k


def _gap(k, o, e):
    return -o - (k - 1) * e if k > 0 else 0


def drops(best, i, rowmax, rj, zdrop, e):
    """the Z-drop predicate of row i against best = best(i - 1) = (H, i, j)"""
    if zdrop < 0:
        return False
    if rowmax <= NEG_LIMIT:
        return True
    return best[0] - rowmax > zdrop + e * abs((i - best[1]) - (rj - best[2]))


def walk(mark_at, I, J):
    """From (I, J) back to (0, 0) over the marks (+k: k rows up, -k: k columns left, 0: diagonal): M / I / D only, global on the prefix
    pair; a walk that reaches row 0 or column 0 finishes with one I or D run."""
    if I == 0 and J == 0:
        return ""
    assert I >= 1 and J >= 1
    el, state, seg = [], "M", 0  # last element first
    while True:
        b = mark_at(I, J)
        if b > 0:
            nxt, step = "D", b
            I -= b
        elif b < 0:
            nxt, step = "I", -b
            J += b
        else:
            nxt, step = "M", 1
            I, J = I - 1, J - 1
        if nxt == state:
            seg += step
        else:
            el.append((state, seg))
            seg, state = step, nxt
        if not (I > 0 and J > 0):
            break
    el.append((state, seg))
    if I > 0:
        el.append(("D", I))
    elif J > 0:
        el.append(("I", J))
    return "".join(f"{n}{op}" for op, n in reversed(el) if n > 0)


def _result(best, qend, rows_done, dropped, ql, to_query_end, mark_at):
    cigar_from = 1 if (to_query_end and qend[1] >= 1) else 0
    I, J = (qend[1], ql) if cigar_from else (best[1], best[2])
    return Ext(best[0], best[1], best[2], qend[0], qend[1], rows_done, dropped, cigar_from), walk(mark_at, I, J)


def extend_align(t, q, match, mismatch, gopen, gext, band, zdrop, to_query_end=False, trace=None):
    """The plain form.  trace: a list that receives (i, rowmax(i), rj(i), best(i - 1)) for every row looked at."""
    match, mismatch, o, e = normalize(match, mismatch, gopen, gext)
    tl, ql = len(t), len(q)
    assert tl >= 1 and ql >= 1 and band >= 0
    inb = lambda i, j: -band <= j - i <= band  # noqa: E731
    hrow = [_gap(j, o, e) if inb(0, j) else NEG for j in range(ql + 1)]
    ecol = [_minus(hrow[j], o) for j in range(ql + 1)]
    vrun = [1] * (ql + 1)
    marks = {}
    best = (0, 0, 0)
    qend = (NO_QEND, -1)
    rows_done, dropped = tl, 0
    for i in range(1, tl + 1):
        nrow = [NEG] * (ql + 1)
        nrow[0] = _gap(i, o, e) if inb(i, 0) else NEG
        f, hrun = _minus(nrow[0], o), 1
        rowmax, rj = nrow[0], 0
        necol, nvrun, nmarks = list(ecol), list(vrun), {}
        for j in range(max(1, i - band), min(ql, i + band) + 1):
            diag = hrow[j - 1] + (match if t[i - 1] == q[j - 1] else mismatch)
            assert hrow[j - 1] > NEG_LIMIT  # the diagonal predecessor of an in-band cell is in the band
            down = ecol[j] if inb(i - 1, j) else NEG
            right = f if inb(i, j - 1) else NEG
            if diag >= down and diag >= right:
                h, mark = diag, 0
            elif right >= down:
                h, mark = right, -hrun
            else:
                h, mark = down, vrun[j]
            nmarks[(i, j)] = mark
            if h - o > _minus(down, e):
                necol[j], nvrun[j] = h - o, 1
            else:
                necol[j], nvrun[j] = down - e, vrun[j] + 1
            if h - o > _minus(right, e):
                f, hrun = h - o, 1
            else:
                f, hrun = right - e, hrun + 1
            nrow[j] = h
            if h > rowmax:
                rowmax, rj = h, j
        if trace is not None:
            trace.append((i, rowmax, rj, best))
        if drops(best, i, rowmax, rj, zdrop, e):
            rows_done, dropped = i - 1, 1
            break
        hrow, ecol, vrun = nrow, necol, nvrun
        marks.update(nmarks)
        if rowmax > best[0]:
            best = (rowmax, i, rj)
        if inb(i, ql) and hrow[ql] >= qend[0]:
            qend = (hrow[ql], i)
    return _result(best, qend, rows_done, dropped, ql, to_query_end, lambda i, j: marks[(i, j)])


def extend_align_np(t, q, match, mismatch, gopen, gext, band, zdrop, to_query_end=False):
    """The same function one row at a time (numpy).  Row i's in-band columns are a slice; with gopen >= gext the F of a row is a running
    maximum (an H that F made never opens a better gap than extending the one it came from), otherwise the row is done cell by cell.
    Marks are kept band-relative: marks[i][j - (i - band)]."""
    match, mismatch, o, e = normalize(match, mismatch, gopen, gext)
    tl, ql = len(t), len(q)
    assert tl >= 1 and ql >= 1 and band >= 0
    band = min(band, max(tl, ql))  # (a wider band holds the same cells)
    ta = np.frombuffer(bytes(t), np.uint8)
    qa = np.frombuffer(bytes(q), np.uint8)
    marks = []
    cols = np.arange(ql + 1, dtype=np.int64)
    hrow = np.where(cols <= band, np.where(cols > 0, -o - (cols - 1) * e, 0), NEG)
    ecol = np.where(hrow > NEG_LIMIT, hrow - o, NEG)
    vrun = np.ones(ql + 1, np.int64)
    best = (0, 0, 0)
    qend = (NO_QEND, -1)
    rows_done, dropped = tl, 0
    for i in range(1, tl + 1):
        a, b = max(1, i - band), min(ql, i + band)
        n = b - a + 1
        h0 = _gap(i, o, e) if i <= band else NEG
        if n <= 0:  # the band has left the matrix
            if drops(best, i, NEG, 0, zdrop, e):
                rows_done, dropped = i - 1, 1
                break
            marks.append(None)
            continue
        js = cols[a:b + 1]
        f0 = _minus(h0 if a == 1 else NEG, o)
        diag = hrow[a - 1:b] + np.where(qa[a - 1:b] == ta[i - 1], match, mismatch)
        down = ecol[a:b + 1].copy()
        if b == i + band:
            down[-1] = NEG  # (i - 1, b) is above the band
        vr = vrun[a:b + 1]
        hv = np.maximum(diag, down)
        if o >= e:
            k = js - a
            g = np.empty(n, np.int64)
            g[0] = f0
            g[1:] = hv[:-1] - o + (k[:-1] + 1) * e  # opened behind column a + k', seen from column a
            run = np.maximum.accumulate(g)
            F = np.where(run > NEG_LIMIT, run - k * e, NEG)
            H = np.maximum(hv, F)
        else:
            F = np.empty(n, np.int64)
            H = np.empty(n, np.int64)
            fv = f0
            for x in range(n):
                F[x] = fv
                H[x] = max(int(hv[x]), fv)
                fv = max(int(H[x]) - o, _minus(fv, e))
        Fe = np.where(F > NEG_LIMIT, F - e, NEG)
        De = np.where(down > NEG_LIMIT, down - e, NEG)
        f_open = H - o > Fe
        e_open = H - o > De
        idx = np.arange(n)
        last_open = np.maximum.accumulate(np.where(np.concatenate(([True], f_open[:-1])), idx, -1))
        hrun = idx - last_open + 1  # the horizontal run entering each cell
        is_diag = (diag >= down) & (diag >= F)
        is_right = ~is_diag & (F >= down)
        x = int(np.argmax(H))  # the first of the largest
        rowmax, rj = (int(H[x]), a + x) if int(H[x]) > h0 else (h0, 0)
        if drops(best, i, rowmax, rj, zdrop, e):
            rows_done, dropped = i - 1, 1
            break
        marks.append(np.where(is_diag, 0, np.where(is_right, -hrun, vr)).astype(np.int32))
        ecol[a:b + 1] = np.where(e_open, H - o, De)
        vrun[a:b + 1] = np.where(e_open, 1, vr + 1)
        hrow = np.full(ql + 1, NEG, np.int64)
        hrow[0] = h0
        hrow[a:b + 1] = H
        if rowmax > best[0]:
            best = (rowmax, i, rj)
        if b == ql and int(H[-1]) >= qend[0]:
            qend = (int(H[-1]), i)

    def at(i, j):
        assert -band <= j - i <= band
        return int(marks[i - 1][j - max(1, i - band)])

    return _result(best, qend, rows_done, dropped, ql, to_query_end, at)


def cigar_spans(cigar):
    """(target bases, query bases) a CIGAR text spends"""
    import re

    els = [(int(n), op) for n, op in re.findall(r"(\d+)([MID])", cigar)]
    assert "".join(f"{n}{op}" for n, op in els) == cigar
    return sum(n for n, op in els if op in "MD"), sum(n for n, op in els if op in "MI")


def cigar_score(cigar, t, q, match, mismatch, gopen, gext):
    """the score of the global alignment of the prefix pair that a CIGAR text describes"""
    import re

    match, mismatch, o, e = normalize(match, mismatch, gopen, gext)
    i = j = s = 0
    for n, op in re.findall(r"(\d+)([MID])", cigar):
        n = int(n)
        if op == "M":
            s += sum(match if t[i + x] == q[j + x] else mismatch for x in range(n))
            i, j = i + n, j + n
        else:
            s -= o + (n - 1) * e
            if op == "I":
                j += n
            else:
                i += n
    return s


def cigar_binary_to_text(words):
    """BAM-style uint32 elements (len << 4 | op, M=0 I=1 D=2) -> text."""
    return "".join(f"{int(w) >> 4}{'MID'[int(w) & 15]}" for w in words)


# ---- mirror of mgl_amd/csrc/sw_extend.h: one pair's workspace slot (the range guard is the banded entry's, banded_range_ok)
def extend_strip_steps(ql, band):
    return (min(ql, 2 * band + 64) + 63 + 7) & ~7


def extend_pair_bytes(tl, ql, band, score_only=False):
    r = lambda x: (x + 255) // 256 * 256  # noqa: E731
    carry, elems = r((ql + 1) * 8), r((tl + ql + 4) * 4)
    return carry + (0 if score_only else elems + 32 * ((tl + 63) // 64) * extend_strip_steps(ql, band))


def extend_slot_bytes(max_tl, max_ql, band, score_only=False):
    """What the host sizes every slot with: the formula is monotone in tl and ql, so the largest pair the bounds admit is the bounds."""
    return extend_pair_bytes(max_tl, max_ql, min(band, max(max_tl, max_ql)), score_only)
