"""mgl_sw_extend_batch_device with MGL_SW_FLAG_EXTEND_ADAPTIVE_BAND, written from its definition (include/mgl_sw.h)
and nothing else: the checker the GPU kernel is compared against.  Everything is tests/extend_textbook.py's (section 9c) except the band,
which is re-centred every R = 64 rows:

Rows are grouped in blocks of R: row i >= 1 is in block b = (i - 1) // R, row 0 counts with block 0.  Block b has a centre d_b, d_0 = 0,
and a cell (i, j), border cells included, is in the band iff d_b - band <= j - i <= d_b + band for the block b of ITS OWN ROW.  For
b >= 1, d_b = rj(R b) - R b: the diagonal of the smallest column that holds the largest in-band H of row R b (the border column included
where it is in that row's band); where row R b has no in-band cell, d_b = d_(b-1) (and every later row is empty too).  A cell has one
band, its row's, and an out-of-band cell is minus infinity for every reader: row R b + 1 reads H and E of row R b only where row R b had
them under d_(b-1).  So the diagonal predecessor of an in-band cell may be out of the band now, and a band that moved left holds cells no
path reaches: their H is minus infinity, they take no part in any maximum, and a row that has a cell always has a finite one (asserted).
|d_b - d_(b-1)| <= band follows (rj(R b) lies in row R b's band) and is asserted, not clamped.  The border column is in the band of row i
whenever i + d_b - band <= 0, H(i, 0) = -(o + (i - 1) e) as before; a row has a cell iff i + d_b - band <= ql.

rowmax, rj, best, the drop predicate, rows_done, dropped, score_qend / t_end_qend, cigar_from, the walk and its tie rules are section
9c's, evaluated over this band.  Two identities: a pair with tl <= R, and any pair at band >= tl + ql, give the flag-off result.

extend_adaptive_align() is the plain form, one cell at a time; extend_adaptive_align_np() the same function one row at a time for long
pairs (tests/test_extend_adaptive_textbook.py: the two agree on every output).  Both return (Ext, cigar text); `centres`: a list that
receives d_0, d_1, ... of the blocks looked at.  The last part mirrors mgl_amd/csrc/sw_extend.h: one pair's workspace slot."""
import numpy as np

from extend_textbook import NEG, NEG_LIMIT, NO_QEND, _gap, _minus, _result, drops, extend_pair_bytes, normalize

R = 64  # MGL_SW_EXTEND_RECENTRE_ROWS: part of the function's definition


def _next_centre(d, i, rj, has_cell, band):
    """d of the block that starts behind row i (a multiple of R), from that row's rj"""
    if not has_cell:
        return d
    nd = rj - i
    assert abs(nd - d) <= band, (d, nd, band)
    return nd


def extend_adaptive_align(t, q, match, mismatch, gopen, gext, band, zdrop, to_query_end=False, centres=None):
    """The plain form."""
    match, mismatch, o, e = normalize(match, mismatch, gopen, gext)
    tl, ql = len(t), len(q)
    assert tl >= 1 and ql >= 1 and band >= 0
    d = 0
    if centres is not None:
        centres.append(d)
    hrow = [_gap(j, o, e) if -band <= j <= band else NEG for j in range(ql + 1)]  # out-of-band cells are NEG, in every row kept
    ecol = [_minus(hrow[j], o) for j in range(ql + 1)]
    vrun = [1] * (ql + 1)
    marks = {}
    best = (0, 0, 0)
    qend = (NO_QEND, -1)
    rows_done, dropped = tl, 0
    rj, has_cell = 0, True  # of the row above
    for i in range(1, tl + 1):
        if i > 1 and (i - 1) % R == 0:
            d = _next_centre(d, i - 1, rj, has_cell, band)
            if centres is not None:
                centres.append(d)
        lo, hi = d - band, d + band
        has_cell = i + lo <= ql
        nrow, necol, nvrun = [NEG] * (ql + 1), [NEG] * (ql + 1), [1] * (ql + 1)
        nrow[0] = _gap(i, o, e) if i + lo <= 0 else NEG
        f, hrun = _minus(nrow[0], o), 1
        rowmax, rj = nrow[0], 0
        for j in range(max(1, i + lo), min(ql, i + hi) + 1):
            diag = hrow[j - 1] + (match if t[i - 1] == q[j - 1] else mismatch) if hrow[j - 1] > NEG_LIMIT else NEG
            down, right = ecol[j], f  # (minus infinity where the cell above / to the left is out of its row's band)
            if diag >= down and diag >= right:
                h, mark = diag, 0
            elif right >= down:
                h, mark = right, -hrun
            else:
                h, mark = down, vrun[j]
            if h <= NEG_LIMIT:  # a cell no path reaches
                f, hrun = NEG, 1
                continue
            marks[(i, j)] = mark
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
        assert (rowmax > NEG_LIMIT) == has_cell
        if drops(best, i, rowmax, rj, zdrop, e):
            rows_done, dropped = i - 1, 1
            break
        hrow, ecol, vrun = nrow, necol, nvrun
        if rowmax > best[0]:
            best = (rowmax, i, rj)
        if i + lo <= ql <= i + hi and hrow[ql] > NEG_LIMIT and hrow[ql] >= qend[0]:
            qend = (hrow[ql], i)
    return _result(best, qend, rows_done, dropped, ql, to_query_end, lambda i, j: marks[(i, j)])


def extend_adaptive_align_np(t, q, match, mismatch, gopen, gext, band, zdrop, to_query_end=False, centres=None):
    """The same function one row at a time (numpy), as extend_textbook.extend_align_np does it: a row's in-band columns are a slice, F a
    running maximum where gopen >= gext.  hrow and ecol hold minus infinity outside the band of the row they belong to."""
    match, mismatch, o, e = normalize(match, mismatch, gopen, gext)
    tl, ql = len(t), len(q)
    assert tl >= 1 and ql >= 1 and band >= 0
    ta = np.frombuffer(bytes(t), np.uint8)
    qa = np.frombuffer(bytes(q), np.uint8)
    fin = lambda v: v > NEG_LIMIT  # noqa: E731
    marks = []
    cols = np.arange(ql + 1, dtype=np.int64)
    d = 0
    if centres is not None:
        centres.append(d)
    hrow = np.where(cols <= band, np.where(cols > 0, -o - (cols - 1) * e, 0), NEG)
    ecol = np.where(fin(hrow), hrow - o, NEG)
    vrun = np.ones(ql + 1, np.int64)
    best = (0, 0, 0)
    qend = (NO_QEND, -1)
    rows_done, dropped = tl, 0
    rj, has_cell = 0, True
    for i in range(1, tl + 1):
        if i > 1 and (i - 1) % R == 0:
            d = _next_centre(d, i - 1, rj, has_cell, band)
            if centres is not None:
                centres.append(d)
        lo, hi = d - band, d + band
        a, b = max(1, i + lo), min(ql, i + hi)
        n = b - a + 1
        has_cell = i + lo <= ql
        h0 = _gap(i, o, e) if i + lo <= 0 else NEG
        if n <= 0:  # no interior cell: the band has left the matrix, or holds the border column alone
            rowmax, rj = h0, 0
            assert fin(rowmax) == has_cell
            if drops(best, i, rowmax, rj, zdrop, e):
                rows_done, dropped = i - 1, 1
                break
            marks.append(None)
            hrow = np.full(ql + 1, NEG, np.int64)
            hrow[0] = h0
            ecol = np.full(ql + 1, NEG, np.int64)
            continue
        js = cols[a:b + 1]
        f0 = _minus(h0 if a == 1 else NEG, o)
        up = hrow[a - 1:b]
        diag = np.where(fin(up), up + np.where(qa[a - 1:b] == ta[i - 1], match, mismatch), NEG)
        down = ecol[a:b + 1].copy()
        vr = vrun[a:b + 1]
        hv = np.maximum(diag, down)
        if o >= e:
            k = js - a
            g = np.empty(n, np.int64)
            g[0] = f0
            g[1:] = np.where(fin(hv[:-1]), hv[:-1] - o + (k[:-1] + 1) * e, NEG)  # opened behind column a + k', seen from column a
            run = np.maximum.accumulate(g)
            F = np.where(fin(run), run - k * e, NEG)
            H = np.maximum(hv, F)
        else:
            F = np.empty(n, np.int64)
            H = np.empty(n, np.int64)
            fv = f0
            for x in range(n):
                F[x] = fv
                H[x] = max(int(hv[x]), fv)
                fv = max(_minus(int(H[x]), o), _minus(fv, e))
        Fe = np.where(fin(F), F - e, NEG)
        De = np.where(fin(down), down - e, NEG)
        Ho = np.where(fin(H), H - o, NEG)
        f_open = Ho > Fe
        e_open = Ho > De
        idx = np.arange(n)
        last_open = np.maximum.accumulate(np.where(np.concatenate(([True], f_open[:-1] | ~fin(H[:-1]))), idx, -1))
        hrun = idx - last_open + 1  # the horizontal run entering each cell
        is_diag = (diag >= down) & (diag >= F)
        is_right = ~is_diag & (F >= down)
        x = int(np.argmax(H))  # the first of the largest
        rowmax, rj = (int(H[x]), a + x) if int(H[x]) > h0 else (h0, 0)
        assert fin(rowmax) == has_cell
        if drops(best, i, rowmax, rj, zdrop, e):
            rows_done, dropped = i - 1, 1
            break
        marks.append((a, np.where(is_diag, 0, np.where(is_right, -hrun, vr)).astype(np.int32)))
        necol = np.full(ql + 1, NEG, np.int64)
        necol[a:b + 1] = np.where(e_open, Ho, De)
        nvrun = np.ones(ql + 1, np.int64)
        nvrun[a:b + 1] = np.where(e_open, 1, vr + 1)
        ecol, vrun = necol, nvrun
        hrow = np.full(ql + 1, NEG, np.int64)
        hrow[0] = h0
        hrow[a:b + 1] = H
        if rowmax > best[0]:
            best = (rowmax, i, rj)
        if b == ql and fin(int(H[-1])) and int(H[-1]) >= qend[0]:
            qend = (int(H[-1]), i)

    def at(i, j):
        a, m = marks[i - 1]
        return int(m[j - a])

    return _result(best, qend, rows_done, dropped, ql, to_query_end, at)


# ---- mirror of mgl_amd/csrc/sw_extend.h: one pair's workspace slot with the flag on -- section 9c's, and one int32 per strip of 64 rows
# (the strip's centre d_k, which the walk reads back) unless score-only
def extend_adaptive_pair_bytes(tl, ql, band, score_only=False):
    return extend_pair_bytes(tl, ql, band, score_only) + (0 if score_only else (4 * ((tl + 63) // 64) + 255) // 256 * 256)


def extend_adaptive_slot_bytes(max_tl, max_ql, band, score_only=False):
    """What the host sizes every slot with: monotone in tl and ql as section 9c's.  The band is clamped at max_tl + max_ql here, not at the
    larger length: a band that follows the path covers a pair's matrix wherever it stands only from tl + ql on."""
    return extend_adaptive_pair_bytes(max_tl, max_ql, min(band, max_tl + max_ql), score_only)
