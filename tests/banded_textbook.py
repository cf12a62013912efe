"""The banded function of mgl_sw_align_batch_device_banded, written from its definition (include/mgl_sw.h) and
nothing else: the checker the GPU kernel is compared against.

For a pair of lengths tl, ql and a band >= 0:  lo = min(0, ql - tl) - band,  hi = max(0, ql - tl) + band;  a cell (i, j), border row
and column included, is in the band iff lo <= j - i <= hi.  The recurrence, priorities, tie rules, run lengths, end-cell scans and
the walk are those of oracle/sw_oracle.c (fill_core, swo_cigar) with three additions:

 1. only in-band interior cells are computed; a value read from an out-of-band cell (H, E from above, F from the left) is minus
    infinity: it loses every comparison strictly and stays minus infinity under - gext;
 2. the last-column and last-row scans visit in-band cells only, in the oracle's order with its tie rules;
 3. the walk starts where the oracle's starts and reads in-band decisions only.

banded_align() is the plain form (one cell at a time, minus infinity is None-like NEG kept exact); banded_align_np() the same function
vectorised by row for long pairs (the two agree on every output: tests/test_banded_textbook.py).  Both return
(offset, (mqe, mqe_t, max, max_t, max_q, seg_length), cigar text).  path_band() is the smallest band that holds a golden record's path.
The last part mirrors mgl_amd/csrc/sw_banded.h: the kernel's range guard and its workspace slot."""
import re

import numpy as np

SOFTCLIP, INDEL, LEADING_INDEL, IGNORE = 1, 2, 4, 8
NEG = -(1 << 60)      # minus infinity: anything at or below NEG_LIMIT is it
NEG_LIMIT = -(1 << 59)
SWO_NEG_INF = -0x40000000


def normalize(match, mismatch, gopen, gext):
    return abs(match), -abs(mismatch), abs(gopen), abs(gext)


def band_limits(tl, ql, band):
    return min(0, ql - tl) - band, max(0, ql - tl) + band


def _minus(v, k):
    """v - k with minus infinity staying what it is."""
    return NEG if v <= NEG_LIMIT else v - k


def _border(k, o, e, indel):
    return -o - (k - 1) * e if (indel and k > 0) else 0


def banded_fill(t, q, match, mismatch, gopen, gext, strategy, band):
    """-> (btr, ez): btr maps every in-band interior cell (i, j) to the oracle's mark (+k rows up, -k columns left, 0 diagonal)."""
    match, mismatch, o, e = normalize(match, mismatch, gopen, gext)
    tl, ql = len(t), len(q)
    assert tl >= 1 and ql >= 1 and band >= 0
    lo, hi = band_limits(tl, ql, band)
    indel = strategy in (INDEL, LEADING_INDEL)
    inb = lambda i, j: lo <= j - i <= hi  # noqa: E731
    hrow = [_border(j, o, e, indel) if inb(0, j) else NEG for j in range(ql + 1)]
    ecol = [_minus(hrow[j], o) for j in range(ql + 1)]
    vrun = [1] * (ql + 1)
    btr = {}
    mqe, mqe_t = SWO_NEG_INF, -1
    for i in range(1, tl + 1):
        nrow = [NEG] * (ql + 1)
        nrow[0] = _border(i, o, e, indel) if inb(i, 0) else NEG
        f, hrun = _minus(nrow[0], o), 1
        for j in range(max(1, i + lo), min(ql, i + hi) + 1):
            hdiag = hrow[j - 1]
            assert hdiag > NEG_LIMIT  # the diagonal predecessor of an in-band cell is in the band
            diag = hdiag + (match if t[i - 1] == q[j - 1] else mismatch)
            down = ecol[j] if inb(i - 1, j) else NEG
            right = f if inb(i, j - 1) else NEG
            if diag >= down and diag >= right:
                h, mark = diag, 0
            elif right >= down:
                h, mark = right, -hrun
            else:
                h, mark = down, vrun[j]
            btr[(i, j)] = mark
            if h - o > _minus(down, e):
                ecol[j], vrun[j] = h - o, 1
            else:
                ecol[j], vrun[j] = down - e, vrun[j] + 1
            if h - o > _minus(right, e):
                f, hrun = h - o, 1
            else:
                f, hrun = right - e, hrun + 1
            nrow[j] = h
        hrow = nrow
        if inb(i, ql) and hrow[ql] >= mqe:
            mqe, mqe_t = hrow[ql], i
    mx, max_t, max_q, seg = mqe, mqe_t, ql, 0
    for j in range(1, ql + 1):
        if not inb(tl, j):
            continue
        sc = hrow[j]
        if sc > mx or (sc == mx and abs(tl - j) < abs(max_t - max_q)):
            mx, max_t, max_q, seg = sc, tl, j, ql - j
    return btr, (mqe, mqe_t, mx, max_t, max_q, seg)


def walk(btr_at, tl, ql, strategy, ez):
    """swo_cigar over btr_at(i, j) -> (offset, cigar text)."""
    mqe, mqe_t, mx, max_t, max_q, seg_length = ez
    seg = 0
    if strategy == INDEL:
        I, J = tl, ql
    elif strategy != LEADING_INDEL:
        I, J, seg = max_t, max_q, seg_length
    else:
        I, J = mqe_t, ql
    assert 1 <= I <= tl and 1 <= J <= ql
    el = []  # last element first
    if seg > 0 and strategy == SOFTCLIP:
        el.append(("S", seg))
        seg = 0
    state = "M"
    while True:
        b = btr_at(I, J)
        step = 1
        if b > 0:
            nxt, step = "D", b
            I -= step
        elif b < 0:
            nxt, step = "I", -b
            J -= step
        else:
            nxt = "M"
            I, J = I - 1, J - 1
        if nxt == state:
            seg += step
        else:
            el.append((state, seg))
            seg, state = step, nxt
        if not (I > 0 and J > 0):
            break
    if strategy == SOFTCLIP:
        el.append((state, seg))
        if J > 0:
            el.append(("S", J))
        off = I
    elif strategy == IGNORE:
        el.append((state, seg + J))
        off = I - J
    else:
        el.append((state, seg))
        if I > 0:
            el.append(("D", I))
        elif J > 0:
            el.append(("I", J))
        off = 0
    return off, "".join(f"{n}{op}" for op, n in reversed(el) if n > 0)


def banded_align(t, q, match, mismatch, gopen, gext, strategy, band):
    """The plain form."""
    btr, ez = banded_fill(t, q, match, mismatch, gopen, gext, strategy, band)
    off, cigar = walk(lambda i, j: btr[(i, j)], len(t), len(q), strategy, ez)
    return off, ez, cigar


def banded_align_np(t, q, match, mismatch, gopen, gext, strategy, band):
    """The same function one row at a time (numpy), for long pairs.  Row i's in-band columns are a slice; with gopen >= gext the F of a
    row is a running maximum (an H that F made never opens a better gap than extending the one it came from), otherwise the row is
    done cell by cell.  Marks are kept band-relative: mark[i][j - (i + lo)]."""
    match, mismatch, o, e = normalize(match, mismatch, gopen, gext)
    tl, ql = len(t), len(q)
    assert tl >= 1 and ql >= 1 and band >= 0
    lo, hi = band_limits(tl, ql, min(band, max(tl, ql)))
    indel = strategy in (INDEL, LEADING_INDEL)
    W = hi - lo + 1
    ta = np.frombuffer(bytes(t), np.uint8)
    qa = np.frombuffer(bytes(q), np.uint8)
    marks = np.zeros((tl + 1, W), np.int32)
    cols = np.arange(ql + 1, dtype=np.int64)
    bord = np.where(cols > 0, -o - (cols - 1) * e, 0) if indel else np.zeros(ql + 1, np.int64)
    hrow = np.where(cols <= hi, bord, NEG)
    ecol = np.where(hrow > NEG_LIMIT, hrow - o, NEG)
    vrun = np.ones(ql + 1, np.int64)
    mqe, mqe_t = SWO_NEG_INF, -1
    for i in range(1, tl + 1):
        a, b = max(1, i + lo), min(ql, i + hi)
        n = b - a + 1
        js = cols[a:b + 1]
        h0 = int(_border(i, o, e, indel)) if -i >= lo else NEG  # H[i][0]
        hleft = h0 if a == 1 else NEG                           # H[i][a - 1] as the band sees it
        f0 = _minus(hleft, o)
        diag = hrow[a - 1:b] + np.where(qa[a - 1:b] == ta[i - 1], match, mismatch)
        down = ecol[a:b + 1].copy()
        if b == i + hi:
            down[-1] = NEG  # (i - 1, b) is above the band
        vr = vrun[a:b + 1]
        hv = np.maximum(diag, down)
        F = np.empty(n, np.int64)
        H = np.empty(n, np.int64)
        if o >= e:
            k = js - a
            g = np.empty(n, np.int64)
            g[0] = f0 if f0 > NEG_LIMIT else NEG
            g[1:] = hv[:-1] - o + (k[:-1] + 1) * e  # opened behind column a + k', seen from column a
            run = np.maximum.accumulate(g)
            F = np.where(run > NEG_LIMIT, run - k * e, NEG)
            H = np.maximum(hv, F)
        else:
            fv = f0
            for x in range(n):
                F[x] = fv
                H[x] = max(int(hv[x]), fv)
                fv = max(int(H[x]) - o, _minus(fv, e))
        Fe = np.where(F > NEG_LIMIT, F - e, NEG)
        De = np.where(down > NEG_LIMIT, down - e, NEG)
        f_open = H - o > Fe
        e_open = H - o > De
        # the horizontal run length entering each cell: 1 behind an open (or at the band's first column), else one more
        idx = np.arange(n)
        last_open = np.maximum.accumulate(np.where(np.concatenate(([True], f_open[:-1])), idx, -1))
        hrun = idx - last_open + 1
        is_diag = (diag >= down) & (diag >= F)
        is_right = ~is_diag & (F >= down)
        marks[i, a - (i + lo):a - (i + lo) + n] = np.where(is_diag, 0, np.where(is_right, -hrun, vr))
        ecol[a:b + 1] = np.where(e_open, H - o, De)
        vrun[a:b + 1] = np.where(e_open, 1, vr + 1)
        nrow = np.full(ql + 1, NEG, np.int64)
        nrow[0] = h0
        nrow[a:b + 1] = H
        hrow = nrow
        if b == ql and int(H[-1]) >= mqe:
            mqe, mqe_t = int(H[-1]), i
    mx, max_t, max_q, seg = mqe, mqe_t, ql, 0
    for j in range(max(1, tl + lo), ql + 1):
        sc = int(hrow[j])
        if sc > mx or (sc == mx and abs(tl - j) < abs(max_t - max_q)):
            mx, max_t, max_q, seg = sc, tl, j, ql - j
    ez = (mqe, mqe_t, mx, max_t, max_q, seg)

    def at(i, j):
        assert lo <= j - i <= hi
        return int(marks[i, j - (i + lo)])

    off, cigar = walk(at, tl, ql, strategy, ez)
    return off, ez, cigar


_EL = re.compile(r"(\d+)([MIDS])")


def path_cells(tl, ql, strategy, offset, cigar):
    """(first, moves): the border cell a record's walk stops in and its moves in path order (an 'M' covers one diagonal step, an
    'I' / 'D' element one gap run), overhang elements that the strategies add after the walk taken off."""
    els = [(op, int(n)) for n, op in _EL.findall(cigar)]
    assert "".join(f"{n}{op}" for op, n in els) == cigar
    if strategy == SOFTCLIP:
        i0, j0 = offset, 0
        if els and els[0][0] == "S":
            j0 = els[0][1]
            els = els[1:]
        if els and els[-1][0] == "S":
            els = els[:-1]
        return (i0, j0), els
    if strategy == IGNORE:
        return None, None  # the overhang is folded into the first and last element: the path cannot be read back
    # INDEL, LEADING_INDEL: offset 0; a leading D / I may be the overhang the strategy adds (the walk stopped on a border) or a run of
    # the path that reached the border itself -- the same cells either way
    return (0, 0), els


def path_band(g):
    """The smallest band that holds every cell of a golden record's path, or None where the record does not determine the path
    (IGNORE).  Cells: from the walk's start cell to the border cell it stops in, gap runs included."""
    tl, ql = len(g.t), len(g.q)
    first, els = path_cells(tl, ql, g.strategy, g.offset, g.cigar)
    if first is None:
        return None
    i, j = first
    dmin = dmax = j - i
    for op, n in els:
        if op == "M":
            i, j = i + n, j + n
        elif op == "I":
            j += n
        elif op == "D":
            i += n
        else:
            raise ValueError(g.cigar)
        dmin, dmax = min(dmin, j - i), max(dmax, j - i)
    # lo = min(0, ql - tl) - band <= dmin and hi = max(0, ql - tl) + band >= dmax
    return max(0, min(0, ql - tl) - dmin, dmax - max(0, ql - tl))


def cigar_binary_to_text(words):
    """BAM-style uint32 elements (len << 4 | op, M=0 I=1 D=2 S=4) -> text."""
    return "".join(f"{int(w) >> 4}{'MIDNS'[int(w) & 15]}" for w in words)


# ---- mirror of mgl_amd/csrc/sw_banded.h: the kernel's range guard and one pair's workspace slot, pinned by tests/test_banded_textbook.py
BANDED_MAX_LEN = 1 << 28
BANDED_MAX_SCORE = 1 << 29


def banded_range_ok(tl, ql, match, mismatch, gopen, gext):
    """On the normalised parameters: every finite H, E, F of the pair stays within +-2^29."""
    if tl < 1 or ql < 1 or tl > BANDED_MAX_LEN or ql > BANDED_MAX_LEN:
        return False
    if match < 0 or mismatch > 0 or gopen < 0 or gext < 0 or gopen > (1 << 24) or gext > (1 << 24):
        return False
    return max(match, -mismatch) * min(tl, ql) + 2 * gopen + gext * max(tl, ql) <= BANDED_MAX_SCORE


def banded_strip_steps(tl, ql, band):
    lo, hi = band_limits(tl, ql, band)
    return (min(ql, hi - lo + 64) + 63 + 7) & ~7


def banded_pair_bytes(tl, ql, band, score_only=False):
    r = lambda x: (x + 255) // 256 * 256  # noqa: E731
    carry, elems = r((ql + 1) * 8), r((tl + ql + 4) * 4)
    return carry + (0 if score_only else elems + (tl + 63) // 64 * banded_strip_steps(tl, ql, band) * 32)


def banded_slot_bound(max_tl, max_ql, band, score_only=False):
    """Mirror of sw_banded.h banded_slot_bound(): what the host sizes a slot with -- at least the banded_pair_bytes of every pair within
    (max_tl, max_ql).  Per number of strips: above tl the steps grow with ql (max_ql, fewest rows); below tl they peak where ql meets
    tl - ql + 2 band + 64 (most rows)."""
    r = lambda x: (x + 255) // 256 * 256  # noqa: E731
    fixed = r((max_ql + 1) * 8) + (0 if score_only else r((max_tl + max_ql + 4) * 4))
    if score_only:
        return fixed
    strips = (max_tl + 63) // 64
    if strips > (1 << 16):
        return fixed + strips * ((max_ql + 63 + 7) & ~7) * 32
    best = 0
    for k in range(1, strips + 1):
        t_min, t_max = 64 * (k - 1) + 1, min(64 * k, max_tl)
        peak = (t_max + 2 * band + 64 + 1) // 2
        for q in (max_ql, min(peak, max_ql), min(peak + 1, max_ql), min(t_max, max_ql)):
            q = max(q, 1)
            best = max(best, k * max(banded_strip_steps(t_min, q, band), banded_strip_steps(t_max, q, band)))
    return fixed + best * 32
