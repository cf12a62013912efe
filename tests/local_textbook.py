"""The local (zero-floor) Smith-Waterman function of mgl_sw_local_batch_device_matrix, written from its definition
(include/mgl_sw.h) and nothing else: the checker the GPU kernels are compared against.

    E[i][j] = max(H[i-1][j] - o, E[i-1][j] - e)        vertical, consumes target, 'D'
    F[i][j] = max(H[i][j-1] - o, F[i][j-1] - e)        horizontal, consumes query, 'I'
    H[i][j] = max(0, H[i-1][j-1] + s, E[i][j], F[i][j])
    H[0][*] = H[*][0] = 0, E[0][*] = F[*][0] = -inf

score = max H over i, j >= 1 (0 if none); (t_end, q_end) = the smallest (i, j) with H == score, i first.  The walk starts there in
state H: H == 0 stops, then diagonal, then F, then E; in F / E extension wins ties.

local_align() is the plain form (one cell at a time); local_align_np() the same function vectorised by row (the F recurrence of a row
is a running maximum, numpy's maximum.accumulate over H - o + k e).  Both return (score, t_begin, t_end, q_begin, q_end, cigar) with
the CIGAR as text; the two agree on every field (tests/test_local_textbook.py).  local_scores_np() is the score alone for one target
against many queries at once (a tile), pinned against local_align() in the same file."""
import numpy as np

NEG = -(1 << 40)


def _score(code, matrix, tb, qb):
    return int(matrix[code[tb]][code[qb]])


def cigar_text(ops):
    """'MMID' -> '2M1I1D' (adjacent equal operations merged)."""
    out, k = [], 0
    while k < len(ops):
        m = k
        while m < len(ops) and ops[m] == ops[k]:
            m += 1
        out.append(f"{m - k}{ops[k]}")
        k = m
    return "".join(out)


def _walk(t, q, code, matrix, o, e, H, E, F, ti, qj):
    i, j, state, ops = ti, qj, "H", []
    while True:
        if state == "H":
            if i == 0 or j == 0 or H[i][j] == 0:
                break
            s = _score(code, matrix, t[i - 1], q[j - 1])
            if H[i][j] == H[i - 1][j - 1] + s:
                ops.append("M")
                i, j = i - 1, j - 1
            elif H[i][j] == F[i][j]:
                state = "F"
            else:
                state = "E"
        elif state == "F":
            ops.append("I")
            ext = F[i][j - 1] - e >= H[i][j - 1] - o
            j -= 1
            state = "F" if ext else "H"
        else:
            ops.append("D")
            ext = E[i - 1][j] - e >= H[i - 1][j] - o
            i -= 1
            state = "E" if ext else "H"
    return i, j, "".join(reversed(ops))


def _finish(t, q, code, matrix, o, e, H, E, F):
    tl, ql = len(t), len(q)
    best, bi, bj = 0, 0, 0
    for i in range(1, tl + 1):
        for j in range(1, ql + 1):
            if H[i][j] > best:
                best, bi, bj = int(H[i][j]), i, j
    if best == 0:
        return 0, 0, 0, 0, 0, ""
    i0, j0, ops = _walk(t, q, code, matrix, o, e, H, E, F, bi, bj)
    return best, i0, bi, j0, bj, cigar_text(ops)


def local_align(t, q, code, matrix, gap_open, gap_extend):
    """t, q: bytes; code: 256 ints -> 0..31; matrix: 32 x 32 (row = target code, column = query code).  The plain form."""
    o, e = abs(int(gap_open)), abs(int(gap_extend))
    tl, ql = len(t), len(q)
    H = [[0] * (ql + 1) for _ in range(tl + 1)]
    E = [[NEG] * (ql + 1) for _ in range(tl + 1)]
    F = [[NEG] * (ql + 1) for _ in range(tl + 1)]
    for i in range(1, tl + 1):
        for j in range(1, ql + 1):
            E[i][j] = max(H[i - 1][j] - o, E[i - 1][j] - e)
            F[i][j] = max(H[i][j - 1] - o, F[i][j - 1] - e)
            H[i][j] = max(0, H[i - 1][j - 1] + _score(code, matrix, t[i - 1], q[j - 1]), E[i][j], F[i][j])
    return _finish(t, q, code, matrix, o, e, H, E, F)


def local_matrices_np(t, q, code, matrix, gap_open, gap_extend):
    """H, E, F as int64 arrays [tl + 1, ql + 1], row by row."""
    o, e = abs(int(gap_open)), abs(int(gap_extend))
    code = np.asarray(code, dtype=np.int64)
    matrix = np.asarray(matrix, dtype=np.int64)
    tl, ql = len(t), len(q)
    tc = code[np.frombuffer(bytes(t), np.uint8)] if tl else np.zeros(0, np.int64)
    qc = code[np.frombuffer(bytes(q), np.uint8)] if ql else np.zeros(0, np.int64)
    H = np.zeros((tl + 1, ql + 1), np.int64)
    E = np.full((tl + 1, ql + 1), NEG, np.int64)
    F = np.full((tl + 1, ql + 1), NEG, np.int64)
    k = np.arange(ql + 1, dtype=np.int64)
    for i in range(1, tl + 1):
        E[i, 1:] = np.maximum(H[i - 1, 1:] - o, E[i - 1, 1:] - e)
        hv = np.maximum(0, np.maximum(H[i - 1, :-1] + matrix[tc[i - 1], qc], E[i, 1:]))
        if o < e:  # an F-made H can open a better gap than its own source: cell by cell
            for j in range(1, ql + 1):
                F[i, j] = max(H[i, j - 1] - o, F[i, j - 1] - e)
                H[i, j] = max(hv[j - 1], F[i, j])
            continue
        # F[i][j] = max over j' < j of (H[i][j'] - o - (j - 1 - j') e).  With o >= e an H that F made is never the best source (its
        # own source gives at least as much), so the running maximum over hv (H without F) gives F exactly
        g = np.empty(ql + 1, np.int64)
        g[0] = -o  # H[i][0] = 0
        g[1:] = hv - o + k[1:] * e
        run = np.maximum.accumulate(g)
        F[i, 1:] = run[:-1] - k[:-1] * e
        H[i, 1:] = np.maximum(hv, F[i, 1:])
    return H, E, F


def local_align_np(t, q, code, matrix, gap_open, gap_extend):
    """The same function, vectorised by row (for pairs of hundreds of residues)."""
    o, e = abs(int(gap_open)), abs(int(gap_extend))
    H, E, F = local_matrices_np(t, q, code, matrix, gap_open, gap_extend)
    if H.size == 0 or H[1:, 1:].size == 0:
        return 0, 0, 0, 0, 0, ""
    best = int(H[1:, 1:].max())
    if best <= 0:
        return 0, 0, 0, 0, 0, ""
    flat = int(np.argmax(H[1:, 1:] == best))  # row-major: smallest i, then smallest j
    bi, bj = divmod(flat, H.shape[1] - 1)
    bi, bj = bi + 1, bj + 1
    i0, j0, ops = _walk(t, q, code, matrix, o, e, H, E, F, bi, bj)
    return best, i0, bi, j0, bj, cigar_text(ops)


def local_scores_np(t, qs, code, matrix, gap_open, gap_extend):
    """The scores of one target against many queries (a tile): int64[len(qs)].  The same recurrence as local_matrices_np, one target row
    at a time over ALL queries at once ([len(qs), longest query]), keeping only the previous row.  A query shorter than the longest is
    padded with a column code of its own whose score lies below any real one, and the maximum is taken over a query's own columns only
    (a cell depends on cells above and left of it, so what padding holds never reaches a real cell).  o < e goes pair by pair through
    local_align_np (an F-made H can open a better gap than its source: no running maximum)."""
    o, e = abs(int(gap_open)), abs(int(gap_extend))
    n = len(qs)
    out = np.zeros(n, np.int64)
    if o < e:
        for k, q in enumerate(qs):
            out[k] = local_align_np(t, q, code, matrix, o, e)[0]
        return out
    code = np.asarray(code, dtype=np.int64)
    tl, L = len(t), max((len(q) for q in qs), default=0)
    if n == 0 or tl == 0 or L == 0:
        return out
    m = np.full((32, 33), -(1 << 20), np.int64)  # column 32: the padding
    m[:, :32] = np.asarray(matrix, dtype=np.int64)
    tc = code[np.frombuffer(bytes(t), np.uint8)]
    qc = np.full((n, L), 32, np.int64)
    real = np.zeros((n, L), bool)
    for k, q in enumerate(qs):
        qc[k, : len(q)] = code[np.frombuffer(bytes(q), np.uint8)]
        real[k, : len(q)] = True
    col = np.arange(L + 1, dtype=np.int64) * e
    H = np.zeros((n, L + 1), np.int64)
    E = np.full((n, L), NEG, np.int64)
    g = np.empty((n, L + 1), np.int64)
    g[:, 0] = -o
    for i in range(tl):
        E = np.maximum(H[:, 1:] - o, E - e)
        hv = np.maximum(0, np.maximum(H[:, :-1] + m[tc[i]][qc], E))
        g[:, 1:] = hv - o + col[1:]
        F = np.maximum.accumulate(g, axis=1)[:, :-1] - col[:-1]
        H[:, 1:] = np.maximum(hv, F)
        out = np.maximum(out, np.where(real, H[:, 1:], 0).max(axis=1))
    return out


def replay(t, q, code, matrix, gap_open, gap_extend, t_begin, q_begin, cigar):
    """The score of a CIGAR over t[t_begin:], q[q_begin:] and the (t_end, q_end) it reaches."""
    o, e = abs(int(gap_open)), abs(int(gap_extend))
    i, j, total = t_begin, q_begin, 0
    num = ""
    for ch in cigar:
        if ch.isdigit():
            num += ch
            continue
        n, num = int(num), ""
        if ch == "M":
            for _ in range(n):
                total += _score(code, matrix, t[i], q[j])
                i, j = i + 1, j + 1
        elif ch == "I":
            total -= o + (n - 1) * e
            j += n
        elif ch == "D":
            total -= o + (n - 1) * e
            i += n
        else:
            raise ValueError(cigar)
    return total, i, j


def cigar_binary_to_text(words):
    """BAM-style uint32 elements (len << 4 | op, M=0 I=1 D=2) -> text."""
    return "".join(f"{int(w) >> 4}{'MID'[int(w) & 15]}" for w in words)


def top_k(scores, k):
    """scores: [Q, D] -> indices [Q, k]: score descending, then database index ascending."""
    scores = np.asarray(scores)
    order = np.lexsort((np.broadcast_to(np.arange(scores.shape[1]), scores.shape), -scores.astype(np.int64)), axis=-1)
    return order[:, :k]


def dna_matrix(match=2, mismatch=-3, n_score=None):
    """A +/- matrix over ACGTN for the textbook (same layout as mgl_amd.protein.dna_matrix)."""
    code = np.full(256, 4, np.uint8)
    for k, ch in enumerate("ACGT"):
        code[ord(ch)] = k
        code[ord(ch.lower())] = k
    m = np.full((32, 32), mismatch, np.int8)
    for k in range(4):
        m[k, k] = match
    m[4, :] = m[:, 4] = mismatch if n_score is None else n_score
    return code, m


# ---- mirror of mgl_amd/csrc/sw_local.h: local_lane_ok() (kernel A's range guard), pinned by tests/test_local_textbook.py
LOCAL_LANE_LDS_LIMIT = 64 * 1024
LOCAL_LANE_R = 32


def local_lane_bias(smin):
    return max(0, -int(smin))


def local_lane_lds_bytes(max_tl):
    strips = (max_tl + LOCAL_LANE_R - 1) // LOCAL_LANE_R
    return 256 + 32 * 32 + 33 * LOCAL_LANE_R + (strips * LOCAL_LANE_R + 15) // 16 * 16


def local_lane_ok(smin, smax, gopen, gext, max_tl, max_ql):
    """Kernel A (packed unsigned 16-bit, zero floor) may run a batch of these bounds: a profile byte S + K (K = max(0, -smin)) for every
    entry, H + S + K within 16 bits, gap constants within 16 bits, the target's codes within the LDS carve."""
    if max_tl < 1 or max_ql < 1 or gext < 0 or gopen < 0:
        return False
    k = local_lane_bias(smin)
    if smax + k > 255:
        return False
    if max(int(smax), 0) * min(max_tl, max_ql) + 255 > 65535:
        return False
    if gopen > 65535 or gext > 65535:
        return False
    return local_lane_lds_bytes(max_tl) <= LOCAL_LANE_LDS_LIMIT
