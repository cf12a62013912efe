"""Python mirrors of the host-side 16-bit range guards of the DNA kernels, edge finders built on them, a plain int64 reference of the
recurrence with full H, E and F, and the strip kernel's window measured on it.  A helper module for tests/test_range_guards.py (CPU)
and tests/test_gpu_range_edges.py (GPU); the CPU tests pin every mirror to the planner, so the GPU edge tests move with the guards.

Parameters are normalised (match > 0, mismatch <= match, gopen >= gext >= 0), as the library passes them to the guards.
    dp16_range_ok      sw_dp16.hip      sw_dp16_kernel, sw_dp16_lane_kernel, sw_dp16_lane_ck_kernel (+ fold twins), grouped batches
    strip16_range_ok   sw_dp16_strip.hip  sw_dp16_strip_kernel in all its forms, and the strip walk (a static bound, no fall-back)
    small_fits_int16   sw_small.hip     narrow or wide sw_small_kernel / one-pair service
    coop16_possible / coop16_worthwhile   sw_dp_coop.hip   sw_dp_coop16_kernel (checks its own window, falls back to int32)
"""
import numpy as np

STRIP_LEVEL = -14000  # sw_dp16_strip.hip: where a move of the baseline puts a strip's first row
STRIP_MOVE_COLS = 16  # ... moved every 16 columns (column groups cg with cg % (16 / STRIP_CPS) == 0)
SOFTCLIP, INDEL, LEAD_INDEL, IGNORE = 1, 2, 4, 8


def dp16_range_ok(tl, ql, match, mismatch, gopen, gext):
    if match <= 0 or gopen < gext:
        return False
    top = match * min(tl, ql) + gext * (tl + ql)
    low = -3 * gopen - (match - mismatch) - 2 * gext - 64
    return 32767 - top + low >= -32768 and match - mismatch <= 30000 and gopen <= 10000 and gext <= 5000 and match + 2 * gext <= 30000


def dp16_slack(tl, ql, match, mismatch, gopen, gext):
    """How far the guard's inequality is from failing (0: tight; negative: refused)."""
    top = match * min(tl, ql) + gext * (tl + ql)
    low = -3 * gopen - (match - mismatch) - 2 * gext - 64
    return 32767 - top + low + 32768


def strip16_window(match, mismatch, gopen, gext):
    """(above, below): how far over / under STRIP_LEVEL the guard lets a strip's values go."""
    up, down, mis2 = match + gopen + gext, gopen - gext, mismatch + 2 * gext
    above = 31 * up + 20 * up + gopen + (match + 2 * gext) + 64
    below = 31 * down + 20 * up + up + down + abs(mis2) + 64
    return above, below


def strip16_range_ok(match, mismatch, gopen, gext):
    if match <= 0 or mismatch > match or gext < 0 or gopen < gext or match > 4000 or mismatch < -4000 or gopen > 4000 or gext > 4000:
        return False
    above, below = strip16_window(match, mismatch, gopen, gext)
    return STRIP_LEVEL + above <= 32767 and STRIP_LEVEL - below >= -32768


def small_span(tl, ql, match, mismatch, gopen, gext):
    hi = match * min(tl, ql) + (tl + ql) * gext
    lo = -2 * gopen - (tl + ql) * gext
    return hi - lo


def small_fits_int16(tl, ql, match, mismatch, gopen, gext):
    if match < 0 or mismatch > match or gopen < 0 or gext < 0:
        return False
    return small_span(tl, ql, match, mismatch, gopen, gext) <= 65000


def coop16_below(match, mismatch, gopen, gext):
    mis2 = mismatch + 2 * gext
    return 34 * (gopen - gext) + 2 * (match + gopen + gext) + (gopen - gext) + abs(mis2) + 64


def coop16_above(match, gopen, gext):
    return 34 * (match + gopen + gext) + gopen + (match + 2 * gext) + 64


def coop16_possible(match, mismatch, gopen, gext):
    if match <= 0 or mismatch > match or gext < 0 or gopen < gext or match > 4000 or mismatch < -4000 or gopen > 4000 or gext > 4000:
        return False
    return coop16_below(match, mismatch, gopen, gext) + coop16_above(match, gopen, gext) <= 60000


def coop16_worthwhile(match, mismatch, gopen, gext):
    if not coop16_possible(match, mismatch, gopen, gext):
        return False
    margin = coop16_below(match, mismatch, gopen, gext) + coop16_above(match, gopen, gext)
    return 128 * (match + 2 * gext) + 2 * (gopen - gext) + margin <= 64000


# ---- edge finders

def last_true(ok, lo, hi):
    """The largest v in [lo, hi] with ok(v), for ok true up to some point and false after it (lo - 1 when ok(lo) fails)."""
    if not ok(lo):
        return lo - 1
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if ok(mid):
            lo = mid
        else:
            hi = mid - 1
    return lo


def dp16_largest_ql(tl, params, cap=1 << 16):
    """The largest query length dp16_range_ok admits with a target of tl rows (0: none)."""
    return max(0, last_true(lambda ql: dp16_range_ok(tl, ql, *params), 1, cap))


def param_edge(ok, params, index, step, limit):
    """Walk parameter `index` from params in steps of `step` (+1 / -1) while ok(*params) holds, up to `limit`: the last admitted
    set, i.e. the value at which the guard's inequality is tight (None when params itself is refused)."""
    def at(v):
        p = list(params)
        p[index] = v
        return tuple(p)

    if not ok(*params):
        return None
    n = last_true(lambda k: ok(*at(params[index] + step * k)), 0, abs(limit - params[index]))
    return at(params[index] + step * n)


def past(params, index, step):
    p = list(params)
    p[index] += step
    return tuple(p)


# ---- a plain reference of the recurrence (the reference's sw.cpp:5-146; oracle/sw_oracle.c restates it cell by cell)

def border(k, gopen, gext, indel):
    return np.where((k > 0) & indel, -gopen - (k - 1) * gext, 0) if isinstance(k, np.ndarray) else (-gopen - (k - 1) * gext if indel and k > 0 else 0)


def dp_full(t: bytes, q: bytes, params, strategy):
    """int64 H[0..tl][0..ql], E[..], F[..], vectorised by anti-diagonal.  E[i][j] is the vertical gap value entering cell (i, j) from
    above (E[1][j] = H[0][j] - o), F[i][j] the horizontal one from the left (F[i][1] = H[i][0] - o); H = max(diag, E, F).  Row and
    column 0 of E and F do not exist: they hold H there, which every measurement below covers anyway."""
    m, x, o, e = (int(v) for v in params)
    tl, ql = len(t), len(q)
    indel = (strategy & (INDEL | LEAD_INDEL)) != 0
    ta = np.frombuffer(t, np.uint8).astype(np.int64)
    qa = np.frombuffer(q, np.uint8).astype(np.int64)
    H = np.zeros((tl + 1, ql + 1), np.int64)
    E = np.zeros_like(H)
    F = np.zeros_like(H)
    H[0, :] = border(np.arange(ql + 1), o, e, indel)
    H[:, 0] = border(np.arange(tl + 1), o, e, indel)
    E[0, :], E[:, 0] = H[0, :], H[:, 0]
    F[0, :], F[:, 0] = H[0, :], H[:, 0]
    for d in range(2, tl + ql + 1):
        i = np.arange(max(1, d - ql), min(tl, d - 1) + 1)
        j = d - i
        diag = H[i - 1, j - 1] + np.where(ta[i - 1] == qa[j - 1], m, x)
        up = np.where(i == 1, H[0, j] - o, np.maximum(H[i - 1, j] - o, E[i - 1, j] - e))
        left = np.where(j == 1, H[i, 0] - o, np.maximum(H[i, j - 1] - o, F[i, j - 1] - e))
        E[i, j] = up
        F[i, j] = left
        H[i, j] = np.maximum(diag, np.maximum(up, left))
    return H, E, F


def score_max(H):
    """ScoreMax (mqe, mqe_t, max, max_t, max_q, seg_length) from H, with the reference's tie rules (sw.cpp:100-127)."""
    tl, ql = H.shape[0] - 1, H.shape[1] - 1
    col = H[1:, ql]
    mqe_t = int(tl - np.argmax(col[::-1]))  # later row wins ties
    mqe = int(H[mqe_t, ql])
    best, bt, bq, seg = mqe, mqe_t, ql, 0
    for j in range(1, ql + 1):
        sc = int(H[tl, j])
        if sc > best or (sc == best and abs(tl - j) < abs(bt - bq)):
            best, bt, bq, seg = sc, tl, j, ql - j
    return (mqe, mqe_t, best, bt, bq, seg)


# ---- the strip kernel's window (sw_dp16_strip.hip:14-21, 232-260)

def strip_spread(H, E, F, gext, rows):
    """How far a strip's values rise above / fall below STRIP_LEVEL in the kernel's representation.

    Strip g holds target rows i0 + 1 .. i0 + rows (i0 = g * rows) and takes H and E of row i0 from the strip above.  Its baseline
    moves before column group cg whenever cg % 4 == 0: the column then in its registers is c0 = 16 k, and the move puts
    H[i0 + 1][c0] + (i0 + 1 + c0) e at STRIP_LEVEL.  Columns c0 + 1 .. c0 + 16 are then computed under that baseline, and the F
    it hands to column c0 + 17.  Every value X is held as X + (i + j) e - B.  Over rows i0 .. i0 + rows + 1 (the row above, the
    strip, the E it hands down) and columns c0 .. c0 + 17 of H, E and F, returns (above, below): the largest rise and fall."""
    tl, ql = H.shape[0] - 1, H.shape[1] - 1
    ij = np.add.outer(np.arange(tl + 1), np.arange(ql + 1)) * gext
    hi = np.maximum(np.maximum(H, E), F) + ij
    lo = np.minimum(np.minimum(H, E), F) + ij
    href = H + ij
    above = below = -(1 << 62)
    for i0 in range(0, tl, rows):
        r1 = min(i0 + rows + 1, tl)
        cmax = hi[i0:r1 + 1].max(axis=0)
        cmin = lo[i0:r1 + 1].min(axis=0)
        for c0 in range(0, ql, STRIP_MOVE_COLS):
            c1 = min(c0 + STRIP_MOVE_COLS + 1, ql)
            ref = href[i0 + 1, c0]
            above = max(above, int(cmax[c0:c1 + 1].max()) - ref)
            below = max(below, ref - int(cmin[c0:c1 + 1].min()))
    return above, below


def strip_fraction(H, E, F, params, rows):
    """(fraction of `above` reached, fraction of `below` reached, above, below) for strips of `rows` rows."""
    a, b = strip_spread(H, E, F, params[3], rows)
    wa, wb = strip16_window(*params)
    return a / wa, b / wb, a, b


def strip_candidates(seed=11, n=2400):
    """The pool the strip inputs are picked from: name -> (target, query), all ACGT."""
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(b"ACGT", np.uint8)
    g = alpha[rng.integers(0, 4, n + 200)].tobytes()
    h = alpha[rng.integers(0, 4, n)].tobytes()
    ins = alpha[rng.integers(0, 4, 40)].tobytes()
    blocks = b"".join((b"C" * 48 + b"A" * 80) for _ in range(n // 128 + 1))[:n]
    return {
        "identical": (g[:n], g[:n]),
        "insertion40": (g[:n // 2] + ins + g[n // 2:n - 40], g[:n]),
        "deletion40": (g[:n], g[:n // 2] + g[n // 2 + 40:n + 40]),
        "mismatch_blocks": (b"A" * n, blocks),
        "homopolymer": (b"A" * n, b"A" * (n - 7)),
        "homopolymer_short_query": (b"A" * n, b"A" * (n // 3)),
        "disjoint": (b"A" * n, b"C" * n),
        "unrelated": (g[:n], h),
    }


def pick_strip_inputs(params, strategy, rows, pool=None):
    """The candidates that reach the largest fraction of each side of the window: ((name, fa), (name, fb))."""
    pool = pool or strip_candidates()
    best_a = best_b = (None, -1.0)
    for name, (t, q) in pool.items():
        H, E, F = dp_full(t, q, params, strategy)
        fa, fb, _, _ = strip_fraction(H, E, F, params, rows)
        if fa > best_a[1]:
            best_a = (name, fa)
        if fb > best_b[1]:
            best_b = (name, fb)
    return best_a, best_b
