"""Inputs that put the one-wave pair kernel (small_pair() of sw_small_pair.h: the body of sw_small_kernel and of the mailbox waves of
sw_service_kernel) on its own seams, and the kernel's geometry and walk restated in plain Python.

One wave takes one pair: lane L owns target rows R L + 1 .. R L + R (R = 2, 4, 6 or 8 by tl), the fill moves along the query in
blocks of four steps that run masked (the ramps), unmasked (every lane inside the matrix) or clamped (finished lanes store into a
spare column), the kept scores are 16-bit (narrow) or 32-bit (wide) by the bounds of the BATCH, and the walk reads every move off the
kept H: diagonal runs of up to 64 cells a round, gap candidates 64 a round, ties by rule.  The restatement here names those numbers
(rows_per_lane, lanes, column_words, lds_bytes, supported, fill_schedule), walk() restates the walk on a numpy H matrix with every tie
rule switchable, and the builders make small batches whose paths, lengths, ties and bytes lie on the seams:

    rows, ramps, runs, round_ties, last_cell_ties, bytes, span, fits, slots

A Case is one batch: (name, targets, queries, params, strategies, cigar_stride, intent).  Pair 0 of every batch is the anchor, a pair
of max_tl x max_ql: it fixes the bounds the launch is sized by, and with them narrow or wide.  intent[k] says what pair k is for.
tests/test_small_cases.py checks the restated geometry against the planner and every case against the oracle (no GPU),
tests/test_gpu_small_seams.py runs the cases."""
import functools
import re
import zlib
from collections import namedtuple

import numpy as np

import range_guards as rg

SOFTCLIP, INDEL, LEADING_INDEL, IGNORE = 1, 2, 4, 8
STRATEGIES = (SOFTCLIP, INDEL, LEADING_INDEL, IGNORE)
GATK = (200, -150, 260, 11)
UNIT = (1, -1, 1, 1)
WIDE = (3000, -2500, 4000, 100)     # beyond 16 bits at every bound of this module that has a target of 64 rows or more
TIE_PARAMS = (UNIT, (5, -4, 10, 1), (3, -3, 0, 0))
LDS_LIMIT = 160 * 1024              # sw_small.hip: small_supported
ERR_CIGAR_OVERFLOW = 2              # include/mgl_sw.h

Case = namedtuple("Case", "name targets queries params strategies cigar_stride intent")
# kind: what the pair is for; row, col, n, d: the numbers its check needs (see intent_met)
Intent = namedtuple("Intent", "kind row col n d")
Intent.__new__.__defaults__ = (None, None, None, None)

_ALPHA = np.frombuffer(b"ACGT", np.uint8)
_ACG = np.frombuffer(b"ACG", np.uint8)


# ---- the kernel's geometry, restated (sw_small_pair.h, sw_small.hip)

def rows_per_lane(tl):
    """small_rows_per_lane"""
    return ((tl + 63) // 64 + 1) & ~1


def lanes(tl):
    """nl: the lanes that own rows"""
    r = rows_per_lane(tl)
    return (tl + r - 1) // r


def rows_past(tl):
    """rows the last lane owns beyond tl: whole lanes are stored"""
    return lanes(tl) * rows_per_lane(tl) - tl


def column_words(tl, wide):
    """small_column_words: dwords per kept column"""
    r, nl = rows_per_lane(tl), lanes(tl)
    if wide:
        return (nl * r) | 1
    cs = nl * r // 2
    return cs if (r // 2 - cs) & 1 else cs + 1


def lane_stride_words(tl, wide):
    """the distance in dwords between the cells two neighbouring lanes store in one step: one column back, one lane up"""
    r = rows_per_lane(tl)
    return (r if wide else r // 2) - column_words(tl, wide)


def text_cap(tl, ql, cigar_stride):
    """small_text_cap"""
    need = 2 * (tl + ql) + 4
    return (min(cigar_stride, need) + 3) & ~3


def lds_bytes(max_tl, max_ql, cigar_stride, wide):
    """small_lds_bytes"""
    kept = (max_tl + 8 if wide else (max_tl + 7) // 2 + 1) * (max_ql + 1) * 4
    return kept + ((max_tl + 3) & ~3) + ((max_ql + 3) & ~3) + text_cap(max_tl, max_ql, cigar_stride) + 8


def base(tl, ql, match, gopen, gext):
    """small_base: the middle of the range the kept values can take"""
    s = match * min(tl, ql) + (tl + ql) * gext - 2 * gopen - (tl + ql) * gext
    return s // 2 if s >= 0 else -(-s // 2)   # (C division: towards zero)


def supported(max_tl, max_ql, cigar_stride, match, mismatch, gopen, gext):
    """small_supported -> (ok, wide)"""
    if max_tl > 512 or max_tl < 1 or max_ql < 1 or not (match - mismatch < (1 << 23) and gext < (1 << 23)):
        return False, False
    wide = not rg.small_fits_int16(max_tl, max_ql, match, mismatch, gopen, gext)
    return lds_bytes(max_tl, max_ql, cigar_stride, wide) <= LDS_LIMIT, wide


def fill_schedule(tl, ql):
    """[(s0, form)] of the fill's blocks of four steps, form in 'masked', 'unmasked', 'clamp' (small_fill's four loops)"""
    nl = lanes(tl)
    steps = ql + nl - 1
    out, s0 = [], 0
    if nl == 64:
        while s0 < 64 and s0 < steps:
            out.append((s0, "masked"))
            s0 += 4
        while s0 + 3 <= ql - 1:
            out.append((s0, "unmasked"))
            s0 += 4
        if s0 >= 64:
            while s0 < steps:
                out.append((s0, "clamp"))
                s0 += 4
    while s0 < steps:
        out.append((s0, "masked"))
        s0 += 4
    return out


def block_step(row, col, tl):
    """u: which of its block's four steps computes cell (row, col) -- the lane's column j = s0 + u - lane + 1"""
    return (col - 1 + (row - 1) // rows_per_lane(tl)) % 4


def full_stride(max_tl, max_ql):
    """a CIGAR slot no pair of these bounds can overflow, a multiple of four"""
    return (2 * (max_tl + max_ql) + 4 + 3) & ~3


# ---- the recurrence and the walk, restated

def h_matrix(t, q, params, strategy):
    """H[0..tl][0..ql] (int64) of sw.cpp:5-146, column by column.  With gopen >= gext a gap never does better by opening from a cell
    that a gap of the same direction reached, so E[i][j] = max_r<i (H'[r][j] + r e) - o - (i - 1) e over H' = max(diag, F): a running
    maximum.  tests/test_small_cases.py holds this against range_guards.dp_full."""
    m, x, o, e = (int(v) for v in params)
    assert o >= e >= 0
    tl, ql = len(t), len(q)
    indel = (strategy & (INDEL | LEADING_INDEL)) != 0
    ta, qa = np.frombuffer(bytes(t), np.uint8), np.frombuffer(bytes(q), np.uint8)
    S = np.where(ta[:, None] == qa[None, :], m, x).astype(np.int64)
    H = np.zeros((tl + 1, ql + 1), np.int64)
    H[0, :] = rg.border(np.arange(ql + 1), o, e, indel)
    H[:, 0] = rg.border(np.arange(tl + 1), o, e, indel)
    ramp = np.arange(tl, dtype=np.int64) * e
    F = H[1:, 0] - o
    for j in range(1, ql + 1):
        if j > 1:
            F = np.maximum(H[1:, j - 1] - o, F - e)
        G = np.maximum(H[:-1, j - 1] + S[:, j - 1], F)
        above = np.concatenate([H[0:1, j], G[:-1]]) + ramp          # H'[r][j] + r e, r = 0 .. tl - 1
        H[1:, j] = np.maximum(G, np.maximum.accumulate(above) - o - ramp)
    return H, S


# every rule of the walk and of the last cells as the kernel has it; a test switches one off to ask whether a case can tell
Rules = namedtuple("Rules", "gap_largest later_round col_later_row row_nearer row_smaller_col row_strict")
RULES = Rules(True, True, True, True, True, True)


def score_max(H, rules=RULES):
    """ScoreMax (mqe, mqe_t, max, max_t, max_q, seg_length), sw.cpp:100-127: the last column keeps the later row; the last row keeps
    the nearer diagonal, then the smaller column; the row wins over the column only with rd < |mqe_t - ql|."""
    tl, ql = H.shape[0] - 1, H.shape[1] - 1
    col = H[1:, ql]
    mqe = int(col.max())
    rows = np.flatnonzero(col == mqe) + 1
    mqe_t = int(rows[-1] if rules.col_later_row else rows[0])
    row = H[tl, 1:]
    rm = int(row.max())
    js = np.flatnonzero(row == rm) + 1
    dist = np.abs(tl - js)
    rd = int(dist.min() if rules.row_nearer else dist.max())
    cand = js[dist == rd]
    rj = int(cand[0] if rules.row_smaller_col else cand[-1])
    cd = abs(mqe_t - ql)
    if rm > mqe or (rm == mqe and (rd < cd if rules.row_strict else rd <= cd)):
        return (mqe, mqe_t, rm, tl, rj, ql - rj)
    return (mqe, mqe_t, mqe, mqe_t, ql, 0)


def last_cells(H):
    """(rows of the last column that hold its maximum, columns of the last row that hold its maximum, the two maxima)"""
    tl, ql = H.shape[0] - 1, H.shape[1] - 1
    col, row = H[1:, ql], H[tl, 1:]
    return list(np.flatnonzero(col == col.max()) + 1), list(np.flatnonzero(row == row.max()) + 1), int(col.max()), int(row.max())


def gap_candidates(line, o, e):
    """value of candidate k = 1 .. len(line): line[-k] - o - (k - 1) e (line: H of the row or column in front of the cell)"""
    k = np.arange(1, len(line) + 1)
    return line[::-1] - o - (k - 1) * e


def _pick(vals, rules):
    """(value, k) as row_gap / column_gap pick it: 64 candidates a round, the largest k of a round's maximum, a later round wins a tie"""
    best = int(vals.max())
    at = np.flatnonzero(vals == best) + 1
    if not rules.gap_largest:
        return best, int(at[0])
    if rules.later_round:
        return best, int(at[-1])
    first = (at[0] - 1) // 64                       # an earlier round keeps its answer: the largest k of the first round that holds one
    return best, int(at[(at - 1) // 64 == first][-1])


def move(H, S, i, j, o, e, rules=RULES):
    """+k (k rows up), -k (k columns left) or 0: a cell is a diagonal move iff H == diag, else a row gap if F == H, else a column gap"""
    h = H[i, j]
    if h == H[i - 1, j - 1] + S[i - 1, j - 1]:
        return 0
    fv, fk = _pick(gap_candidates(H[i, :j], o, e), rules)
    if fv == h:
        return -fk
    return _pick(gap_candidates(H[:i, j], o, e), rules)[1]


def walk(t, q, params, strategy, rules=RULES, HS=None):
    """(offset, cigar, ScoreMax): calculateCigar (sw.cpp:149-255) on the moves read off H"""
    H, S = HS if HS is not None else h_matrix(t, q, params, strategy)
    o, e = int(params[2]), int(params[3])
    tl, ql = len(t), len(q)
    sc = score_max(H, rules)
    D = H[1:, 1:] == H[:-1, :-1] + S
    out = []

    def push(op, n):
        if n > 0:
            out.append(f"{n}{op}")

    seg = 0
    if strategy == INDEL:
        I, J = tl, ql
    elif strategy == LEADING_INDEL:
        I, J = sc[1], ql
    else:
        I, J, seg = sc[3], sc[4], sc[5]
    if seg > 0 and strategy == SOFTCLIP:
        push("S", seg)
        seg = 0
    state = "M"
    while True:
        if D[I - 1, J - 1]:
            back = np.diagonal(D[:I, :J][::-1, ::-1])
            stop = np.flatnonzero(~back)
            nxt, step = "M", int(stop[0]) if len(stop) else len(back)
            I, J = I - step, J - step
        else:
            b = move(H, S, I, J, o, e, rules)
            if b > 0:
                nxt, step = "D", b
                I -= b
            else:
                nxt, step = "I", -b
                J += b
        if nxt == state:
            seg += step
        else:
            push(state, seg)
            seg, state = step, nxt
        if not (I > 0 and J > 0):
            break
    if strategy == SOFTCLIP:
        push(state, seg)
        push("S", J)
        off = I
    elif strategy == IGNORE:
        push(state, seg + J)
        off = I - J
    else:
        push(state, seg)
        push("D", I) if I > 0 else push("I", J)
        off = 0
    return off, "".join(reversed(out)), sc


# ---- what a CIGAR says about the path

_CIGAR = re.compile(r"(\d+)([MIDS])")


def elements(cigar):
    return [(int(n), op) for n, op in _CIGAR.findall(cigar)]


def gap_row(offset, cigar, op, n, before, after):
    """The target row of the first cell of the run of n `op` that stands between exactly `before` M and exactly `after` M (D: the
    first row deleted; I: the row the run stays on); None if the CIGAR holds no such run."""
    el = elements(cigar)
    i = int(offset)
    for k, (m, o) in enumerate(el):
        if (m, o) == (n, op) and 0 < k < len(el) - 1 and el[k - 1] == (before, "M") and el[k + 1] == (after, "M"):
            return i + 1 if op == "D" else i
        if o in "MD":
            i += m
    return None


# ---- sequences

def _rand(rng, n, alpha=_ALPHA):
    return alpha[rng.integers(0, len(alpha), int(n))]


def _other(rng, b, alpha=_ALPHA):
    k = int(np.flatnonzero(alpha == b)[0]) if b in alpha else 0
    return alpha[(k + int(rng.integers(1, len(alpha)))) % len(alpha)]


def _unrelated(rng, n, near):
    """n bases of which none equals the base of ``near`` at the same place (cyclically)"""
    if n <= 0:
        return np.zeros(0, np.uint8)
    near = np.asarray(near, np.uint8)
    ref = near[np.arange(n) % len(near)] if len(near) else np.full(n, ord("A"), np.uint8)
    return _ALPHA[(np.searchsorted(_ALPHA, ref) + rng.integers(1, 4, n)) % 4]


def _b(a):
    return a if isinstance(a, bytes) else bytes(np.asarray(a, np.uint8))


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def make_case(name, pairs, params, strategies=STRATEGIES, cigar_stride=None, wide=None, on_kernel=True):
    """A batch of [(target, query, intent)] behind its anchor: a random target of max_tl rows and a query of max_ql bases cut from
    it.  ``wide``: what the batch's bounds have to make of the kept scores (None: whatever they make); ``on_kernel`` False: a batch
    that small_supported must refuse."""
    rng = _rng(name)
    max_tl, max_ql = max(len(p[0]) for p in pairs), max(len(p[1]) for p in pairs)
    t = _rand(rng, max_tl)
    q = np.resize(t[int(rng.integers(0, max(1, max_tl // 3))):], max_ql).copy()
    for x in np.flatnonzero(rng.random(max_ql) < 0.03):
        q[x] = _other(rng, q[x])
    stride = full_stride(max_tl, max_ql) if cigar_stride is None else cigar_stride
    ok, w = supported(max_tl, max_ql, stride, *params)
    assert ok == on_kernel, (name, max_tl, max_ql, params)
    assert wide is None or w == wide, (name, max_tl, max_ql, params, w)
    pairs = [(_b(t), _b(q), Intent("anchor", max_tl, max_ql))] + list(pairs)
    return Case(name, tuple(_b(p[0]) for p in pairs), tuple(_b(p[1]) for p in pairs), tuple(params), tuple(strategies), stride,
                tuple(p[2] for p in pairs))


def split_cases(name, pairs, params, strategies=STRATEGIES, wide=None):
    """The pairs in batches whose bounds small_supported admits (and that are wide or narrow as asked), in order; a pair that no batch
    can hold -- its own lengths are beyond the kernel -- is left out and named in the second list."""
    out, left, cur, part = [], [], [], 0

    def fits(ps, form=wide):
        mt, mq = max(len(p[0]) for p in ps), max(len(p[1]) for p in ps)
        ok, w = supported(mt, mq, full_stride(mt, mq), *params)
        return ok and (form is None or w == form)

    for p in pairs:
        if not fits([p], None):
            left.append(p)
        elif cur and not fits(cur + [p]):
            out.append(make_case(f"{name}/{part}", cur, params, strategies, wide=wide))
            cur, part = [p], part + 1
        else:
            cur.append(p)
    if cur:
        out.append(make_case(f"{name}/{part}", cur, params, strategies, wide=wide))
    return out, left


# ---- rows: every R, both sides of every nl == 64 edge, odd tl, 1 .. 7 rows past tl

ROWS_TL = sorted({1, 2, 3, 63, 64, 65} | set(range(126, 131)) | set(range(191, 194)) | set(range(252, 258)) | set(range(319, 322))
                 | set(range(378, 386)) | set(range(447, 450)) | set(range(504, 513)))
ROWS_QL = [1, 2, 3, 4, 5] + list(range(63, 73)) + [150]


def lane_seam(tl):
    """(the last row of a lane, the first row of the lane above it) near the middle of the target; one lane: (its last row, row 1)"""
    r = rows_per_lane(tl)
    if tl <= r:
        return tl, 1
    b = r * max(1, (tl // 2) // r)
    return b, b + 1


def rows_pairs(tl, ql, rng):
    """identical (the query is the target's tail), one substitution in the last row of a lane, one in the first row of a lane, unrelated"""
    t = _rand(rng, tl)
    out = [(t, t[tl - ql:] if ql <= tl else np.concatenate([_unrelated(rng, ql - tl, t), t]), Intent("identical", tl, ql))]
    for row in lane_seam(tl):
        if ql <= tl:
            lo = min(max(row - 1 - ql // 2, 0), tl - ql)
            q = t[lo:lo + ql].copy()
            q[row - 1 - lo] = _other(rng, t[row - 1])
        else:
            q = np.concatenate([_unrelated(rng, ql - tl, t), t])
            q[ql - tl + row - 1] = _other(rng, t[row - 1])
        out.append((t, q, Intent("substitution", row, None)))
    out.append((t, _rand(rng, ql), Intent("unrelated", tl, ql)))
    return out


def rows_cases():
    out, left = [], []
    for params, wide in ((GATK, False), (WIDE, True)):
        for ql in ROWS_QL:
            name = f"rows/{'wide' if wide else 'narrow'}/ql{ql}"
            rng = _rng(name)
            pairs = [p for tl in ROWS_TL[::-1] for p in rows_pairs(tl, ql, rng)]    # (longest first: the first batch holds what fits)
            cs, lo = split_cases(name, pairs, params, wide=wide)
            out += cs
            left += [(len(p[0]), len(p[1]), wide) for p in lo]
    return out, left


# ---- ramps: the full-wave ends and their ragged partners against every query length around the three stages of the fill

RAMPS_TL = (128, 256, 384, 512, 127, 253, 379, 505)
RAMPS_QL = list(range(1, 9)) + list(range(60, 77))


def ramps_pairs(tl, ql, rng):
    """Targets of A, C and G; T is what matches nothing.  The first pair's best cell lies in the last column on a row of lane 63 (the
    query is the piece of the target that ends there), the twin's in the last row (the query goes on with T behind the target's end)."""
    r = rows_per_lane(tl)
    t = _rand(rng, tl, _ACG)
    row = tl if ql < 12 else 63 * r + 1
    out = [(t, t[row - ql:row], Intent("last_column", row, ql))]
    if ql >= 2:
        k = ql - max(1, ql // 4)
        out.append((t, np.concatenate([t[tl - k:], np.full(ql - k, ord("T"), np.uint8)]), Intent("last_row", tl, k)))
    return out


def ramps_cases():
    out = []
    for tl in RAMPS_TL:
        for params, name in ((GATK, "narrow"), (WIDE, "wide")):
            nm = f"ramps/{name}/tl{tl}"
            rng = _rng(nm)
            pairs = [p for ql in RAMPS_QL for p in ramps_pairs(tl, ql, rng)]
            if name == "wide":      # (512 x 76 in 32 bits fits; the next query length does not)
                pairs = [p for p in pairs if supported(tl, len(p[1]), full_stride(tl, len(p[1])), *params)[0]]
            cs, left = split_cases(nm, pairs, params, strategies=(SOFTCLIP, INDEL))
            assert not left
            out += cs
    return out


# ---- runs: one gap of a round's length between diagonal stretches of a round's length

RUN_GAPS = (1, 2, 63, 64, 65, 127, 128, 129)
RUN_DIAGS = (63, 64, 65, 127, 128, 129, 192)
RUN_FLANK = 24          # the stretch on the other side of the gap
RUN_PARAMS = (GATK, UNIT)
RUN_JUDGE = {GATK: SOFTCLIP, UNIT: INDEL}   # the strategy a run case is judged under: (1, -1, 1, 1) pays a long gap only on a path that must


def del_pair(rng, before, n, after, place):
    """M before, D n, M after.  place 'start': the first deleted row is the last row of a lane; 'end': the last deleted row is the
    first row of a lane -- by unrelated rows in front of the target, as many as it takes (they change tl, and tl changes R)."""
    for pad in range(0, 17):
        tl = pad + before + n + after
        r = rows_per_lane(tl)
        first = pad + before + 1
        if (place == "start" and first % r == 0) or (place == "end" and (first + n - 1) % r == 1):
            break
    else:
        raise AssertionError((before, n, after, place))
    s = _rand(rng, before + after)
    x = _unrelated(rng, n, s[before:])
    bad = {int(s[before - 1]), int(s[before])} if n == 1 else {int(s[before - 1])}
    if int(x[-1]) in bad:
        x[-1] = next(c for c in _ALPHA if int(c) not in bad)
    t = np.concatenate([_unrelated(rng, pad, s), s[:before], x, s[before:]])
    return t, s, Intent("del_" + place, first, None, n, (before, after))


def ins_pair(rng, before, n, after):
    """M before, I n, M after: the run covers columns before + 1 .. before + n on row `before`"""
    s = _rand(rng, before + after)
    x = _unrelated(rng, n, s[before:])
    bad = {int(s[before - 1]), int(s[before])} if n == 1 else {int(s[before - 1])}
    if int(x[-1]) in bad:
        x[-1] = next(c for c in _ALPHA if int(c) not in bad)
    return s, np.concatenate([s[:before], x, s[before:]]), Intent("ins", before, before + 1, n, (before, after))


def runs_pairs(rng):
    out = []
    for n in RUN_GAPS:
        for d in RUN_DIAGS:
            for before, after in ((d, RUN_FLANK), (RUN_FLANK, d)):
                out += [del_pair(rng, before, n, after, "start"), del_pair(rng, before, n, after, "end"), ins_pair(rng, before, n, after)]
    return out


def run_intent_met(pair, cigar, offset):
    t, q, it = pair
    op = "D" if it.kind.startswith("del") else "I"
    return gap_row(offset, cigar, op, it.n, *it.d) == it.row


def _oracle_batch(ts, qs, params, strategy):
    import oracle_lib as ol

    return ol.oracle_align_batch(list(ts), list(qs), params, strategy, nthreads=8)


def runs_cases():
    """-> (cases, pairs generated, pairs dropped because the oracle's path does not do what they were built for)"""
    out, made, dropped = [], 0, 0
    for params in RUN_PARAMS:
        name = f"runs/{params[0]}"
        pairs = runs_pairs(_rng(name))
        off, _, cg = _oracle_batch([p[0] for p in pairs], [p[1] for p in pairs], params, RUN_JUDGE[params])
        keep = [p for k, p in enumerate(pairs) if run_intent_met(p, cg[k], off[k])]
        made, dropped = made + len(pairs), dropped + len(pairs) - len(keep)
        for kind in ("del", "ins"):         # (deletions are tall, insertions wide: together their bounds would not fit LDS)
            cs, left = split_cases(f"{name}/{kind}", sorted((p for p in keep if p[2].kind.startswith(kind)), key=lambda p: len(p[0]) * len(p[1])),
                                   params)
            assert not left
            out += cs
    return out, made, dropped


# ---- round_ties: a row gap whose candidates tie across the first round of 64, found by a seeded search

ROUND_TIE_LIMIT = 200000
_EARLY = RULES._replace(later_round=False)


def round_tie_draw(rng):
    """a low-entropy pair of at most 40 x 200: a short two-letter target, a query of pieces of it between long runs of one letter"""
    ab = _ALPHA[rng.permutation(4)[:2]]
    t = ab[(rng.random(int(rng.integers(6, 41))) < 0.5).astype(int)]
    parts = []
    while sum(map(len, parts)) < 200:
        a = int(rng.integers(0, len(t)))
        parts.append(t[a:a + int(rng.integers(1, 12))])
        parts.append(np.full(int(rng.integers(40, 100)) if rng.random() < 0.5 else int(rng.integers(1, 6)), ab[int(rng.integers(0, 2))], np.uint8))
    return t, np.concatenate(parts)[:int(rng.integers(70, 201))]


def round_tie_search(params, strategy, seed, limit):
    """The first drawn pair whose CIGAR changes when an earlier round of 64 gap candidates keeps a tie against a later one -- the
    candidate lengths k1 <= 64 < k2 hold the same value and the cell at k1 was reached diagonally, or the two texts would be one --
    and how many pairs were drawn; (None, limit) if there is none."""
    rng = np.random.default_rng(seed)
    for n in range(1, limit + 1):
        t, q = round_tie_draw(rng)
        HS = h_matrix(t, q, params, strategy)
        if walk(t, q, params, strategy, RULES, HS)[:2] != walk(t, q, params, strategy, _EARLY, HS)[:2]:
            return (t, q), n
    return None, limit


ROUND_TIE_SEEDS = {UNIT: 1, (5, -4, 10, 1): 2, (3, -3, 0, 0): 3}
ROUND_TIE_BUDGET = 400    # pairs drawn per parameter set here (the issue's bound on the whole search: ROUND_TIE_LIMIT)


def round_ties_cases():
    out = []
    for params in TIE_PARAMS:
        for strategy in (SOFTCLIP, INDEL):
            found, _ = round_tie_search(params, strategy, ROUND_TIE_SEEDS[params] * 10 + strategy, ROUND_TIE_BUDGET)
            if found:
                out.append(make_case(f"round_ties/{params[0]}/{strategy}", [(found[0], found[1], Intent("round_tie"))], params, (strategy,)))
    return out


# ---- last_cell_ties: the two passes over the wave that pick the last column's and the last row's cell

TIE_TL = (128, 256, 100)
TIE_RULES = ("col_later_row", "row_nearer", "row_smaller_col", "row_strict")
TIE_ORDERS = ("lt", "eq", "gt")         # rd against |mqe_t - ql| where the row's best equals the column's best in another cell
TIE_DRAWS = 600                         # two-letter pairs drawn per shape at most


def tie_order(H):
    """'lt', 'eq' or 'gt' -- rd against |mqe_t - ql| -- where the last row's best equals the last column's best and the row's nearest
    cell is not the column's cell; else None"""
    tl, ql = H.shape[0] - 1, H.shape[1] - 1
    rows, cols, cm, rm = last_cells(H)
    if cm != rm:
        return None
    rd, cd = min(abs(tl - j) for j in cols), abs(rows[-1] - ql)
    if rows[-1] == tl and [j for j in cols if abs(tl - j) == rd][0] == ql:
        return None
    return "lt" if rd < cd else "eq" if rd == cd else "gt"


def tie_flips(H):
    """the rules of TIE_RULES under whose opposite the pair's ScoreMax changes"""
    right = score_max(H)
    return {r for r in TIE_RULES if score_max(H, RULES._replace(**{r: False})) != right}


def tie_draw(rng, tl):
    """a two-letter target and a query cut from it with a few letters flipped, a few bases shorter or longer than the target; every
    second draw the other way round (the transposed matrix: what the last row did, the last column does)"""
    ab = _ALPHA[rng.permutation(4)[:2]]
    swap = rng.random() < 0.5
    n = tl + int(rng.integers(-12, 13))
    a_len, b_len = (n, tl) if swap else (tl, n)
    a = ab[(rng.random(a_len) < rng.choice([0.5, 0.8, 0.95])).astype(int)]
    b = np.resize(a[int(rng.integers(0, 12)):], b_len).copy()
    flip = rng.random(b_len) < rng.choice([0.0, 0.03, 0.1])
    b[flip] = ab[rng.integers(0, 2, int(flip.sum()))]
    return (b, a) if swap else (a, b)


# (rows to the left, columns to the right, rows left over, defects) of shifted_pair: (tl - dl) match = (tl - g) match - defects (match - mismatch)
SHIFTS = {UNIT: {"eq": (2, 2, 0, 1), "gt": (3, 1, 1, 1)}, (5, -4, 10, 1): {"eq": (9, 9, 0, 5), "gt": (10, 2, 1, 5)}}


def shifted_pair(tl, shape, junk, rng):
    """A target of period dl + dr and a query that is the target dl rows later up to column tl - dl and dr rows earlier from there
    on.  The diagonal from (dl, 0) reaches the last row at (tl, tl - dl) with tl - dl matches; the one from (0, dr) reaches the last
    column at (tl - g, ql), ql = tl - g + dr, with tl - g matches but for `defects` residues of the period that change once, half way
    down: the same score, dl from the main diagonal against dr.  junk: one more query base that matches nothing there, and the last
    column is out of it."""
    dl, dr, g, defects = shape
    P = dl + dr
    X = _rand(rng, P)
    while any((X == np.roll(X, k)).mean() > 0.5 for k in range(1, P)):
        X = _rand(rng, P)
    Y = X.copy()
    for r in rng.permutation(P)[:defects]:
        Y[r] = _other(rng, X[r])
    k = np.arange(1, tl + 1)
    t = np.where(k < tl // 2 + dl, X[k % P], Y[k % P])
    q = np.concatenate([t[dl:], t[tl - P:tl - g]])
    return t, np.concatenate([q, [_other(rng, t[-1])]]) if junk else q


def last_cell_pairs(tl, params, rng):
    """Homopolymers and two-letter periodic pairs whose last column ties inside a lane's rows and across lanes; then, drawn until
    every one is there, a pair for each rule of TIE_RULES that the opposite rule gets wrong, and a pair for each order of TIE_ORDERS."""
    n = tl - 37
    two = lambda s, k: np.frombuffer((s * k)[:k], np.uint8)  # noqa: E731
    out = [(two(b"A", tl), two(b"A", n), Intent("column_tie", tl, n)),            # every row from n on ties: the later row, lane after lane
           (two(b"AC", tl), two(b"CA", n), Intent("column_tie", None, n)),        # every second row
           (two(b"A", tl), two(b"A", tl + 20), Intent("row_tie", tl, tl))]        # columns tl .. tl + 20 tie: the diagonal's
    want = {("flips", r) for r in TIE_RULES} | {("order", o) for o in TIE_ORDERS}
    for t, q, _ in out:                 # (what the three above show already: the later row, the nearer diagonal, rd < |mqe_t - ql|)
        H, _ = h_matrix(t, q, params, SOFTCLIP)
        want -= {("flips", r) for r in tie_flips(H)} | {("order", tie_order(H))}
    built = [(SHIFTS[params]["eq"], False), (SHIFTS[params]["eq"], True), (SHIFTS[params]["gt"], False)] * 3   # (a period may match itself: three goes)
    for n in range(TIE_DRAWS):
        if not want:
            break
        t, q = shifted_pair(tl, *built[n], rng) if n < len(built) else tie_draw(rng, tl)
        H, _ = h_matrix(t, q, params, SOFTCLIP)
        got = ({("flips", r) for r in tie_flips(H)} | {("order", tie_order(H))}) & want
        if got:
            want -= got
            out.append((t, q, Intent("tie", tuple(sorted(v for k, v in got if k == "flips")), next((v for k, v in got if k == "order"), None))))
    return out, want


def last_cell_cases():
    """-> (cases, [(tl, params, what no draw gave)])"""
    out, missing = [], []
    for tl in TIE_TL:
        for params in (UNIT, (5, -4, 10, 1)):
            nm = f"last_cell_ties/tl{tl}/{params[0]}"
            pairs, want = last_cell_pairs(tl, params, _rng(nm))
            out.append(make_case(nm, pairs, params, (SOFTCLIP, IGNORE, LEADING_INDEL)))
            missing += [(tl, params, w) for w in sorted(want)]
    return out, missing


# ---- bytes: the base codes of the lookup path and the raw bytes of the compare path

SHARES = ((ord("N"), ord("G")), (ord("a"), ord("A")), (ord("c"), ord("C")), (ord("g"), ord("G")), (ord("t"), ord("T")), (ord("B"), ord("C")),
          (0x00, ord("A")), (0xff, ord("G")))        # a byte that is no base, and the base whose two code bits ((b >> 1) & 3) it shares
BYTES_TL = (100, 200, 330, 450)                       # R = 2, 4, 6, 8
BYTES_QL = 60


def code_bits(b):
    return (b >> 1) & 3


def bytes_pairs(tl, rng):
    out = []
    lo = (tl - BYTES_QL) // 2
    t0 = _rand(rng, tl)
    for byte, shares in SHARES:                       # ACGT target, the byte opposite the base it shares a code with, on the diagonal
        t, cols = t0.copy(), []
        for u in (0, 3):                              # ... in the first and in the last step of a block of four
            j = next(j for j in range(8 + 20 * (u > 0), BYTES_QL) if block_step(lo + j, j, tl) == u)
            t[lo + j - 1] = shares
            cols.append(j)
        q = t[lo:lo + BYTES_QL].copy()
        q[[j - 1 for j in cols]] = byte
        out.append((t, q, Intent("query_byte", byte, tuple(cols))))
    for row in (1, tl, lane_seam(tl)[1]):             # a target with one N: the byte compare for the whole pair
        t = t0.copy()
        t[row - 1] = ord("N")
        a = min(max(row - 1 - BYTES_QL // 2, 0), tl - BYTES_QL)
        for q_has_n in (True, False):
            q = t[a:a + BYTES_QL].copy()
            if not q_has_n:
                q[row - 1 - a] = ord("G")
            out.append((t, q, Intent("target_n", row, int(q_has_n))))
    lower = np.frombuffer(bytes(t0).lower(), np.uint8)
    out.append((lower, lower[lo:lo + BYTES_QL], Intent("lower_both")))
    out.append((lower, t0[lo:lo + BYTES_QL], Intent("lower_target")))
    high = np.array([0x80, 0x91, 0xa2, 0xff], np.uint8)[rng.integers(0, 4, tl)]
    q = high[lo:lo + BYTES_QL].copy()
    out.append((high, q, Intent("high_equal")))
    q = q.copy()
    q[::7] ^= 0x40
    out.append((high, q, Intent("high_unequal")))
    out.append((high, t0[lo:lo + BYTES_QL], Intent("high_target")))
    return out


def bytes_cases():
    out = []
    for tl in BYTES_TL:
        for params, wide in ((GATK, False), (WIDE, True)):
            nm = f"bytes/tl{tl}/{'wide' if wide else 'narrow'}"
            out.append(make_case(nm, bytes_pairs(tl, _rng(nm)), params, (SOFTCLIP, INDEL), wide=wide))
    return out


# ---- span: the narrow form at the edge of small_fits_int16, one step past it the wide one

SPAN_SHAPES = ((256, 150, (400, -300, 400, 5), 2), (128, 300, (400, -300, 470, 5), 0))   # (tl, ql, where the walk starts, the parameter walked)


def span_edge(tl, ql, start, index):
    return rg.param_edge(lambda *p: rg.small_fits_int16(tl, ql, *p), start, index, +1, 100000)


def span_pairs(tl, ql):
    half = ql // 2
    out = []
    for rows in (tl, tl - 3):     # (253: rows past tl must not matter)
        out += [(b"A" * rows, b"A" * ql, Intent("all_match", rows, ql)), (b"A" * rows, b"C" * ql, Intent("all_mismatch", rows, ql)),
                (b"A" * rows, b"A" * half + b"C" * (ql - half), Intent("half", rows, ql)), (b"A" * rows, b"C" * half + b"A" * (ql - half), Intent("half", rows, ql))]
    return [(np.frombuffer(t, np.uint8), np.frombuffer(q, np.uint8), it) for t, q, it in out]


def span_cases():
    out = []
    for tl, ql, start, index in SPAN_SHAPES:
        edge = span_edge(tl, ql, start, index)
        for params, wide in ((edge, False), (rg.past(edge, index, 1), True)):
            on = supported(tl, ql, full_stride(tl, ql), *params)[0]    # (128 x 300 in 32 bits is beyond LDS: one past the edge leaves the kernel)
            out.append((make_case(f"span/{tl}x{ql}/{'past' if wide else 'edge'}", span_pairs(tl, ql), params, (SOFTCLIP, INDEL), wide=wide, on_kernel=on), on))
    return out


# ---- fits: the largest geometry that LDS admits, and the query's staging in blocks of 512

FITS_TL = (64, 128, 256, 384, 512)
FITS_STRIDE = 64          # what mgl_sw_explain plans with
STAGING_QL = (511, 512, 513, 1023, 1024, 1025, 2048)


def largest_ql(tl, params, cigar_stride=FITS_STRIDE):
    return rg.last_true(lambda ql: supported(tl, ql, cigar_stride, *params)[0], 1, 1 << 16)


def fits_pairs(tl, ql, rng):
    """CIGARs of a few characters: the target inside the query (the query inside the target), all mismatch, the last base alone"""
    if ql >= tl:
        q = _rand(rng, ql)
        a = min(ql - tl, 500 if ql > 540 else ql // 3)     # (the match straddles the query's staging seam at 512 where there is one)
        hit = (q[a:a + tl].copy(), q)
        tail = (q[ql - tl:].copy(), q)
    else:
        t = _rand(rng, tl)
        hit, tail = (t, t[tl // 3:tl // 3 + ql].copy()), (t, t[tl - ql:].copy())
    return [hit + (Intent("inside", tl, ql),), tail + (Intent("inside", tl, ql),),
            (np.full(tl, ord("A"), np.uint8), np.full(ql, ord("C"), np.uint8), Intent("all_mismatch", tl, ql))]


def fits_cases():
    """-> [(case, on_kernel)]: at the largest admitted query length the kernel, one past it another"""
    out = []
    for tl in FITS_TL:
        for params, wide in ((GATK, False), (WIDE, True)):
            edge = largest_ql(tl, params)
            assert supported(tl, edge, FITS_STRIDE, *params) == (True, wide), (tl, edge, params)
            for ql, on in ((edge, True), (edge + 1, False)):
                nm = f"fits/tl{tl}/{'wide' if wide else 'narrow'}/ql{ql}"
                pairs = fits_pairs(tl, ql, _rng(nm))
                if on:
                    out.append((make_case(nm, pairs, params, (SOFTCLIP,), cigar_stride=FITS_STRIDE, wide=wide), True))
                else:
                    out.append((make_case(nm, pairs, params, (SOFTCLIP,), cigar_stride=FITS_STRIDE, on_kernel=False), False))
    for ql in STAGING_QL:
        nm = f"fits/staging/ql{ql}"
        rng = _rng(nm)
        top = max(tl for tl in range(1, 38) if supported(tl, ql, FITS_STRIDE, *GATK)[0])     # (37 up to 1 025 bases, 29 at 2 048)
        pairs = [p for tl in (top, 5, 1) for p in fits_pairs(tl, ql, rng)]
        out.append((make_case(nm, pairs, GATK, (SOFTCLIP, INDEL), cigar_stride=FITS_STRIDE), True))
    return out


# ---- slots: CIGAR slots that are exact, one short, and no multiple of four bytes wide

def slots_pairs(rng):
    """CIGARs of a known length: 60M (3), 20M3D40M (8), 25M11I35M (10), 20M3D15M2I23M (13)"""
    s = _rand(rng, 60)
    out = [(np.concatenate([_unrelated(rng, 20, s), s, _unrelated(rng, 20, s[::-1])]), s)]
    t, q, _ = del_pair(rng, 20, 3, 40, "start")
    out.append((t, q))
    t, q, _ = ins_pair(rng, 25, 11, 35)
    out.append((t, q))
    t1, q1, _ = del_pair(rng, 20, 3, 15, "start")
    t2, q2, _ = ins_pair(rng, 0 + 1, 2, 23)
    return out + [(np.concatenate([t1, t2[1:]]), np.concatenate([q1, q2[1:]]))]


def slots_cases():
    """one batch per stride: L - 1, L, L + 1, L + 3 around each pair's own L, and 7, 9, 513 (no multiple of four: the byte-wise copy)"""
    import oracle_lib as ol

    pairs = slots_pairs(_rng("slots"))
    lengths = sorted({len(ol.oracle_align(_b(t), _b(q), GATK, SOFTCLIP)["cigar"]) for t, q in pairs})
    strides = sorted({L + d for L in lengths for d in (-1, 0, 1, 3)} | {7, 9, 513})
    out = []
    for stride in strides:
        ps = [(t, q, Intent("slot", None, None, stride)) for t, q in pairs]
        c = make_case(f"slots/{stride}", ps, GATK, (SOFTCLIP,), cigar_stride=stride)
        out.append(c)
    return out, lengths


# ---- what the oracle's answer has to say about a pair

def intent_met(case, k, score, H=None):
    v = _intent_met(case, k, score, H)
    return None if v is None else bool(v)


def _intent_met(case, k, score, H):
    """Does the oracle's ScoreMax (under SOFTCLIP) do what pair k of the case was built for?  None: the kind promises nothing here."""
    it = case.intent[k]
    tl, ql = len(case.targets[k]), len(case.queries[k])
    mqe, mqe_t, mx, max_t, max_q, seg = (int(v) for v in score)
    if it.kind == "last_column":
        return (mqe_t - 1) // rows_per_lane(tl) == 63 and mqe_t == it.row and max_q == ql and seg == 0
    if it.kind == "last_row":
        return max_t == tl and max_q == it.col and seg == ql - it.col
    if it.kind in ("column_tie", "row_tie"):
        rows, cols, cm, rm = last_cells(H)
        r = rows_per_lane(tl)
        if it.kind == "column_tie":     # ... inside one lane's rows and across lanes; the later row
            in_lanes = [(x - 1) // r for x in rows]
            inside = len(in_lanes) > len(set(in_lanes)) or it.row is None       # (every second row: with R = 2 one row a lane)
            return len(set(in_lanes)) >= 2 and inside and mqe_t == rows[-1] and rows[-1] >= tl - 1
        return len(cols) >= 2 and (max_t, max_q) == (tl, it.col) and min(abs(tl - j) for j in cols) == 0
    if it.kind == "tie":
        return set(it.row) <= tie_flips(H) and (it.col is None or tie_order(H) == it.col)
    return None


@functools.lru_cache(maxsize=None)
def built():
    """Every set, built once: {set name: [Case]} and what the builders have to report."""
    rows, rows_left = rows_cases()
    runs, made, dropped = runs_cases()
    slots, slot_lengths = slots_cases()
    fits, span = fits_cases(), span_cases()
    ties, ties_missing = last_cell_cases()
    sets = {"rows": rows, "ramps": ramps_cases(), "runs": runs, "round_ties": round_ties_cases(), "last_cell_ties": ties,
            "bytes": bytes_cases(), "span": [c for c, _ in span], "fits": [c for c, _ in fits], "slots": slots}
    report = {"rows_left": rows_left, "runs_made": made, "runs_dropped": dropped, "slot_lengths": slot_lengths, "ties_missing": ties_missing,
              "on_kernel": {c.name: on for c, on in fits + span}}
    return sets, report


def cases(name):
    return built()[0][name]


def service_subset():
    """About 150 pairs for the one-pair entry: (target, query, params, strategy, where) -- every R, pairs of every set, one that needs
    more than 64 KiB of LDS"""
    sets, _ = built()
    out = []
    for name, cs in sets.items():
        if name in ("slots",):
            continue
        want = 32 if name == "rows" else 16
        step = max(1, sum(len(c.targets) - 1 for c in cs) // want)
        n = 0
        for c in cs:
            for k in range(1, len(c.targets)):
                if n % step == 0 and len(c.targets[k]) <= 512 and len(c.queries[k]) <= 2048:
                    out.append((c.targets[k], c.queries[k], c.params, c.strategies[(n // step) % len(c.strategies)], f"{c.name}[{k}]"))
                n += 1
    big = next(c for c in sets["rows"] if c.name.startswith("rows/narrow/ql150"))
    k = next(k for k in range(1, len(big.targets)) if len(big.targets[k]) == 512)
    out.append((big.targets[k], big.queries[k], big.params, SOFTCLIP, f"{big.name}[{k}] (more than 64 KiB of LDS)"))
    return out
