"""Inputs that put the long-read strip kernel (sw_dp16_strip.hip, sw_strip_walk.hip) on its seams at a CHOSEN strip height.

The planner derives the rows per strip from the longest target of a batch: with n = 128 * waves * passes strip slots it takes the
smallest height c of 17 .. 31 (22 .. 31 with several passes) with ceil(tl / c) <= n, else 32.  height_interval() restates that rule,
seam_strips() names the strips at which something changes hands -- lane 63 -> the next wave's lane 0 through the LDS mailbox, strip
NL - 1 (low halves) -> strip NL (high halves), the last strip of a pass -> the first of the next through the kept row -- and cases()
builds small pairs whose paths cross exactly those rows: on a diagonal, in a vertical run, in a horizontal run lying over a baseline
move or over the band's checkpoint column.  Every batch holds the anchor, a target of the interval's last length, so that the
planner chooses the height the cases were built for.  Pure Python and numpy; tests/test_strip_cases.py checks on the CPU, from the
oracle's CIGARs, that the cases mean what they say, tests/test_gpu_strip_heights.py runs them."""
import re
from collections import namedtuple

import numpy as np

SOFTCLIP, INDEL, LEADING_INDEL, IGNORE = 1, 2, 4, 8
STRATEGIES = (SOFTCLIP, INDEL, LEADING_INDEL, IGNORE)
GATK = (200, -150, 260, 11)
NOT_FOLDING = (25, -50, 110, 6)
CPS, CK_COLS = 4, 128                       # sw_device.h: STRIP_CPS, STRIP_CK_COLS
QL_CYCLE = (37, 64, 65, 127, 128, 129, 131)  # groups of four, baseline blocks of 16, the 128-column checkpoint
TINY_QL = (1, 3, 4, 5, 15, 16, 17)
MAX_QL = 160
NOISE = 0.03
BORDER_REACH = 1000                         # rows: 11 a row against the 200 a base of a 130-base window, with a margin of two

Case = namedtuple("Case", "target query strategy intent")
# family: anchor | row_tl | col_tl | diag | del | ins16 | insck | tiny | bytes_t | bytes_q | bytes_both
# row: the boundary row b (diag, del, ins*, bytes*) or tl (row_tl, col_tl, tiny); col: the column an I run is to contain; r: (tl - 1) % sr
Intent = namedtuple("Intent", "family row col r strip")
Intent.__new__.__defaults__ = (None, None, None, None)

_ALPHA = np.frombuffer(b"ACGT", np.uint8)


def bands_k(sr):
    """strips per kept band of the kernels without stored flags (sw_capi.cpp: 64 / rows)"""
    return 64 // sr


def slots(waves, passes=1):
    return 128 * waves * passes


def first_strip_target():
    """The shortest target (max_ql = max_tl) a default context gives to the strip kernel: the planner wants 40 % of the issued lanes
    to be real cells -- strips of the 128 slots x column groups of all steps (sw_capi.cpp: used >= 0.4)."""
    tl = 1
    while True:
        g = (tl + CPS - 1) // CPS
        if ((tl + 16) // 17) / 128.0 * g / (g + 127) >= 0.4:
            return tl
        tl += 1


def height_interval(sr, waves, passes=1):
    """(lo, hi): the longest targets of a batch for which the planner runs strips of sr rows on waves waves in passes passes."""
    if waves not in (1, 2, 4) or passes < 1 or (passes > 1 and waves != 4):
        raise ValueError((waves, passes))
    floor = 22 if passes > 1 else 17
    if not floor <= sr <= 32:
        raise ValueError((sr, waves, passes))
    n = slots(waves, passes)
    # the targets of this (waves, passes): strips of 32 rows decide both
    first = {1: first_strip_target(), 2: 32 * 128 + 1, 4: 32 * 256 + 1}[waves] if passes == 1 else 32 * 512 * (passes - 1) + 1
    lo = first if sr == floor else n * (sr - 1) + 1
    return lo, n * sr


def seam_strips(waves, passes=1):
    """The strips at whose first row something changes hands, sorted."""
    nl = 64 * waves
    s = {0, 1, 63, 64, nl - 1, nl, nl + 63, nl + 64, 2 * nl - 1}
    if passes > 1:
        for p in range(1, passes):
            s |= {2 * nl * p - 1, 2 * nl * p}
        s.add(2 * nl * passes - 1)
    return sorted(g for g in s if 0 <= g < slots(waves, passes))


def row_tl_strips(waves, passes=1):
    """... and the owners the row-tl family visits: those, and lane 0 and lane 63 of every wave in either half"""
    s = set(seam_strips(waves, passes))
    for half in (0, 1):
        for w in range(waves):
            s |= {64 * waves * half + 64 * w, 64 * waves * half + 64 * w + 63}
    return sorted(s)


def owner(g, waves):
    """(pass, half, wave, lane) of strip g"""
    nl = 64 * waves
    return g // (2 * nl), g // nl % 2, g % nl // 64, g % 64


def _rand(rng, n):
    return _ALPHA[rng.integers(0, 4, int(n))]


def _noisy(rng, seq, rate=NOISE):
    """substitutions (always to another base) at the given rate; pieces shorter than 24 bases stay as they are"""
    out = np.array(seq, np.uint8)
    if len(out) < 24:
        return out
    for x in np.nonzero(rng.random(len(out)) < rate)[0]:
        out[x] = _ALPHA[(int(np.nonzero(_ALPHA == out[x])[0][0]) + int(rng.integers(1, 4))) % 4]
    return out


def _unrelated(rng, n, near):
    """n bases of which none equals the base of ``near`` at the same place (cyclically): no accidental diagonal through them"""
    if n <= 0:
        return np.zeros(0, np.uint8)
    near = np.asarray(near, np.uint8)
    ref = near[np.arange(n) % len(near)] if len(near) else np.full(n, ord("A"), np.uint8)
    code = np.searchsorted(_ALPHA, ref)
    return _ALPHA[(code + rng.integers(1, 4, n)) % 4]


def _b(a):
    return bytes(np.asarray(a, np.uint8))


def ck_column(sr, b):
    """The checkpoint column of the band that holds row b + 1 in the query's first 160 columns, and where a 20-column I run has to
    start to span it with flanks that outweigh it: (column, columns in front of the run).  j = 128 cc - 4 K band."""
    k = bands_k(sr)
    j = (-CPS * k * (b // (sr * k))) % CK_COLS or CK_COLS
    if j >= 24:
        return j, j - 10
    return j + CK_COLS, j + CK_COLS - 17


def anchor(sr, waves, passes, rng):
    hi = height_interval(sr, waves, passes)[1]
    t = _rand(rng, hi)
    q = _noisy(rng, t[hi - 150:hi - 20])
    return Case(_b(t), _b(q), SOFTCLIP, Intent("anchor", hi, strip=(hi - 1) // sr))


def row_tl_case(sr, g, r, rng, last_row=True):
    """Row tl = sr g + r + 1 on register row r of strip g, the query a noisy copy of the target's tail.  last_row: nine more query
    bases than the tail has, so that the maximum is in the last row with seg > 0 -- the register row the kernel picks for row tl
    decides the result; else nine unrelated bases in front, so that the maximum is in the last column (family col_tl)."""
    tl = sr * g + r + 1
    ql = QL_CYCLE[r % len(QL_CYCLE)]
    t = _rand(rng, tl)
    c = min(ql - 9, tl)
    tail = _noisy(rng, t[tl - c:])
    front = _unrelated(rng, ql - 9 - c, t)
    if last_row:
        q = np.concatenate([front, tail, _unrelated(rng, 9, t[::-1])])
    else:
        q = np.concatenate([_unrelated(rng, 9, t), front, tail])
    return _b(t), _b(q), Intent("row_tl" if last_row else "col_tl", tl, None, r, g)


def diag_case(sr, b, hi, rng, ql=130):
    tl = min(hi, b + ql // 2 + 7)
    t = _rand(rng, tl)
    lo = max(0, b - ql // 2)
    q = _noisy(rng, t[lo:min(tl, lo + ql)])
    return _b(t), _b(q), Intent("diag", b, strip=b // sr)


def del_case(sr, b, hi, rng, ql=128):
    """the target carries sr + 5 bases the query does not, centred on the boundary below row b"""
    x = sr + 5
    x0 = b - x // 2                  # 0-based index of the first extra base
    s = _rand(rng, ql)
    h = min(ql // 2, x0)
    right = s[h:h + max(0, min(ql - h, hi - (x0 + x)))]
    pad = _rand(rng, max(0, min(7, hi - (x0 + x + len(right)))))
    t = np.concatenate([_rand(rng, x0 - h), s[:h], _unrelated(rng, x, right if len(right) else s), right, pad])
    q = np.concatenate([s[:h], right])
    return _b(t), _b(q), Intent("del", b, strip=b // sr)


def ins_case(sr, b, hi, rng, col, lead, family, ql=MAX_QL):
    """the query carries 20 bases the target does not, behind the base aligned to row b + 1 (the first row of the strip below the
    boundary): columns lead + 1 .. lead + 20, of which ``col`` is the one the case is about"""
    assert lead < col <= lead + 20
    right_n = min(ql - lead - 20, hi - (b + 1))
    tl = min(hi, b + 1 + right_n + 7)
    t = _rand(rng, tl)
    own = min(lead, b + 1)
    left = np.concatenate([_unrelated(rng, lead - own, t), t[b + 1 - own:b + 1]])
    right = t[b + 1:b + 1 + right_n]
    ins = _unrelated(rng, 20, right)
    if ins[-1] == left[-1]:          # (the run is not to slide to the left either)
        ins[-1] = _ALPHA[(int(np.searchsorted(_ALPHA, ins[-1])) + 1) % 4]
    q = np.concatenate([left, ins, right])
    return _b(t), _b(q), Intent(family, b, col, strip=b // sr)


def crossers(sr, b, hi, rng):
    """the four pairs of one boundary row b"""
    out = [diag_case(sr, b, hi, rng), del_case(sr, b, hi, rng)]
    # any 20 columns hold a multiple of 16.  (Beyond BORDER_REACH a longer piece in front of the run: under INDEL, which pays for all
    # the rows above the window anyway, 56 bases score as much scattered over those rows in pieces of five as in one piece and a gap.)
    lead = min(104 if b > BORDER_REACH else 56, b + 1)
    out.append(ins_case(sr, b, hi, rng, (lead + 16) // 16 * 16, lead, "ins16"))
    col, lead = ck_column(sr, b)
    out.append(ins_case(sr, b, hi, rng, col, lead, "insck"))
    return out


def boundary_rows(sr, waves, passes=1):
    """b = sr g for every seam strip g > 0, and the band boundary sr K m nearest to each"""
    hi, k = height_interval(sr, waves, passes)[1], bands_k(sr)
    rows = set()
    for g in seam_strips(waves, passes):
        if g == 0:
            continue
        rows.add(sr * g)
        m = max(1, (g + k // 2) // k)
        while sr * k * m >= hi:
            m -= 1
        rows.add(sr * k * m)
    return sorted(rows)


def strategy_of(k, intent):
    """The strategies rotate with the case index, a step further every fourth case so that a family of every fourth case meets all
    of them.  INDEL and LEADING_INDEL charge the path 11 a row for the rows above it: a window more than BORDER_REACH rows down is
    beyond what 160 query bases can pay, the best score of the last column is then some scattered alignment at the top and neither
    the maximum (both) nor the path (LEADING_INDEL starts there; INDEL starts at the corner and does cross the seam) is where the
    case wants it.  There a path case takes INDEL for LEADING_INDEL -- the fill kernels do not tell the two apart -- and a row-tl
    case the unbordered strategy of the same parity -- as it does where the target is shorter than the query, whose leading bases the
    border charges for in the same way."""
    s = STRATEGIES[(k + k // 4) % 4]
    if intent.family in ("row_tl", "col_tl"):
        if intent.row > BORDER_REACH or intent.row < MAX_QL:
            s = {INDEL: SOFTCLIP, LEADING_INDEL: IGNORE}.get(s, s)
    elif intent.row > BORDER_REACH and s == LEADING_INDEL:
        s = INDEL
    return s


def _with_strategies(triples):
    return [Case(t, q, strategy_of(k, intent), intent) for k, (t, q, intent) in enumerate(triples)]


def cases(sr, waves, passes, rng):
    """Every family at one height: a list of Case(target, query, strategy, intent), the anchor first."""
    hi = height_interval(sr, waves, passes)[1]
    gs = row_tl_strips(waves, passes)
    # even r: the maximum in the last row, odd r: in the last column ...
    out = [row_tl_case(sr, gs[r % len(gs)], r, rng, last_row=r % 2 == 0) for r in range(sr)]
    # ... and the odd register rows in the last row's form as well, in other strips: only that form tells which register row the
    # kernel took for row tl (at the corner of the matrix the last column wins the tie whatever the last row holds)
    out += [row_tl_case(sr, gs[(r + len(gs) // 2) % len(gs)], r, rng) for r in range(1, sr, 2)]
    # (the owners beyond the residues, so that every one of them holds row tl once)
    out += [row_tl_case(sr, gs[r % len(gs)], r % sr, rng) for r in range(sr, len(gs))]
    rows = boundary_rows(sr, waves, passes)
    for b in rows:
        out += crossers(sr, b, hi, rng)
    g = seam_strips(waves, passes)[-1]
    for ql in TINY_QL:
        t = _rand(rng, sr * g + 1)
        out.append((_b(t), _b(t[len(t) - ql:]), Intent("tiny", sr * g + 1, ql, 0, g)))
    # bytes: one vertical-run pair, with letters the 2-bit codes cannot hold
    b = sr * min(64 * waves, slots(waves, passes) - 1)
    t, q, _ = del_case(sr, b, hi, rng)
    x0 = b - (sr + 5) // 2
    tn = bytearray(t)
    tn[x0 - 20] = ord("N")
    qn = bytearray(q)
    qn[10] = ord("N")
    qn[30:34] = bytes(qn[30:34]).lower()
    tr, qr = bytearray(t), bytearray(q)
    h = min(64, x0)
    tr[x0 - 40:x0 - 36] = b"RYKM"
    qr[h - 40:h - 36] = b"RYKM"
    out += [(bytes(tn), q, Intent("bytes_t", b, strip=b // sr)), (t, bytes(qn), Intent("bytes_q", b, strip=b // sr)),
            (bytes(tr), bytes(qr), Intent("bytes_both", b, strip=b // sr))]
    return [anchor(sr, waves, passes, rng)] + _with_strategies(out)


def pass_cases(sr, passes, rng):
    """Several passes (four waves): the crossers of every pass seam (row 512 sr p), row tl in the first strip of the second pass and
    in the last strip of it at four register rows each, and the anchor."""
    hi = height_interval(sr, 4, passes)[1]
    out = []
    for p in range(1, passes):
        out += crossers(sr, 512 * sr * p, hi, rng)
    for g in (512, 1023):
        for r in (0, 1, sr - 2, sr - 1):
            out.append(row_tl_case(sr, g, r, rng))
    return [anchor(sr, 4, passes, rng)] + _with_strategies(out)


def rng_for(sr, waves, passes=1, pass_seams=False):
    """the generator of one height's cases: the CPU test that judges the cases and the GPU test that runs them build the same ones"""
    return np.random.default_rng(77 * sr + passes if pass_seams else 1000 * sr + 10 * waves + passes)


def batches(cs):
    """{strategy: [case index]}: the cases of one strategy together with the anchor (case 0), whose target is the batch's longest"""
    by = {}
    for k, c in enumerate(cs):
        if k:
            by.setdefault(c.strategy, [0]).append(k)
    return by


_CIGAR = re.compile(r"(\d+)([MIDS])")


def path_rows_ops(offset, cigar, tl, ql):
    """What a CIGAR says about the path: ({b: (op, run length)} for every boundary below row b the path crosses -- M or D --,
    [(row, first column, last column)] of every I run), rows and columns counted from 1."""
    i, j = int(offset), 0
    cross, runs = {}, []
    for n, op in _CIGAR.findall(cigar):
        n = int(n)
        if op == "S":
            j += n
        elif op == "I":
            runs.append((i, j + 1, j + n))
            j += n
        else:
            for b in range(i, i + n):
                cross[b] = (op, n)
            i += n
            if op == "M":
                j += n
    assert j == ql, (offset, cigar, tl, ql)   # (IGNORE stretches the first and last element beyond the target: rows outside 1 .. tl)
    return cross, runs


def intent_met(case, offset, cigar, score, sr):
    """Does the oracle's answer do what the case was built for?  (None: the family promises nothing about the path.)"""
    it, tl, ql = case.intent, len(case.target), len(case.query)
    if it.family in ("anchor", "tiny"):
        return None
    if it.family in ("row_tl", "col_tl"):
        _, _, _, max_t, max_q, seg = (int(x) for x in score)
        return (max_t == tl and seg > 0) if it.family == "row_tl" else (max_q == ql and seg == 0)
    cross, runs = path_rows_ops(offset, cigar, tl, ql)
    if it.family == "diag":
        return cross.get(it.row, ("", 0))[0] == "M"
    if it.family in ("del", "bytes_t", "bytes_q", "bytes_both"):
        op, n = cross.get(it.row, ("", 0))
        return op == "D" and n >= sr
    return any(last - first + 1 >= 16 and first <= it.col <= last for _, first, last in runs)
