"""Inputs that put the workgroup kernels (sw_dp_coop.hip: sw_dp_coop_kernel, 64 rows per wave in int32, and sw_dp_coop16_kernel,
128 rows per wave in packed int16) on their own seams at a CHOSEN number of waves per pair.

W waves run the stripes of one pair as a pipeline: stripe k belongs to wave k mod W, the carry of its last row goes to the next wave
through an LDS ring of 256 columns and -- from the last wave back to wave 0 -- through a row in HBM whose columns carry a 16-bit tag
of the round and H - E' in 16 bits.  seam_rows() names the rows after which the carry changes hands, tl_values() / ql_values() the
lengths at which the stripe count, the owner of row tl, the 32-step groups, the lean / edge split, the ring lap and the sequence
numbers per stripe step, and cases() builds small pairs whose paths cross exactly those rows: on a diagonal, in a deletion run that
ends on, starts behind or straddles the seam, in an insertion run on the row in front of or behind it; pairs whose last column ties
across waves and rounds; gap penalties at the bound of the 16-bit H - E' field.  Every batch holds the anchor, a target of at least
R W rows, because the planner lowers W to the stripe count of the batch's longest target (sw_capi.cpp: plan_batch_as).

A form is 32 (sw_dp_coop_kernel) or 16 (sw_dp_coop16_kernel).  The builders judge their own pairs with the CPU oracle and draw again,
from the same generator, until the oracle's path does what the case is for; tests/test_coop_cases.py checks that once more from the
outside, tests/test_gpu_coop_seams.py runs the cases."""
import functools
import re
from collections import namedtuple

import numpy as np

SOFTCLIP, INDEL, LEADING_INDEL, IGNORE = 1, 2, 4, 8
STRATEGIES = (SOFTCLIP, INDEL, LEADING_INDEL, IGNORE)
GATK = (200, -150, 260, 11)
TIE_PARAMS = ((1, -1, 1, 1), (5, -4, 10, 1))
FIELD_PARAMS = ((200, -150, 65535, 0), (200, -150, 65535, 11), (5, -3, 300, 300))   # o - e = 65535, 65524 and 0
FIELD_REFUSED = ((200, -150, 65536, 0), (5, -3, 2, 9))                              # sw_capi.cpp: gopen < 65536 && gopen >= gext
FORMS = (32, 16)
WAVES = (2, 4, 16)
R = {32: 64, 16: 128}          # sw_dp_coop.hip: nstripes = (tl + 63) >> 6; nds = (tl + 127) >> 7
RING_COLS, AHEAD = 256, 40     # sw_dp_coop.hip: constexpr int RING_COLS = 256, AHEAD = 40
MAIN_LO = {32: 64, 16: 128}    # sw_dp_coop.hip: main_lo = 64 (coop32_body), 128 (coop16_body)
MAX_QL = 600
NOISE = 0.03
DEL_RUNS = (1, 2, 63, 64, 65)  # ... and R + 1
MIN_FLANK = 24                 # bases in front of a deletion run: what lies nearer to row 1 cannot be built

Case = namedtuple("Case", "target query params strategy intent")
# family: anchor | diag | del | ins | row_tl | col_ql | ties | gap_field | gap_refused | mixed
# row: the seam row b (diag, del, ins, gap_field) or tl; col: the column an I run is to contain (ins), 1 where the last column is to
# tie across waves (ties), 2 where the last row is to decide (ties); first, last: the rows a D run is to cover, or the row of an I run
Intent = namedtuple("Intent", "family row col first last")
Intent.__new__.__defaults__ = (None, None, None, None)

_ALPHA = np.frombuffer(b"ACGT", np.uint8)


# ---- the kernel's geometry, restated

def sps32(ql):
    """steps per 64-row stripe (sw_device.h: coop_sps_for)"""
    return (ql + 95) & ~31


def sps16(ql):
    """steps per 128-row double stripe (sw_device.h: coop16_sps_for)"""
    return (ql + 160) & ~31


def sps(form, ql):
    return sps32(ql) if form == 32 else sps16(ql)


def seq_numbers(form, ql):
    """S, the sequence numbers a stripe takes on its ring (sw_dp_coop.hip: S = (sps + 64 + RING_MASK) & ~RING_MASK)"""
    return (sps(form, ql) + 64 + 255) & ~255


def main_hi(ql):
    """sw_dp_coop.hip: main_hi = ql & ~31 -- the groups inside [main_lo, main_hi) touch no edge"""
    return ql & ~31


def wrap_tag(k, W):
    """sw_dp_coop.hip: wrap_tag -- the tag of the HBM row's columns that stripe k consumes"""
    return (k // W & 0x7fff) + 1


def coop16_below(match, mismatch, gopen, gext):
    """sw_dp_coop.hip: coop16_below"""
    return 34 * (gopen - gext) + 2 * (match + gopen + gext) + (gopen - gext) + abs(mismatch + 2 * gext) + 64


def coop16_above(match, gopen, gext):
    """sw_dp_coop.hip: coop16_above"""
    return 34 * (match + gopen + gext) + gopen + (match + 2 * gext) + 64


def coop16_possible(match, mismatch, gopen, gext):
    """sw_dp_coop.hip: coop16_possible"""
    if match <= 0 or mismatch > match or gext < 0 or gopen < gext or match > 4000 or mismatch < -4000 or gopen > 4000 or gext > 4000:
        return False
    return coop16_below(match, mismatch, gopen, gext) + coop16_above(match, gopen, gext) <= 60000


def coop16_worthwhile(match, mismatch, gopen, gext):
    """sw_dp_coop.hip: coop16_worthwhile"""
    if not coop16_possible(match, mismatch, gopen, gext):
        return False
    margin = coop16_below(match, mismatch, gopen, gext) + coop16_above(match, gopen, gext)
    return 128 * (match + 2 * gext) + 2 * (gopen - gext) + margin <= 64000


def stripes(form, tl):
    return (tl + R[form] - 1) // R[form]


def owner(form, W, row):
    """(round, wave) of the stripe that holds target row ``row``"""
    k = (row - 1) // R[form]
    return k // W, k % W


def hbm_rows(form, W):
    """the rows after which the carry goes through the pair's HBM row: R W r for r = 1, 2 (tags 2 and 3 come in)"""
    return [R[form] * W * r for r in (1, 2)]


def seam_rows(form, W):
    """The rows b after which the carry changes hands: R k through a ring, R W r through the HBM row."""
    return sorted({R[form] * k for k in range(1, W)} | set(hbm_rows(form, W)))


def tl_values(form, W):
    """b - 1, b, b + 1 around the rows that make the stripe count 1, W - 1, W, W + 1, 2 W and 2 W + 1; for the 16-bit form b + 2 as
    well, so that tl mod 128 is 127, 0, 1 and 2: row tl in lane 63 low, lane 63 high, lane 0 low and lane 0 high."""
    out = set()
    for n in (1, W - 1, W, W + 1, 2 * W, 2 * W + 1):
        b = R[form] * n
        out |= {b - 1, b, b + 1} | ({b + 2} if form == 16 else set())
    return sorted(out)


def ql_values(form):
    """The query lengths at the kernel's column seams, up to MAX_QL (and 513)."""
    out = {1, 2, 3}
    for g in (32, 64, 96, 128, 160):                   # the 32-step groups; main_lo; main_hi = ql & ~31
        out |= {g - 1, g, g + 1}
    for ql in range(2, MAX_QL + 1):                    # where S steps
        if seq_numbers(form, ql) != seq_numbers(form, ql - 1):
            out |= {ql - 1, ql}
    for lap in (RING_COLS, 2 * RING_COLS):             # the ring's lap
        out |= {lap - 1, lap, lap + 1}
    return sorted(out)


# ---- sequences

def _rand(rng, n):
    return _ALPHA[rng.integers(0, 4, int(n))]


def _other(rng, base):
    return _ALPHA[(int(np.searchsorted(_ALPHA, base)) + int(rng.integers(1, 4))) % 4]


def _noisy(rng, seq, rate=NOISE):
    """substitutions (always to another base) at the given rate; pieces shorter than 24 bases stay as they are"""
    out = np.array(seq, np.uint8)
    if len(out) < 24:
        return out
    for x in np.nonzero(rng.random(len(out)) < rate)[0]:
        out[x] = _other(rng, out[x])
    return out


def _unrelated(rng, n, near):
    """n bases of which none equals the base of ``near`` at the same place (cyclically): no accidental diagonal through them"""
    if n <= 0:
        return np.zeros(0, np.uint8)
    near = np.asarray(near, np.uint8)
    ref = near[np.arange(n) % len(near)] if len(near) else np.full(n, ord("A"), np.uint8)
    return _ALPHA[(np.searchsorted(_ALPHA, ref) + rng.integers(1, 4, n)) % 4]


def _b(a):
    return bytes(np.asarray(a, np.uint8))


def path_ql(b):
    """The query length of a path case at seam row b: INDEL and LEADING_INDEL charge 11 a row for the rows above the window, the
    window has to pay for them with 200 a base and a half to spare."""
    return 192 if 11 * b + 260 < 100 * 192 else MAX_QL


# ---- what a CIGAR says about the path

_CIGAR = re.compile(r"(\d+)([MIDS])")


def path_rows_ops(offset, cigar, ql):
    """({row: (op, run length)} for every target row the path consumes -- M or D --, [(row, first column, last column)] of every I
    run: the row is the last one consumed in front of it), rows and columns counted from 1."""
    i, j = int(offset), 0
    rows, runs = {}, []
    for n, op in _CIGAR.findall(cigar):
        n = int(n)
        if op == "S":
            j += n
        elif op == "I":
            runs.append((i, j + 1, j + n))
            j += n
        else:
            for r in range(i + 1, i + n + 1):
                rows[r] = (op, n)
            i += n
            if op == "M":
                j += n
    assert j == ql, (offset, cigar, ql)
    return rows, runs


def _oracle(case, want_btr=False):
    import oracle_lib as ol

    return ol.oracle_align(case.target, case.query, case.params, case.strategy, want_btr=want_btr)


def tie_rows(case, form, W):
    """(the rows among the last rows of every stripe and row tl at which the last column attains its maximum, the oracle's result):
    H[i][ql] depends on the rows up to i alone, so row x attains the maximum iff the pair cut to x target rows reports it in row x."""
    full = _oracle(case)
    best, tl = full["score"][0], len(case.target)
    out = []
    for x in sorted({min(tl, R[form] * k) for k in range(1, stripes(form, tl) + 1)}):
        s = _oracle(case._replace(target=case.target[:x]))["score"]
        if s[0] == best and s[1] == x:
            out.append(x)
    return out, full


def intent_met(case, form, W):
    """Does the oracle's answer do what the case was built for?  (None: the family promises nothing about the path.)"""
    it = case.intent
    if it.family in ("anchor", "row_tl", "col_ql", "mixed", "gap_refused"):
        return None
    if it.family == "ties":
        if it.col == 1:
            rows, _ = tie_rows(case, form, W)
            return len({owner(form, W, x)[1] for x in rows}) >= 2 and len({owner(form, W, x)[0] for x in rows}) >= 2
        if it.col == 2:
            mqe, _, mx, max_t, _, seg = _oracle(case)["score"]
            return max_t == len(case.target) and mx == mqe and seg > 0
        return None
    o = _oracle(case)
    rows, runs = path_rows_ops(o["offset"], o["cigar"], len(case.query))
    if it.family == "diag":
        return rows.get(it.row, ("", 0))[0] == "M" and rows.get(it.row + 1, ("", 0))[0] == "M"
    if it.family in ("del", "gap_field"):
        n = it.last - it.first + 1
        return (rows.get(it.first) == ("D", n) and rows.get(it.last) == ("D", n) and rows.get(it.first - 1, ("M", 0))[0] == "M"
                and rows.get(it.last + 1, ("", 0))[0] == "M")
    if it.family == "ins":
        return any(i == it.first and last - first + 1 >= 16 and first <= it.col <= last for i, first, last in runs)
    raise ValueError(it.family)


def _draw(build, form, W, tries=40):
    """the first pair of ``build()`` that the oracle takes the way the case wants"""
    for _ in range(tries):
        case = build()
        if intent_met(case, form, W) is not False:
            return case
    raise AssertionError(("no draw does what the case is for", case.intent, case.params, case.strategy))


# ---- the families

def anchor(form, W, rng):
    tl = R[form] * W + 37
    t = _rand(rng, tl)
    return Case(_b(t), _b(_noisy(rng, t[max(0, tl - 170):tl - 20])), GATK, SOFTCLIP, Intent("anchor", tl))


def diag_case(form, b, strategy, rng):
    """a noisy copy whose diagonal crosses row b, with a mismatch on row b and one on row b + 1"""
    ql = path_ql(b)
    lo = max(0, b - ql // 2)
    t = _rand(rng, lo + ql + 7)
    q = _noisy(rng, t[lo:lo + ql])
    for row in (b, b + 1):
        q[row - 1 - lo] = _other(rng, t[row - 1])
    return Case(_b(t), _b(q), GATK, strategy, Intent("diag", b))


def del_case(form, b, first, n, strategy, rng, params=GATK, family="del", left=None, right=None):
    """the target carries n bases the query does not, rows first .. first + n - 1; left / right: bases in front of and behind them"""
    ql = path_ql(b)
    h = min(ql // 2, first - 1) if left is None else left
    s = _rand(rng, h + (ql - h if right is None else right))
    x = _unrelated(rng, n, s[h:])    # (x[0] != s[h]: the run cannot slide downwards)
    bad = {int(s[h - 1]), int(s[h])} if n == 1 else {int(s[h - 1])}
    if int(x[-1]) in bad:            # (... nor upwards)
        x[-1] = next(c for c in _ALPHA if int(c) not in bad)
    t = np.concatenate([_rand(rng, first - 1 - h), s[:h], x, s[h:], _rand(rng, 7)])
    return Case(_b(t), _b(s), params, strategy, Intent(family, b, None, first, first + n - 1))


def del_placements(form, b):
    """(first row, run length) of the deletion runs at seam row b: every length ending exactly on b, starting exactly on b + 1 and
    straddling b -- those whose first row leaves MIN_FLANK rows above it for the query to hold on to."""
    out = []
    for n in sorted(set(DEL_RUNS) | {R[form] + 1}):
        firsts = [b - n + 1, b + 1] + ([b - n // 2 + 1] if n > 1 else [])
        out += [(f, n) for f in firsts if f - 1 >= MIN_FLANK]
    return out


def ins_case(form, b, row, col, strategy, rng):
    """the query carries 20 bases the target does not, behind the base aligned to row ``row``: columns col - 9 .. col + 10"""
    lead = col - 10
    right_n = 70 if 11 * b + 260 < 100 * (lead + 70) else 330
    t = _rand(rng, row + right_n + 7)
    own = min(lead, row)
    left = np.concatenate([_unrelated(rng, lead - own, t), t[row - own:row]])
    right = t[row:row + right_n]
    ins = _unrelated(rng, 20, right)
    if ins[-1] == left[-1]:          # (the run is not to slide to the left either)
        ins[-1] = _ALPHA[(int(np.searchsorted(_ALPHA, ins[-1])) + 1) % 4]
    return Case(_b(t), _b(np.concatenate([left, ins, right])), GATK, strategy, Intent("ins", b, col, row))


def ins_placements(b):
    """(row, column) of the insertion runs at seam row b: on the first row behind the seam -- F opens in the first row a wave
    computes from staged carry -- and on the row in front of it, over a multiple of 32 and over a multiple of 256"""
    return [(b + 1, 96), (b + 1, 256), (b, 96), (b, 256)]


def length_case(tl, ql, last_row, strategy, rng, family=None):
    """tl x ql with the query a noisy copy of the target's tail.  last_row: nine more query bases than the tail has, the maximum is
    in the last row; else nine unrelated bases in front, the maximum is in the last column."""
    t = _rand(rng, tl)
    if ql < 33:
        q = t[tl - ql:] if ql <= tl else np.concatenate([_unrelated(rng, ql - tl, t), t])
    else:
        c = min(ql - 9, tl)
        tail, front, nine = _noisy(rng, t[tl - c:]), _unrelated(rng, ql - 9 - c, t), _unrelated(rng, 9, t[::-1])
        q = np.concatenate([front, tail, nine] if last_row else [nine, front, tail])
    return Case(_b(t), _b(q), GATK, strategy, Intent(family or ("row_tl" if last_row else "col_ql"), tl))


def length_cases(form, W, rng):
    """every tl_values x a cycle of ql_values, every strategy in turn; tl = 1 against ql = 513; 2 W + 1 stripes and a row against
    the tiny queries"""
    tls, qls = tl_values(form, W), ql_values(form)
    per = -(-len(qls) // len(tls))
    pairs = [(tl, qls[(per * k + m) % len(qls)]) for k, tl in enumerate(tls) for m in range(per)]
    pairs += [(1, 513)] + [(2 * W * R[form] + 1, ql) for ql in (1, 2, 3)]
    return [length_case(tl, ql, k % 2 == 0, STRATEGIES[(k + k // 4) % 4], rng) for k, (tl, ql) in enumerate(pairs)]


def tie_cases(form, W, rng):
    """A^n against A^m, (AC)^n against (CA)^m, A^n against random AT, the target over 2 W + 1 stripes: without a border the last
    column of the first two holds its maximum in every row from m on (every second one): it ties between rows of every wave and of
    three rounds -- the larger row has to win (sw.cpp:100-104).  Where the target is shorter than MAX_QL, A^n against A^MAX_QL: the
    last row ties with the last column and wins, being closer to the diagonal (sw.cpp:116-127)."""
    tl = 2 * W * R[form] + R[form] // 2 + 3
    pairs = [(b"A" * tl, b"A" * 97), ((b"AC" * tl)[:tl], b"CA" * 48 + b"C"), (b"A" * tl, _b(np.frombuffer(b"AT", np.uint8)[rng.integers(0, 2, 150)]))]
    out = []
    for params in TIE_PARAMS:
        if form == 16 and not coop16_possible(*params):
            continue
        for n, (t, q) in enumerate(pairs):   # (the third pattern ties inside the matrix, between gap lengths and placements)
            out += [Case(t, q, params, s, Intent("ties", tl, 1 if n < 2 and s in (SOFTCLIP, IGNORE) else 0)) for s in STRATEGIES]
        if tl < MAX_QL:
            out += [Case(b"A" * tl, b"A" * MAX_QL, params, s, Intent("ties", tl, 2)) for s in (SOFTCLIP, IGNORE)]
    return out


def gap_field_cases(W, rng):
    """int32 form, W <= 4: deletion runs across the first HBM row under gap penalties at the bounds of the row's 16-bit H - E'
    field (0 <= H - E' <= o - e), the pair within 2000 bases.  A gap of 65535 is worth 328 matches: only a path that has to pay for
    one anyway takes it, so the strategies are the two that charge the leading rows, and the target begins with the left flank."""
    b = R[32] * W
    out = []
    for params in FIELD_PARAMS + FIELD_REFUSED:
        runs = [(b - 32, 65), (b - 63, 64), (b + 1, 63)] if params[2] > 60000 else [(b, 2), (b, 1), (b + 1, 1)]
        for k, (first, n) in enumerate(runs):
            fam = "gap_field" if params in FIELD_PARAMS else "gap_refused"
            out.append(_draw(lambda: del_case(32, b, first, n, (INDEL, LEADING_INDEL)[k % 2], rng, params, fam, left=first - 1, right=340), 32, W))
            assert len(out[-1].target) + len(out[-1].query) <= 2000
    return out


def mixed_cases(form, W, rng):
    """pairs of 1, 2, W - 1, W, W + 1, 2 W and 2 W + 1 stripes, two of each, the queries drawn across ql_values, in shuffled order:
    one batch per strategy"""
    qls = ql_values(form)
    out = []
    for s in STRATEGIES:
        ns = [n for n in (1, 2, W - 1, W, W + 1, 2 * W, 2 * W + 1) for _ in (0, 1)]
        batch = [length_case(R[form] * (n - 1) + int(rng.integers(1, R[form] + 1)), int(qls[rng.integers(0, len(qls))]), k % 2 == 0, s, rng, "mixed")
                 for k, n in enumerate(ns)]
        out += [batch[k] for k in rng.permutation(len(batch))]
    return out


def rng_for(form, W):
    """the generator of one form's cases at W waves: the CPU test that judges them and the GPU test that runs them build the same"""
    return np.random.default_rng(100 * form + W)


def cases(form, W, rng):
    """Every family of one form at W waves: a list of Case(target, query, params, strategy, intent), the anchor first.  The path
    families cross every seam row at W = 2 and 4, the two HBM rows alone at W = 16."""
    out = [anchor(form, W, rng)]
    k = 0
    for b in (seam_rows(form, W) if W <= 4 else hbm_rows(form, W)):
        todo = [lambda s, b=b: diag_case(form, b, s, rng)]
        todo += [lambda s, b=b, f=f, n=n: del_case(form, b, f, n, s, rng) for f, n in del_placements(form, b)]
        # (a query that begins with bases from nowhere -- the run lies further right than the seam lies down -- cannot start in the
        # corner: those take the strategies without a border)
        todo += [lambda s, b=b, r=r, c=c: ins_case(form, b, r, c, s if c - 10 <= r else (SOFTCLIP, IGNORE)[s in (LEADING_INDEL, IGNORE)], rng)
                 for r, c in ins_placements(b)]
        for build in todo:
            out.append(_draw(functools.partial(build, STRATEGIES[(k + k // 4) % 4]), form, W))
            k += 1
    out += length_cases(form, W, rng)
    out += tie_cases(form, W, rng)
    if form == 32 and W <= 4:
        out += gap_field_cases(W, rng)
    out += mixed_cases(form, W, rng)
    return out


@functools.lru_cache(maxsize=None)
def cases_for(form, W):
    """cases(form, W, rng_for(form, W)), built once"""
    return tuple(cases(form, W, rng_for(form, W)))


def batches(cs):
    """{(params, strategy, 'mixed' or ''): [case index]}: the cases of one parameter set and strategy together with the anchor
    (case 0), which takes the batch's parameters and strategy; the mixed family keeps its own batches and its order"""
    by = {}
    for k, c in enumerate(cs):
        if k:
            by.setdefault((c.params, c.strategy, "mixed" if c.intent.family == "mixed" else ""), [0]).append(k)
    return by
