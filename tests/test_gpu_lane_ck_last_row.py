"""sw_dp16_lane_ck_kernel, the last row: the last strip of pass 1 keeps the running best of H[tl][1 .. ql] (sw.cpp:116-127: the
largest score, then the smallest |tl - j|, then the earlier column) as one packed key per lane half instead of storing the row and
scanning it afterwards, and reads the corner H[tl][ql] off its registers.  The shapes are the smallest at which that can go wrong:
partial last strips (tl = 113, 120, 127: the row is row 16, 23, 30 of the strip) and full ones, one to three columns after the
last group of four, tl < ql (|tl - j| falls and then rises along the row), an odd pair count, rows full of ties, scores at the
lower and upper ends of the 16-bit range, every build of the column loop, and launches that alternate on one region.  Everything
is compared with the oracle: offsets, all six score fields, CIGAR strings.

The tie classes are not taken on trust: a plain DP of the recurrence (sw.cpp:45-127) computes H[tl][.] and H[.][ql] of every pair of
the tie batch on the CPU, and the test asserts that each class it is meant to cover is present."""
import numpy as np
import pytest

import oracle_lib as ol
import range_guards as rg
from mgl_amd import smithwaterman as sw

pytestmark = pytest.mark.gpu

GATK = (200, -150, 260, 11)
OTHER = (25, -50, 110, 6)  # no folded diagonal: the unfolded kernels
UNIT = (1, -1, 1, 1)
SMALL = (5, -4, 10, 1)
LANE16_CK = 7
# (tl, ql): rows 31, 31, 31, 16, 23, 30, 31 of the last strip hold row tl; 1, 3, 2, 1, 1, 2, 3 columns behind the last group of four
GEOMETRIES = [(64, 97), (64, 99), (96, 70), (113, 33), (120, 97), (127, 70), (128, 99)]


def _rand(rng, alpha, n):
    return alpha[rng.integers(0, len(alpha), n)]


def _batch(tl, ql, seed, n=385):
    """Reads cut from the target at every kind of place -- ending at the target's end (the row's maximum at j = ql), starting at
    its start with a foreign tail (at j = tl where tl <= ql, else inside), in the middle with an indel --, unrelated pairs,
    all-mismatch pairs (the lowest scores the borders allow), homopolymers and two-letter pairs (ties).  An odd count."""
    rng = np.random.default_rng(seed)
    acgt, ac = np.frombuffer(b"ACGT", np.uint8), np.frombuffer(b"AC", np.uint8)
    ts, qs = [], []
    for k in range(n):
        kind = k % 8
        alpha = ac if k % 16 >= 8 else acgt
        t = _rand(rng, alpha, tl)
        if kind == 0:  # the read ends where the target ends
            q = np.concatenate([_rand(rng, alpha, ql), t])[-ql:]
        elif kind == 1:  # the read starts where the target starts
            q = np.concatenate([t, _rand(rng, alpha, ql)])[:ql]
        elif kind == 2:  # somewhere inside, one indel
            s = int(rng.integers(0, max(1, tl // 2)))
            src = np.concatenate([t[s:], _rand(rng, alpha, ql + 8)])
            at, g = int(rng.integers(1, ql)), int(rng.integers(1, 6))
            q = (np.concatenate([src[:at], src[at + g:]]) if k % 3 else np.concatenate([src[:at], _rand(rng, alpha, g), src[at:]]))[:ql]
        elif kind == 3:
            q = _rand(rng, alpha, ql)
        elif kind == 4:  # nothing matches
            t = np.full(tl, ord("A"), np.uint8)
            q = np.full(ql, ord("C"), np.uint8)
        elif kind == 5:  # homopolymers: H[tl][j] = match * min(tl, j) under SOFTCLIP
            t = np.full(tl, ord("G"), np.uint8)
            q = np.full(ql, ord("G"), np.uint8)
            if k % 3 == 0:
                q[int(rng.integers(0, ql))] = ord("T")
            elif k % 3 == 1 and tl < ql:  # d foreign bases up to column tl: with (1, -1, 1, 1) H[tl][tl - d] = H[tl][tl + d], less in between
                d = 1 + (k // 24) % 3
                q[tl - d:tl] = ord("T")
        elif kind == 6:  # only the read's first base matches, and only the target's last one
            t = np.full(tl, ord("A"), np.uint8)
            t[-1] = ord("C")
            q = np.full(ql, ord("G"), np.uint8)
            q[0] = ord("C")
        else:  # a short period: the same score at many columns
            p = int(rng.integers(2, 6))
            unit = _rand(rng, ac, p)
            t = np.resize(unit, tl)
            q = np.resize(np.roll(unit, int(rng.integers(0, p))), ql)
        ts.append(t.tobytes())
        qs.append(q.tobytes())
    assert len(ts) % 2 == 1
    return ts, qs


def _last_row_and_column(ts, qs, params, indel):
    """H[tl][1 .. ql] and H[1 .. tl][ql] of every pair of a uniform batch: the recurrence of sw.cpp:45-98 over all pairs at once"""
    m, x, o, e = params
    T = np.frombuffer(b"".join(ts), np.uint8).reshape(len(ts), -1)
    Q = np.frombuffer(b"".join(qs), np.uint8).reshape(len(qs), -1)
    n, tl = T.shape
    ql = Q.shape[1]
    border = lambda k: (-o - (k - 1) * e) if (indel and k > 0) else 0
    sc = np.array([[border(j) for j in range(ql + 1)]] * n, np.int64)  # H[i - 1][.]
    E = np.full((n, ql + 1), -o, np.int64) + (sc if indel else 0)
    E[:, 0] = -o
    col = np.zeros((n, tl), np.int64)
    for i in range(1, tl + 1):
        F = np.full(n, -o + border(i), np.int64)
        new = np.empty_like(sc)
        new[:, 0] = border(i)
        sub = np.where(T[:, i - 1:i] == Q, m, x)
        for j in range(1, ql + 1):
            cur = np.maximum(np.maximum(sc[:, j - 1] + sub[:, j - 1], E[:, j]), F)
            E[:, j] = np.maximum(cur - o, E[:, j] - e)
            F = np.maximum(cur - o, F - e)
            new[:, j] = cur
        sc = new
        col[:, i - 1] = sc[:, ql]
    return sc[:, 1:], col


def _tie_classes(row, col, tl, ql):
    """per pair: what decides the last row's scan and the choice between the row and the last column (sw.cpp:100-127)"""
    out = {k: 0 for k in ("single", "several_distances", "mirror_pair", "at_1", "at_ql", "at_tl", "row_ties_column_row_wins", "row_ties_column_column_wins")}
    for r, c in zip(row, col):
        mx = r.max()
        at = np.flatnonzero(r == mx) + 1
        d = np.abs(tl - at)
        win = at[np.lexsort((at, d))[0]]
        mqe = c.max()
        mqe_t = np.flatnonzero(c == mqe)[-1] + 1  # (>=: the last row that reaches it)
        row_wins = mx > mqe or (mx == mqe and abs(tl - win) < abs(mqe_t - ql))
        out["single"] += len(at) == 1 and row_wins
        out["several_distances"] += len(set(d)) > 1 and row_wins
        out["mirror_pair"] += int((d == d.min()).sum() == 2) and row_wins
        out["at_1"] += win == 1 and row_wins
        out["at_ql"] += win == ql and mx >= mqe  # (the corner is in the last column too: max_q = ql whichever of the two wins)
        out["at_tl"] += win == tl and row_wins
        out["row_ties_column_row_wins"] += mx == mqe and row_wins
        out["row_ties_column_column_wins"] += mx == mqe and not row_wins
    return out


@pytest.fixture()
def lane():
    a = sw.MicrosoftSmithWaterman(0)
    a.set_lane_kernel(2)
    yield a
    a.close()


_batches, _want = {}, {}


def _get(tl, ql):
    if (tl, ql) not in _batches:
        _batches[(tl, ql)] = _batch(tl, ql, seed=tl * 1000 + ql)
    return _batches[(tl, ql)]


def _oracle(key, ts, qs, params, strategy):
    k = (key, params, strategy)
    if k not in _want:
        _want[k] = ol.oracle_align_batch(ts, qs, params, strategy, nthreads=8)
    return _want[k]


def _check(res, want, what):
    off, sc, cg = want
    assert (np.asarray(res.offsets) == off).all(), what
    assert (np.asarray(res.scores) == sc).all(), what
    assert list(res.cigars) == list(cg), what


def _run(lane, key, ts, qs, params, strategy, **kw):
    res = lane.align_batch(ts, qs, params, strategy, **kw)
    assert lane.timing().fill_kernel == LANE16_CK, (key, params, strategy)
    _check(res, _oracle(key, ts, qs, params, strategy), (key, params, strategy))


@pytest.mark.parametrize("tl,ql", GEOMETRIES)
def test_geometries(lane, tl, ql):
    """Every overhang strategy (the three that are not SOFTCLIP start their walk at the corner, or use it) with GATK's parameters,
    which fold, and one strategy each with parameters that do not and with the cheap gaps of the tie tests.  The all-mismatch
    pairs under the indel strategies hold the lowest values a last row can."""
    ts, qs = _get(tl, ql)
    for strategy in ol.STRATEGIES:
        _run(lane, (tl, ql), ts, qs, GATK, strategy)
    _run(lane, (tl, ql), ts, qs, OTHER, ol.INDEL)
    _run(lane, (tl, ql), ts, qs, UNIT, ol.SOFTCLIP)


@pytest.mark.parametrize("params", [UNIT, SMALL, GATK], ids=str)
def test_ties_in_the_last_row(lane, params):
    """64 x 97 (tl < ql: columns on either side of tl, the column tl itself) and 96 x 70 (every column left of tl)."""
    ts, qs = _get(64, 97)
    got = _tie_classes(*_last_row_and_column(ts, qs, params, indel=False), 64, 97)
    for k, v in got.items():
        # (two columns at one distance that tie for the maximum with nothing nearer: the batch has them for unit scores; a search
        # over 3 000 two-letter, periodic and homopolymer pairs found none for the other two sets, where a gap and the matches it
        # buys do not cancel)
        assert v > 0 or (k == "mirror_pair" and params != UNIT), (k, got)
    t2, q2 = _get(96, 70)
    got2 = _tie_classes(*_last_row_and_column(t2, q2, params, indel=False), 96, 70)
    for k in ("single", "at_1", "at_ql", "row_ties_column_column_wins") + (("several_distances",) if params == UNIT else ()):
        assert got2[k] > 0, (k, got2)
    for strategy in ol.STRATEGIES:
        _run(lane, (64, 97), ts, qs, params, strategy)
        _run(lane, (96, 70), t2, q2, params, strategy)


def test_range_edge(lane):
    """128 x 99 with the largest match score dp16_range_ok admits beside GATK's other three: the row's frame
    w = stored + (ql - j) e reaches 32767 at a perfect match and the all-mismatch pairs sit at the bottom."""
    tl, ql = 128, 99
    match = max(mm for mm in range(1, 2000) if rg.dp16_range_ok(tl, ql, mm, *GATK[1:]))
    assert not rg.dp16_range_ok(tl, ql, match + 1, *GATK[1:])
    params = (match,) + GATK[1:]
    ts, qs = _get(tl, ql)
    perfect = bytes(np.random.default_rng(1).choice(np.frombuffer(b"ACGT", np.uint8), tl))
    ts, qs = ts + [perfect, perfect], qs + [perfect[-ql:], perfect[:ql]]
    for strategy in ol.STRATEGIES:
        _run(lane, "edge", ts, qs, params, strategy)


@pytest.mark.parametrize("ql", [65536, 65537])
def test_query_at_the_key_limit(lane, ql):
    """A column's preference fills the key's low 16 bits at ql = 65536; a launch with a longer query (the range guard admits any
    length where gext = 0) stores the row and scans it as before.  Three pairs; the maximum early, late, and tied all along."""
    tl, params = 64, (1, -1, 1, 0)
    assert rg.dp16_range_ok(tl, ql, *params)
    rng = np.random.default_rng(ql)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    t = [_rand(rng, acgt, tl) for _ in range(2)] + [np.full(tl, ord("A"), np.uint8)]
    q = [np.concatenate([t[0], _rand(rng, acgt, ql)])[:ql], np.concatenate([_rand(rng, acgt, ql), t[1]])[-ql:], np.full(ql, ord("A"), np.uint8)]
    ts, qs = [x.tobytes() for x in t], [x.tobytes() for x in q]
    for strategy in (ol.SOFTCLIP, ol.INDEL):
        _run(lane, ("long", ql), ts, qs, params, strategy)


def test_other_builds_of_the_loop(lane):
    """2-bit input, ASCII with an N in one target of every wave (the byte-compare twin), and a CIGAR stride that is no multiple of
    four (results lane by lane: the scatter kernels), with parameters that fold and parameters that do not."""
    from mgl_amd import device_batch as db

    tl, ql = 120, 97
    ts, qs = _get(tl, ql)
    tb, qb = db.pack2bit(b"".join(ts)), db.pack2bit(b"".join(qs))
    t_start = np.arange(len(ts), dtype=np.int64) * tl
    q_start = np.arange(len(qs), dtype=np.int64) * ql
    for params in (GATK, OTHER):
        res = lane.align_packed_2bit(tb, tl * len(ts), t_start, None, qb, ql * len(qs), q_start, None, tl, ql, params, ol.INDEL)
        assert lane.timing().fill_kernel == LANE16_CK
        _check(res, _oracle((tl, ql), ts, qs, params, ol.INDEL), "2-bit")
    rng = np.random.default_rng(3)
    tn = list(ts)
    for k in range(5, len(tn), 128):
        t = bytearray(tn[k])
        t[int(rng.integers(0, tl))] = ord("N")
        tn[k] = bytes(t)
    for params in (GATK, OTHER):
        for strategy in (ol.SOFTCLIP, ol.INDEL):
            _run(lane, "with N", tn, qs, params, strategy)
            _run(lane, (tl, ql), ts, qs, params, strategy, cigar_stride=250)
    _run(lane, "with N", tn, qs, GATK, ol.IGNORE, cigar_stride=250)


def test_grouped_launch(monkeypatch):
    """One launch with two geometries, whole waves of each: the strip that holds the last row, its row in that strip and the
    preference order of the columns change from wave to wave."""
    monkeypatch.setenv("MGL_SW_DEBUG_LANE_GROUP_MIN", "128")
    ts, qs = [], []
    for tl, ql in ((100, 97), (64, 99)):
        t1, q1 = _batch(tl, ql, seed=7 * tl + ql, n=641)  # (the library sorts batches of 1 024 pairs and more)
        ts += t1
        qs += q1
    order = np.random.default_rng(11).permutation(len(ts))
    ts, qs = [ts[k] for k in order], [qs[k] for k in order]
    a = sw.MicrosoftSmithWaterman(0)
    a.set_small_kernel(1)  # (a batch this small would go to the one-wave-per-pair kernel)
    try:
        for strategy in (ol.SOFTCLIP, ol.INDEL, ol.LEAD_INDEL):
            res = a.align_batch(ts, qs, GATK, strategy, cigar_stride=256)
            assert a.timing().fill_kernel == LANE16_CK, "the geometries that fill whole waves should take the lane kernel"
            _check(res, _oracle("grouped", ts, qs, GATK, strategy), strategy)
    finally:
        a.close()


def test_the_row_is_not_read(lane, monkeypatch):
    """Two wave slots, so that every wave takes several tiles in its region, and launches of two geometries and parameter sets in
    turn on one context: where the carry row "entering strip `strips`" of one launch used to be lie the rows, checkpoints and
    flags of the other.  Nothing may depend on what is there."""
    monkeypatch.setenv("MGL_SW_DEBUG_LANE_SLOTS", "2")
    a, b = _get(128, 99), _get(64, 97)
    for _ in range(2):
        _run(lane, (128, 99), *a, GATK, ol.INDEL)
        _run(lane, (64, 97), *b, UNIT, ol.SOFTCLIP)
        _run(lane, (128, 99), *a, OTHER, ol.SOFTCLIP)
        _run(lane, (64, 97), *b, GATK, ol.LEAD_INDEL)
