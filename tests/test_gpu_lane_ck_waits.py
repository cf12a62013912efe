"""sw_dp16_lane_ck_kernel, where prologue, column loop, checkpoint and tail of pass 1 meet: the loop reads the carry row and the
query one group of four columns ahead, and the waits for those reads are counted (`s_waitcnt vmcnt(N)`: the group's own stores stay
in flight behind them).  A count that is too large, or a read consumed before its wait, gives right answers whenever memory happens
to be fast -- the proof of the counts is the reading of the disassembly (scripts/lane_ck_waits.py, docs/history.md), not this
file.  What this file pins is every way the pieces can meet: zero, one and two trips of the group loop with every tail (ql = 1 ... 5,
7, 8, 9, 11, 12), the checkpoint's stores inside the loop and in the tail (ql = 32, 33, 36, 37, 64, 65, 68), the bench's ql = 150;
each against a target of one strip that is the last (tl = 32), of a last strip of one row (33, inside a grouped launch: a uniform
launch of that length takes 16-row strips), two and three strips and eight.  Every launch is 130 - 260 pairs on ONE wave slot
(MGL_SW_DEBUG_LANE_SLOTS=1), so the wave goes through its prologues again for a second and third tile; every output is compared
with the oracle.  The forms: parameters that fold and that do not, the wide records, a target with an N (the wave that compares
bytes), 2-bit input, results stored per lane.  Pass 2's ck_block: gaps placed so that blocks are recomputed for one, two, three and
four rounds of eight columns, in column block 0 and beyond, the two pairs of a lane in different blocks, and one pair of a lane done
while the other waits -- asserted from the oracle's CIGARs.

LAST_ROW_STORED (the last strip of a launch with ql > 65 536) is not exercised at test size."""
import numpy as np
import pytest

import oracle_lib as ol
from mgl_amd import smithwaterman as sw
from test_gpu_lane_ck_narrow_carry import _gapped, _rand, _runs

pytestmark = pytest.mark.gpu

LANE16_CK = 7
CK = 32  # LANE_CK_COLS
ACGT = np.frombuffer(b"ACGT", np.uint8)
GATK = (200, -150, 260, 11)  # folds, o - e = 249: the narrow kernels
UNFOLDED = (25, -50, 110, 6)  # no folded diagonal: the wide kernels, compare mode of their own

QLS = (1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 32, 33, 36, 37, 64, 65, 68, 150)
TLS = (32, 64, 96, 256)  # (33: test_a_last_strip_of_one_row)


def _pairs(tl, ql, seed):
    """130 - 260 pairs of tl x ql: reads cut from their targets, every third with a substitution, every fifth (where the read is
    long enough) with a gap of one to three bases; the rest random"""
    rng = np.random.default_rng(seed)
    n = 130 + (37 * tl + 11 * ql) % 131
    ts, qs = [], []
    for k in range(n):
        t = _rand(rng, tl)
        if k % 7 == 6 or tl < ql:
            q = _rand(rng, ql)
        else:
            s = int(rng.integers(0, tl - ql + 1))
            q = t[s:s + ql].copy()
            if k % 3 == 1:
                j = int(rng.integers(0, ql))
                q[j] = ACGT[(int(np.searchsorted(ACGT, q[j])) + 1) % 4]
            if k % 5 == 2 and ql >= 20:
                g, p = 1 + k % 3, int(rng.integers(8, ql - 8))
                q = (np.concatenate([q[:p], _rand(rng, g), q[p:]]) if k % 2 else np.concatenate([q[:p], q[p + g:], _rand(rng, g)]))[:ql]
        ts.append(t.tobytes())
        qs.append(q.tobytes())
    assert 130 <= len(ts) <= 260
    return ts, qs


@pytest.fixture()
def lane(monkeypatch):
    monkeypatch.setenv("MGL_SW_DEBUG_LANE_SLOTS", "1")  # one wave takes every tile of the launch, one after the other
    a = sw.MicrosoftSmithWaterman(0)
    a.set_lane_kernel(2)
    yield a
    a.close()


_want = {}


def _oracle(ts, qs, params, strategy, key):
    k = (key, params, strategy)
    if k not in _want:
        _want[k] = ol.oracle_align_batch(ts, qs, params, strategy, nthreads=8)
    return _want[k]


def _check(a, ts, qs, params, strategy, key, run=None, **kw):
    res = run(a) if run else a.align_batch(ts, qs, params, strategy, **kw)
    assert a.timing().fill_kernel == LANE16_CK, (key, params, strategy)
    off, sc, cg = _oracle(ts, qs, params, strategy, key)
    assert (np.asarray(res.offsets) == off).all(), (key, params, strategy)
    assert (np.asarray(res.scores) == sc).all(), (key, params, strategy)
    assert list(res.cigars) == list(cg), (key, params, strategy)


@pytest.mark.parametrize("ql", QLS)
def test_pass_1_shapes(lane, ql):
    """every tail and trip count of the group loop against one, two, three and eight strips; SOFTCLIP reads the last row's keys,
    INDEL the corner"""
    for tl in TLS:
        ts, qs = _pairs(tl, ql, 1000 * tl + ql)
        for strategy in (ol.SOFTCLIP, ol.INDEL):
            _check(lane, ts, qs, GATK, strategy, (tl, ql))


def test_a_last_strip_of_one_row(monkeypatch):
    """tl = 33 (a strip of 32 rows and a last strip of ONE) with every ql above, as whole waves of one grouped launch, narrow and wide"""
    monkeypatch.setenv("MGL_SW_DEBUG_LANE_GROUP_MIN", "128")
    monkeypatch.setenv("MGL_SW_DEBUG_LANE_SLOTS", "1")
    ts, qs = [], []
    for ql in QLS:
        t1, q1 = _pairs(33, ql, 33000 + ql)
        ts += t1
        qs += q1
    order = np.random.default_rng(33).permutation(len(ts))
    ts, qs = [ts[k] for k in order], [qs[k] for k in order]
    assert len(ts) >= 1024  # (the library sorts batches of 1 024 pairs and more)
    a = sw.MicrosoftSmithWaterman(0)
    a.set_small_kernel(1)
    try:
        for wide in ("0", "1"):
            monkeypatch.setenv("MGL_SW_DEBUG_CK_WIDE", wide)
            for strategy in (ol.SOFTCLIP, ol.INDEL):
                _check(a, ts, qs, GATK, strategy, "tl 33", cigar_stride=256)
    finally:
        a.close()


# the forms on a subset: no trip and a tail of three, a checkpoint in the tail, one in the loop, the bench's shape
FORM_SHAPES = ((32, 3), (64, 7), (64, 33), (96, 37), (96, 68), (256, 150))


@pytest.mark.parametrize("form", ("unfolded", "wide", "n", "2bit", "per-lane"))
def test_forms(lane, monkeypatch, form):
    from mgl_amd import device_batch as db

    for tl, ql in FORM_SHAPES:
        ts, qs = _pairs(tl, ql, 1000 * tl + ql)
        key, params, run = (tl, ql), GATK, None
        if form == "unfolded":
            params = UNFOLDED
        elif form == "wide":
            monkeypatch.setenv("MGL_SW_DEBUG_CK_WIDE", "1")
        elif form == "n":  # every ninth target has an N: its wave compares bytes, the others codes
            ts = [t[:len(t) // 2] + b"N" + t[len(t) // 2 + 1:] if k % 9 == 4 else t for k, t in enumerate(ts)]
            key = (tl, ql, "N")
        elif form == "2bit":
            tb, qb = db.pack2bit(b"".join(ts)), db.pack2bit(b"".join(qs))
            t_start, q_start = np.arange(len(ts), dtype=np.int64) * tl, np.arange(len(qs), dtype=np.int64) * ql

            def run(a, s=None):
                return a.align_packed_2bit(tb, tl * len(ts), t_start, None, qb, ql * len(qs), q_start, None, tl, ql, params, s)
        else:
            monkeypatch.setenv("MGL_SW_DEBUG_COALESCED_OUT", "0")
        for strategy in (ol.SOFTCLIP, ol.INDEL):
            _check(lane, ts, qs, params, strategy, key, run=(lambda a, s=strategy: run(a, s)) if run else None)


# ---- ck_block: 160 x 150 (ten bands of 16 rows, five blocks of 32 columns)
def _block_batch():
    """259 pairs.  Pair k has ONE gap of three (a deletion, every third an insertion) whose place runs through the rows and the read's
    columns; every fourth pair has none (an exact read: no block to recompute -- its lane's other pair waits alone)."""
    tl, ql = 160, 150
    rng = np.random.default_rng(160150)
    ts, qs = [], []
    for k in range(259):
        pair = None
        if k % 4 != 3:
            for attempt in range(40):
                cut = 8 + (29 * k + 5 * attempt) % (ql - 19)
                pair = _gapped(rng, tl, ql, "D", 9 + (11 * k + attempt) % 140, 3, cut) if k % 3 else _gapped(rng, tl, ql, "I", cut + 1, 3, cut)
                if pair:
                    break
        if not pair:
            t = _rand(rng, tl)
            s = int(rng.integers(0, tl - ql + 1))
            pair = t.tobytes(), t[s:s + ql].tobytes()
        ts.append(pair[0])
        qs.append(pair[1])
    return ts, qs


def _rounds(runs):
    """per pair, from its gap runs ('D', first row, column, length) / ('I', row, first column, length): the (column block, rounds)
    of the block a gap stands in -- a walk comes from the right and from below, so the rightmost column the gap touches in the block
    is the least the block is recomputed up to: round (column - 32 b - 1) // 8 + 1 of its four"""
    out = []
    for mine in runs:
        s = set()
        for kind, _, c, n in mine:
            col = max(c, 1) if kind == "D" else c + n - 1
            b = (col - 1) // CK
            s.add((b, (col - CK * b - 1) // 8 + 1))
        out.append(s)
    return out


def test_block_rounds(lane, monkeypatch):
    ts, qs = _block_batch()
    off, _, cg = _oracle(ts, qs, GATK, ol.SOFTCLIP, "blocks")
    per = _rounds(_runs(off, cg))
    seen = set().union(*per)
    assert {(0, r) for r in (1, 2, 3, 4)} <= seen, sorted(seen)
    assert {r for b, r in seen if b >= 1} == {1, 2, 3, 4}, sorted(seen)
    lanes = [(per[k], per[k + 1]) for k in range(0, 258, 2)]
    assert sum(1 for x, y in lanes if x and y and {b for b, _ in x} != {b for b, _ in y}) >= 20, "pair A and pair B wait for different blocks"
    assert sum(1 for x, y in lanes if bool(x) != bool(y)) >= 20, "one pair of a lane is done while the other waits"
    for wide in ("0", "1"):
        monkeypatch.setenv("MGL_SW_DEBUG_CK_WIDE", wide)
        for strategy in ol.STRATEGIES:
            _check(lane, ts, qs, GATK, strategy, "blocks")
    monkeypatch.delenv("MGL_SW_DEBUG_CK_WIDE")
    _check(lane, ts, qs, UNFOLDED, ol.SOFTCLIP, "blocks")
    ts = [t[:80] + b"N" + t[81:] if k % 9 == 4 else t for k, t in enumerate(ts)]
    _check(lane, ts, qs, GATK, ol.SOFTCLIP, "blocks N")
