"""The chaining DP's definition (tests/chain_dp_textbook.py) against an independent restatement and against values worked out by hand."""
import numpy as np
import pytest

import chain_dp_cases as cases
import chain_dp_textbook as tb
from mgl_amd import synth


def restated(cands, max_pred, mdt, mdq, bw, pen_gap, pen_skip):
    """backward, O(N^2): every j < i is looked at, the window is one more condition, and the arg-max is explicit with the key (score, j)"""
    n = len(cands)
    f, pred = [], []
    for i in range(n):
        ti, qi, li = cands[i]
        options = [(li, -1)]
        for j in range(i):
            tj, qj, lj = cands[j]
            dt, dq = ti - tj - lj, qi - qj - lj
            dd = dt - dq if dt >= dq else dq - dt
            if i - j > max_pred or min(dt, dq) < 0 or dt > mdt or dq > mdq or dd > bw:
                continue
            log = 0
            while (2 << log) <= dd + 1:
                log += 1
            options.append((f[j] + li - (pen_gap * dd + pen_skip * min(dt, dq)) // 256 - log // 2, j))
        s, j = max(options)
        f.append(s), pred.append(j)
    if not n:
        return [], 0, f, pred
    top = max(f)
    i, chain = f.index(top), []
    while i != -1:
        chain.insert(0, cands[i])
        i = pred[i]
    return chain, top, f, pred


@pytest.mark.parametrize("max_pred", (1, 2, 63, 64))
def test_textbook_equals_the_restatement(max_pred):
    rng = np.random.default_rng(100 + max_pred)
    for n in list(cases.RING_SIZES) + [int(rng.integers(0, 201)) for _ in range(12)]:
        tl, ql, c = cases.random_read(rng, n)
        params = cases.random_params(rng, max_pred)
        r = tb.chain_dp(tl, ql, c, *params)
        assert r.status == 0 and (r.chain, r.score, r.f, r.pred) == restated(c, *params), (n, params)
    for tl, ql, c in cases.ring_reads(rng, max_pred):
        r = tb.chain_dp(tl, ql, c, max_pred, *cases.RING)
        assert (r.chain, r.score, r.f, r.pred) == restated(c, max_pred, *cases.RING)


def test_pen_against_hand_values():
    # pen_gap = 100, pen_skip = 1: ((100 dd + dg) >> 8) + (ilog2(dd + 1) >> 1), dg = min(dt, dq)
    hand = {0: (0, 0, 0, 1), 1: (0, 0, 1, 1), 2: (0, 0, 1, 1), 3: (2, 2, 3, 3), 4: (2, 2, 3, 3), 7: (3, 3, 4, 4), 8: (4, 4, 5, 5)}
    for dd, row in hand.items():
        for dg, want in zip((0, 1, 255, 256), row):
            assert tb.pen(dg + dd, dg, 100, 1) == want == tb.pen(dg, dg + dd, 100, 1), (dd, dg)
    assert [tb.ilog2(x) for x in (1, 2, 3, 4, 7, 8, 9, 1 << 30)] == [0, 1, 1, 2, 2, 3, 3, 30]
    assert tb.guard_ok(0, 0, 1, (1 << 31) - 1, 0) and not tb.guard_ok(0, 0, 1, 1 << 31, 0)
    assert tb.guard_ok(1000, 2000, 0, 0, 2147483) and not tb.guard_ok(1000, 2000, 0, 0, 2147484)


@pytest.mark.parametrize("name,params,read,pred", cases.RULE_CASES + cases.LOG_CASES, ids=[c[0] for c in cases.RULE_CASES + cases.LOG_CASES])
def test_rule_edges_and_ties(name, params, read, pred):
    r = tb.chain_dp(*read, *params)
    assert r.status == 0 and r.pred == pred
    assert (r.chain, r.score, r.f, r.pred) == restated(read[2], *params)


def test_ilog2_steps_and_tie_scores():
    by = {c[0]: tb.chain_dp(*c[2], *c[1]) for c in cases.RULE_CASES + cases.LOG_CASES}
    assert [by["ilog2 at dd = %d" % dd].score for dd in (0, 1, 2, 3, 4, 7, 8, 15)] == [45, 45, 45, 44, 44, 44, 44, 43]
    assert by["tie with the start"].f == [1, 5] and by["start wins by one"].f == [1, 5]
    assert by["tie between predecessors"].f == [10, 10, 15]
    r = by["tie for the end"]
    assert r.f == [10, 10, 20, 20] and r.chain == [(0, 0, 10), (10, 10, 10)]
    assert by["overlaps on one diagonal"].f == [20, 20, 20, 30]
    assert by["guard edge, pen_gap"].f == [20, 20, 40] and by["guard edge, pen_skip"].f == [20, 20, 40]


@pytest.mark.parametrize("max_pred", cases.RING_PREDS)
def test_ring_constructions(max_pred):
    tl, ql, c = cases.spaced(64, 2)
    r = tb.chain_dp(tl, ql, c, max_pred, *cases.RING)
    assert r.pred[64] == (0 if max_pred == 64 else -1) and r.pred[128] == (64 if max_pred == 64 else -1)
    assert len(r.chain) == (3 if max_pred == 64 else 1)
    r = tb.chain_dp(*cases.spaced(max_pred, 2), max_pred, *cases.RING)
    assert [r.pred[max_pred], r.pred[2 * max_pred]] == [0, max_pred] and r.score == 30 - 2 * 2
    r = tb.chain_dp(*cases.spaced(max_pred + 1, 2), max_pred, *cases.RING)
    assert set(r.pred) == {-1} and r.score == 10 and r.chain == [(0, 0, 10)]


def test_statuses_and_the_batch_form():
    ok = (64, 100, 100, 50, 38, 0)
    assert tb.chain_dp(10, 10, [], *ok) == tb.Chained(0, [], 0, [], [])
    for tl, ql, c in ((0, 10, []), (10, 0, []), (10, 10, [(0, 0, 0)]), (10, 10, [(-1, 0, 1)]), (10, 10, [(0, -1, 1)]), (10, 10, [(5, 0, 6)]), (10, 10, [(0, 5, 6)])):
        assert tb.chain_dp(tl, ql, c, *ok) == tb.Chained(tb.BAD_ARG, [], 0, [], [])
    assert tb.chain_dp(10, 10, [(5, 5, 5)], *ok).status == 0
    assert tb.chain_dp(10, 10, [(0, 0, 1), (1, 1, 1)], *ok, max_cand=1).status == tb.UNSUPPORTED
    assert tb.chain_dp(10, 0, [(0, 0, 1), (1, 1, 1)], *ok, max_cand=1).status == tb.BAD_ARG  # in the header's order
    batch = cases.mixed_batch(np.random.default_rng(5))
    cs, ct, cq, cl, score, f, pred, status = tb.chain_batch(*batch, 150, *cases.RING_PREDS[3:], *cases.RING)
    n = len(batch[0])
    assert 38 <= n <= 48 and status.count(tb.BAD_ARG) == 8 and status.count(tb.UNSUPPORTED) == 1
    assert status[:2] == [0, 0] == status[-2:] and cs[:3] == [0, 0, 0] and cs[-1] == cs[-3] == len(ct)
    assert any(b < a for a, b in zip(batch[2], batch[2][1:]))
    assert all((k == 0) == (s == 0) or st for k, s, st in zip(np.diff(cs), score, status))
    # a refused read wrote no f: its candidates are None unless another read holds them
    assert sum(x is None for x in f) == sum(x is None for x in pred) > 0


def _accepts(chain, tl, ql):
    """the inequalities mgl_sw_align_chain_batch_device demands of a chain"""
    return (all(l >= 1 and t >= 0 and q >= 0 for t, q, l in chain) and all(a[0] + a[2] <= b[0] and a[1] + a[2] <= b[1] for a, b in zip(chain, chain[1:]))
            and chain[-1][0] + chain[-1][2] <= tl and chain[-1][1] + chain[-1][2] <= ql)


def test_every_chain_is_one_the_chain_entry_accepts():
    rng = np.random.default_rng(9)
    for _ in range(60):
        tl, ql, c = cases.random_read(rng, int(rng.integers(1, 150)))
        params = cases.random_params(rng)
        r = tb.chain_dp(tl, ql, c, *params)
        assert r.chain and _accepts(r.chain, tl, ql)
        assert all(b[0] - a[0] - a[2] <= params[1] and b[1] - a[1] - a[2] <= params[2] for a, b in zip(r.chain, r.chain[1:]))
        assert 1 <= r.score <= sum(l for _, _, l in r.chain) <= ql


def test_chain_on_noisy_candidates_stays_on_the_true_diagonal():
    rng = np.random.default_rng(1043)
    kinds = [0] * 4
    for T, Q, true in synth.chain_pairs(43, 32):
        c, kind = synth.noisy_candidates(rng, len(T), len(Q), true)
        assert c == sorted(c)
        for k in kind:
            kinds[k] += 1
        r = tb.chain_dp(len(T), len(Q), c, *cases.MINIMAP)
        on = {x for x, k in zip(c, kind) if k in (synth.CAND_TRUE, synth.CAND_OVERLAP)}
        assert r.status == 0 and set(r.chain) <= on and _accepts(r.chain, len(T), len(Q))
        assert len(r.chain) >= 0.9 * len(true)
    assert min(kinds) > 300  # every kind is there in numbers: 32 pairs of about 50 true anchors
