"""tests/rank_textbook.py -- the definition of mgl_sw_rank_chains_batch_device -- against an independent restatement (collect every chain,
fully sort, cut; overlaps as set intersections, the logarithm in fractions), against the chain stage's own chain and the strand choice, on
hand cases worked out by hand, on every refusal, and composed with the index textbook on reads from a reference with repeats.  No GPU."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_dp_cases as dpc  # noqa: E402
import chain_dp_textbook as ctb  # noqa: E402
import rank_cases as rc  # noqa: E402
import rank_textbook as rtb  # noqa: E402
import strand_textbook as stb  # noqa: E402


def _lg8(x):
    e = max(k for k in range(40) if 1 << k <= x)
    return int(256 * (e + Fraction(x, 1 << e) - 1) // 1)


def _restated(rows, max_chains, min_score, min_cnt, mask_level):
    """every chain of every row collected, then one full sort, then the cut; the parents from set intersections"""
    chains = []
    for strand, (ql, cands, f, pred, st) in enumerate(rows):
        if st:
            continue
        free = set(range(len(cands)))
        while free:
            e = min(free, key=lambda i: (-f[i], i))
            if f[e] < min_score:
                break
            path = [e]
            free.discard(e)
            while pred[path[-1]] in free:
                free.discard(pred[path[-1]])
                path.append(pred[path[-1]])
            stop = pred[path[-1]]
            score = f[e] - (f[stop] if stop >= 0 else 0)
            if score >= min_score and len(path) >= min_cnt:
                qb, qe = cands[path[-1]][1], cands[e][1] + cands[e][2]
                on_read = range(ql - qe, ql - qb) if strand else range(qb, qe)
                chains.append(dict(score=score, strand=strand, e=e, path=path[::-1], on_read=on_read, t=(cands[path[-1]][0], cands[e][0] + cands[e][2]), q=(qb, qe)))
    chains.sort(key=lambda c: (-c["score"], c["strand"], c["e"]))
    chains = chains[:max_chains]
    for x, c in enumerate(chains):
        c["parent"], c["subs"] = x, []
        for y, o in enumerate(chains[:x]):
            if o["parent"] == y and len(set(c["on_read"]) & set(o["on_read"])) * 256 >= mask_level * min(len(c["on_read"]), len(o["on_read"])):
                c["parent"] = y
                o["subs"].append(c["score"])
                break
    out = []
    for x, c in enumerate(chains):
        q = 0
        if c["parent"] == x:
            sub = min(c["score"], max(c["subs"] + [min_score]))
            raw = Fraction(40 * min(len(c["path"]), 10) * (c["score"] - sub) * _lg8(c["score"]) * 177, 10 * c["score"] * 65536)
            q = max(0, min(60, int(raw // 1) - ((3 * _lg8(len(c["subs"]) + 1) + 128) // 256)))
        out.append(rtb.Ranked(c["score"], c["strand"], len(c["path"]), *c["t"], *c["q"], c["parent"], len(c["subs"]), max(c["subs"] + [0]), q, c["e"]))
    return out, [[rows[c["strand"]][1][i] for i in c["path"]] for c in chains]


@pytest.mark.parametrize("strands", [1, 2])
def test_the_textbook_equals_collect_sort_cut(strands):
    rng = np.random.default_rng(20 + strands)
    kept = 0
    for trial in range(60):
        rows = [rc.forest_row(rng, int(rng.integers(0, 301))) if rng.random() < 0.6 else rc.dp_row(rng, int(rng.integers(0, 301))) for _ in range(strands)]
        if trial % 10 == 0:
            rows[-1] = (rows[-1][0], rows[-1][1], [rc.POISON] * len(rows[-1][1]), [rc.POISON] * len(rows[-1][1]), 5)
        min_score, min_cnt, mask_level = int(rng.integers(1, 80)), int(rng.integers(1, 6)), int(rng.choice((1, 64, 128, 200, 256)))
        for max_chains in (1, 2, 16):
            st, recs, anchors = rtb.rank_read(rows, 300, max_chains, min_score, min_cnt, mask_level)
            want, want_anchors = _restated(rows, max_chains, min_score, min_cnt, mask_level)
            assert st == 0 and recs == want and anchors == want_anchors, (trial, max_chains)
            kept += len(recs)
    assert kept > 400


def test_a_rows_first_chain_is_the_chain_stages():
    rng = np.random.default_rng(31)
    for _ in range(60):
        tl, ql, cands = dpc.random_read(rng, int(rng.integers(1, 200)), spread=int(rng.choice((3, 40, 300))))
        r = ctb.chain_dp(tl, ql, cands, 64, 200, 200, 50, 38, 3)
        (score, e, k, first), *_ = rtb.row_chains(cands, r.f, r.pred, 1, 1)
        assert score == r.score and [cands[i] for i in rtb.chain_anchors(r.pred, e, k)] == r.chain and cands[first] == r.chain[0]


def test_the_first_ranked_chain_is_the_strand_choices():
    rng = np.random.default_rng(32)
    reads = [dpc.random_read(rng, int(rng.integers(1, 120))) for _ in range(40)]
    reads[6] = reads[7] = dpc.random_read(rng, 50)  # a tie: strand 0
    reads[10], reads[11] = (30, 30, []), (30, 30, [])  # two empty rows
    reads[12] = (30, reads[13][1], [])  # the chain on strand 1 alone
    b = dpc.csr(reads)
    cs, ct, cq, cl, score, f, pred, status = ctb.chain_batch(*b, 200, 64, 200, 200, 50, 38, 3)
    strand, _, a_start, at, aq, al, a_score, a_status = stb.select_strand(bytes(4000), [0] * 20, [30] * 20, cs, ct, cq, cl, score)
    nc, recs, rs, rt, rq, rl, st = rtb.rank_batch(2, b[1], b[2], b[3], b[4], b[5], f, pred, status, 200, 4, 1, 1, 128)
    assert st == [0] * 20 and a_status == [0] * 20 and strand[3] == 0 and strand[5] == 0 and strand[6] == 1 and sum(strand) > 3
    for p in range(20):
        chosen = list(zip(at[a_start[p]:a_start[p + 1]], aq[a_start[p]:a_start[p + 1]], al[a_start[p]:a_start[p + 1]]))
        if p == 5:
            assert nc[p] == 0 and chosen == [] and rs[p] == rs[p + 1]
            continue
        first = recs[p][0]
        assert (first.strand, first.score, first.n_anchors) == (strand[p], a_score[p], len(chosen))
        assert list(zip(rt, rq, rl))[rs[p]:rs[p] + first.n_anchors] == chosen


@pytest.mark.parametrize("case", rc.HAND, ids=[c[0] for c in rc.HAND])
def test_hand_cases(case):
    name, strands, rows, (min_score, min_cnt, mask_level), want = case
    st, recs, anchors = rtb.rank_read(rows, 4096, 16, min_score, min_cnt, mask_level)
    assert st == 0 and [(r.score, r.strand, r.end_index, r.n_anchors, r.parent, r.n_sub, r.subsc) for r in recs] == want
    assert all(len(a) == r.n_anchors and a == sorted(a) for a, r in zip(anchors, recs))
    for max_chains in (1, 2):  # the cut: parents, n_sub and subsc over the cut list only
        _, cut, _ = rtb.rank_read(rows, 4096, max_chains, min_score, min_cnt, mask_level)
        assert cut == _restated(rows, max_chains, min_score, min_cnt, mask_level)[0] and len(cut) == min(len(want), max_chains)
        assert all(r.parent <= i and r.n_sub <= max_chains - 1 for i, r in enumerate(cut))


def test_shared_prefix_in_detail():
    _, recs, anchors = rtb.rank_read(rc.HAND[0][2], 4096, 16, 10, 1, 128)
    assert recs[1].score == 30 - 20 and recs[1].n_anchors == 1 and anchors[1] == [(200, 200, 10)]  # f(e) - f(stop); its own anchors only
    assert anchors[0] == [(0, 0, 10), (100, 100, 10), (300, 250, 10), (400, 400, 10)]
    assert (recs[0].t_beg, recs[0].t_end, recs[0].q_beg, recs[0].q_end) == (0, 410, 0, 410)


def test_mapq_table_and_clamps():
    for args, want in rc.MAPQ_TABLE:
        assert rtb.mapq(*args) == want, args
    assert [rtb.lg8(x) for x in (1, 2, 3, 4, 1000, (1 << 31) - 1)] == [0, 256, 384, 512, 2548, 7935]
    assert rtb.mapq(1000, 40, 50, 0) == 60 and rtb.mapq(1 << 30, 40, 10, 0) == 60  # the clamp at 60
    assert rtb.mapq(100, 99, 3, 15) == 0 and rtb.mapq(40, 40, 3, 0) == 0  # raw below the n_sub term; score = sub
    # the largest numerator: below 2^63 for every score below 2^31
    assert 40 * 10 * ((1 << 31) - 1) * rtb.lg8((1 << 31) - 1) * 177 < 1 << 63
    # sub: the best secondary's score, not below min_score, not above the score
    _, recs, _ = rtb.rank_read(rc.HAND[8][2], 4096, 16, 40, 1, 128)
    assert recs[0].mapq == rtb.mapq(100, 90, 1, 1) and recs[1].mapq == 0
    _, recs, _ = rtb.rank_read(rc.HAND[8][2], 4096, 16, 95, 1, 128)
    assert len(recs) == 1 and recs[0].mapq == rtb.mapq(100, 95, 1, 0)


@pytest.mark.parametrize("case", rc.refusals(), ids=[c[0] for c in rc.refusals()])
def test_refusals(case):
    name, strands, rows, max_cand, want = case
    nc, recs, rs, rt, rq, rl, st = rc.textbook(rc.batch([rows], strands), (max_cand, 4, 40, 3, 128))
    assert st == [want] and (want == 0) == (nc[0] > 0) and (want == 0 or (recs == [[]] and rs == [0, 0]))


def test_ranges_that_descend_or_leave_refuse_the_read():
    strands, ql, start, ct, cq, cl, f, pred, st = rc.batch([[rc.GOOD], [rc.GOOD], [rc.GOOD]], 1)
    run = lambda s, total=None: rtb.rank_batch(1, ql, s, ct, cq, cl, f, pred, None, 10, 4, 40, 3, 128, total_cand=total)  # noqa: E731
    assert run(start)[6] == [0, 0, 0]
    assert run([0, 3, 0, 3])[6] == [0, rtb.BAD_ARG, 0] and run([0, 3, 0, 3])[0] == [1, 0, 1]
    assert run([-1, 3, 6, 9])[6] == [rtb.BAD_ARG, 0, 0]
    assert run([0, 3, 6, 10], total=9)[6] == [0, 0, rtb.BAD_ARG] and run([0, 3, 6, 9], total=9)[6] == [0, 0, 0]
    for strands in (1, 2):
        b = rc.mixed_batch(np.random.default_rng(5), strands)
        out = rc.textbook(b, (150, 4, 20, 2, 128))
        assert len(out[0]) == (39 if strands == 2 else 40) and sorted(set(out[6])) == [0, rtb.BAD_ARG, rtb.UNSUPPORTED]
        assert out[0][0] == out[0][1] == out[0][-1] == 0 and out[6][0] == out[6][-1] == 0 and max(out[0]) == 4


def test_reads_from_a_reference_with_repeats():
    """section 9k's composition: a read whose window has an exact copy cannot be placed (mapq 0, a secondary of equal score inside the
    copy, the true place ranked first); one per cent of divergence makes it placeable but not certain; a read without a copy is 60"""
    for divergence in (0.0, 0.01):
        ref, reads, truth, copy, got, (nc, recs, rs, rt, rq, rl, st) = rc.repeat_mapped(divergence)
        chained, chosen = got[1], got[2]
        assert st == [0] * 8 and len(copy) == 4 and len(ref) == 43000 + 4 * 5000
        for p, (pos, n, strand) in enumerate(truth):
            first = recs[p][0]
            assert first.strand == strand == chosen[0][p] and first.score == chosen[6][p] == chained[4][2 * p + strand]
            assert pos <= first.t_beg < first.t_end <= pos + n
            if p >= 4:
                assert nc[p] == 1 and first.mapq == 60
                continue
            second = recs[p][1]
            at, m = copy[p]
            assert nc[p] == 2 and second.parent == 0 and second.mapq == 0 and at <= second.t_beg < second.t_end <= at + m and first.n_sub == 1
            if divergence == 0.0:
                assert first.mapq == 0 and second.score == first.score == first.subsc
            else:
                assert 0 < first.mapq < 60 and second.score < first.score
    # measured here: mapq of the four reads with a copy at one per cent
    assert [r[0].mapq for r in rc.repeat_mapped(0.01)[5][1][:4]] == [38, 20, 19, 43]
