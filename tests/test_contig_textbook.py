"""tests/contig_textbook.py against what it is built on, against an independent restatement, on hand cases -- and the proof that the
reads of the pipeline test (tests/contig_cases.py) are adversarial: without the contig stages each of them goes wrong."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_dp_cases as dpc  # noqa: E402
import chain_dp_textbook as ctb  # noqa: E402
import contig_cases as cc  # noqa: E402
import contig_textbook as gtb  # noqa: E402
import index_textbook as itb  # noqa: E402

P = (64, 200, 200, 50, 38, 3)


def _rows(seed, count):
    rng = np.random.default_rng(seed)
    for _ in range(count):
        n = int(rng.choice((0, 1, 2, 5, 30, 63, 64, 65, 100, 130, 200)))
        tl, ql, cands = dpc.random_read(rng, n, spread=int(rng.choice((3, 40, 300))), jitter=int(rng.choice((0, 6, 40))))
        yield rng, tl, ql, cands, dpc.random_params(rng)


def test_all_groups_equal_is_the_plain_textbook():
    for rng, tl, ql, cands, params in _rows(31, 60):
        for g in (0, 7, 2 ** 31 - 1):
            assert gtb.chain_dp_grouped(tl, ql, cands, [g] * len(cands), *params) == ctb.chain_dp(tl, ql, cands, *params)
        # the refusals are the plain ones too
        if cands:
            assert gtb.chain_dp_grouped(tl, ql, cands, [0] * len(cands), *params, max_cand=len(cands) - 1).status == ctb.UNSUPPORTED
    assert gtb.chain_dp_grouped(0, 5, [], [], *P).status == ctb.BAD_ARG and gtb.chain_dp_grouped(50, 50, [(45, 0, 10)], [0], *P).status == ctb.BAD_ARG


def _split_restatement(tl, ql, cands, groups, max_pred, max_dist_t, max_dist_q, bw, pen_gap, pen_skip):
    """the row split by group, every part chained on its own -- a predecessor still no more than max_pred positions of the WHOLE row
    behind --, the indices mapped back; then the end over the whole row"""
    n = len(cands)
    f, pred = [0] * n, [-1] * n
    for g in sorted(set(groups)):
        where = [i for i in range(n) if groups[i] == g]
        if g < 0:
            for i in where:
                f[i] = cands[i][2]
            continue
        part = [cands[i] for i in where]
        pf, pp = [], []
        for a, (ti, qi, li) in enumerate(part):
            options = [(li, -1)]
            for b in range(a):
                tj, qj, lj = part[b]
                dt, dq = ti - tj - lj, qi - qj - lj
                if where[a] - where[b] <= max_pred and 0 <= dt <= max_dist_t and 0 <= dq <= max_dist_q and abs(dt - dq) <= bw:
                    options.append((pf[b] + li - ctb.pen(dt, dq, pen_gap, pen_skip), b))
            best = max(options)  # (the largest score, then the largest predecessor; -1 is the smallest)
            pf.append(best[0]), pp.append(best[1])
        for a, i in enumerate(where):
            f[i], pred[i] = pf[a], -1 if pp[a] < 0 else where[pp[a]]
    if n == 0:
        return [], 0, f, pred
    end = min(range(n), key=lambda i: (-f[i], i))
    chain, i = [], end
    while i >= 0:
        chain.insert(0, tuple(cands[i]))
        i = pred[i]
    return chain, f[end], f, pred


def test_against_the_row_split_by_group():
    seen = set()
    for rng, tl, ql, cands, params in _rows(32, 60):
        n = len(cands)
        for kind in ("blocks", "interleaved", "random", "with -1"):
            if kind == "blocks":
                groups = [i * 3 // max(n, 1) for i in range(n)]
            elif kind == "interleaved":
                groups = [i % 2 for i in range(n)]
            elif kind == "random":
                groups = rng.integers(0, 4, n).tolist()
            else:
                groups = rng.integers(-1, 3, n).tolist()
            r = gtb.chain_dp_grouped(tl, ql, cands, groups, *params)
            assert (r.chain, r.score, r.f, r.pred) == _split_restatement(tl, ql, [tuple(c) for c in cands], groups, *params), (kind, n)
            assert all(p < 0 or (groups[p] == groups[i] and groups[i] >= 0) for i, p in enumerate(r.pred))
            if n >= 30 and any(p >= 0 and i - p > 1 for i, p in enumerate(r.pred)):
                seen.add(kind)
    assert seen == {"blocks", "interleaved", "random", "with -1"}  # chains that skip over candidates of other groups, in every kind


def test_hand_cases():
    a, b = (100, 0, 10), (120, 20, 10)  # 10 apart on one diagonal
    assert gtb.chain_dp_grouped(500, 500, [a, b], [0, 0], *P).pred == [-1, 0]
    two = gtb.chain_dp_grouped(500, 500, [a, b], [0, 1], *P)
    assert (two.pred, two.f, two.chain) == ([-1, -1], [10, 10], [a])  # two chains; the tie in f goes to the smaller index
    none = gtb.chain_dp_grouped(500, 500, [a, b], [-1, -1], *P)
    assert (none.pred, none.f) == ([-1, -1], [10, 10])  # -1 equals -1 and still does not chain
    # a tie in f across groups: [0, 2] in group 0 and [1, 3] in group 1 both reach 20: the smaller end index wins
    row = [(100, 0, 10), (1100, 0, 10), (120, 20, 10), (1120, 20, 10)]
    tie = gtb.chain_dp_grouped(2000, 500, row, [0, 1, 0, 1], 64, 5000, 5000, 5000, 0, 0)
    assert (tie.f, tie.pred, tie.chain, tie.score) == ([10, 10, 20, 20], [-1, -1, 0, 1], [row[0], row[2]], 20)
    # max_pred counts positions of the whole row: with a stranger between them the two are 2 apart
    assert gtb.chain_dp_grouped(2000, 500, row[:3], [0, 1, 0], 1, 5000, 5000, 5000, 0, 0).pred == [-1, -1, -1]
    assert gtb.chain_dp_grouped(2000, 500, row[:3], [0, 1, 0], 2, 5000, 5000, 5000, 0, 0).pred == [-1, -1, 0]


def test_contig_of_at_every_edge():
    start, length = cc.TABLE
    assert gtb.table_ok(cc.TABLE_LEN, start, length)
    want = {(0, 1): 0, (0, 100): 0, (0, 101): -1, (99, 1): 0, (99, 2): -1, (100, 1): -1, (101, 1): 1, (101, 2): -1, (102, 1): -1, (103, 1): -1, (104, 1): 2,
            (104, 50): 2, (104, 51): -1, (153, 1): 2, (154, 1): -1, (155, 3): 3, (157, 1): 3, (157, 2): -1, (158, 1): -1, (-1, 5): -1, (0, 0): -1}
    for (t, l), c in want.items():
        assert gtb.contig_of(start, length, t, l) == c, (t, l)
    edges = cc.contig_of_edges(start, length)
    assert {gtb.contig_of(start, length, t, l) for t, l in edges} == {-1, 0, 1, 2, 3}
    # one contig: the whole buffer
    assert [gtb.contig_of([0], [40], t, l) for t, l in ((0, 40), (0, 41), (39, 1), (40, 1), (-1, 1))] == [0, -1, 0, -1, -1]
    # the rules of the table
    for ref_len, s, n in ((158, [1, 101], [99, 57]), (158, [0, 100], [100, 58]), (158, [0, 101], [100, 56]), (158, [0, 101], [100, 58]), (158, [0, 101], [0, 57]),
                          (158, [], [])):
        assert not gtb.table_ok(ref_len, s, n)
    buf, s, n = gtb.layout([b"ACGT", b"A", b"TT"], gap=2)
    assert (buf, s, n) == (b"ACGTNNANNTT", [0, 6, 9], [4, 1, 2]) and gtb.table_ok(len(buf), s, n) and gtb.gaps_ok(buf, s, n)
    assert not gtb.gaps_ok(b"ACGTNAANNTT", s, n) and gtb.gaps_ok(b"ACGTnaANNTT", s, n)  # (lower case is no base to the seed stage)


def test_locate_window_contigs_hand_cases():
    start, length, slack, max_tl, cases = cc.locate_cases()
    a_start, at, aq, al = cc.csr([c[2] for c in cases])
    t_start, t_len, out, status, rid = gtb.locate_window_contigs(start, length, [c[1] for c in cases], a_start, at, aq, al, slack, max_tl)
    for p, (name, _, anchors, st, ts, tl, c) in enumerate(cases):
        assert (status[p], t_start[p], t_len[p], rid[p]) == (st, ts, tl, c), name
        assert all((out[i] is None) == (st != 0) for i in range(a_start[p], a_start[p + 1])), name
        assert all(out[i] == at[i] - ts for i in range(a_start[p], a_start[p + 1]) if st == 0)
    # one contig over the whole buffer is index_textbook's locate_window, whatever the anchors
    rng = np.random.default_rng(8)
    q_len = rng.integers(50, 400, 40).tolist()
    chains = [[(int(rng.integers(-800, 10700)), int(rng.integers(0, ql - 20)), 20)] for ql in q_len]
    a_start, at, aq, al = cc.csr(chains)
    got = gtb.locate_window_contigs([0], [10000], q_len, a_start, at, aq, al, 150, 600)
    assert list(got[:4]) == list(itb.locate_window(10000, q_len, a_start, at, aq, al, 150, 600)) and {0, 1, 5} == set(got[3])


def test_the_pipelines_reads_are_adversarial():
    buffer, start, length, names, reads, index, got = cc.pipeline_textbook()
    seeded, groups, chained, chosen, located, fed, ranked = got
    plain = cc.pipeline_ungrouped()
    end = [s + n for s, n in zip(start, length)]
    assert gtb.table_ok(len(buffer), start, length) and gtb.gaps_ok(buffer, start, length) and len(start) == 4
    assert set(groups) == {0, 1, 2, 3}  # (no candidate straddles a gap: a k-mer with an N is no k-mer)

    def span(anchors, t_start):
        return t_start + anchors[0][0], t_start + anchors[-1][0] + anchors[-1][2]

    # ---- the chimeric read: one chain over both contigs without groups, one contig with them, the other half a second primary chain
    p = cc.CHIMERA
    lo, hi = span(plain[4][p][3], plain[4][p][1])
    assert lo < end[0] < start[1] < hi and plain[3][3][p] == 0
    lo, hi = span(fed[p][3], fed[p][1])
    c = located[4][p]
    assert c in (0, 1) and start[c] <= lo < hi <= end[c] and located[3][p] == 0
    recs = ranked[1][p]
    assert ranked[0][p] >= 2 and recs[0].parent == 0 and recs[1].parent == 1
    assert {gtb.contig_of(start, length, r.t_beg, r.t_end - r.t_beg) for r in recs[:2]} == {0, 1}
    # without groups the rank stage sees one chain over the gap
    assert gtb.contig_of(start, length, *(lambda a: (a[0], a[1] - a[0]))(span(plain[4][p][3], plain[4][p][1]))) == -1

    # ---- the read 20 bases into contig 1: the plain window reaches into contig 0, the clipped one starts with the contig
    p = cc.EDGE
    assert plain[3][0][p] < end[0] and plain[3][3][p] == 0
    assert located[0][p] == start[1] and located[4][p] == 1 and located[3][p] == 0 and chosen[0][p] == 1
    assert located[0][p] + located[1][p] <= end[1]

    # ---- read 0: its window is in contig 0 and in contig 3: mapq 0, the secondary in the other contig
    recs = ranked[1][0]
    assert ranked[0][0] >= 2 and recs[0].mapq == 0 and recs[1].parent == 0 and recs[1].score == recs[0].score
    assert [gtb.contig_of(start, length, r.t_beg, r.t_end - r.t_beg) for r in recs[:2]] == [0, 3] and located[4][0] == 0

    # ---- the others: where the truth says, with a mapping quality; the unrelated read unmapped
    _, _, truth = cc.pipeline_set()
    for p, (c, pos, n, strand) in enumerate(truth):
        assert located[4][p] == c and chosen[0][p] == strand and located[3][p] == 0
        assert located[0][p] <= start[c] + pos and start[c] + pos + n <= located[0][p] + located[1][p]
        assert p == 0 or ranked[1][p][0].mapq >= 30
    p = cc.UNRELATED_AT
    assert (located[0][p], located[1][p], located[3][p], located[4][p], ranked[0][p], fed[p][3]) == (0, 0, 0, -1, 0, [])
