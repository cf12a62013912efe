"""tests/seed_extend_textbook.py, the definition of mgl_sw_extend_seed_batch_device, against what it must satisfy whatever computes it: the
mirror identity, an independent three-matrix score, every empty-flank case, the merge across the seed, the drop bits and the adaptive
flag on each side."""
import random

import numpy as np

import extend_adaptive_cases as cases
import extend_textbook as et
import seed_extend_textbook as st
from test_extend_textbook import PARAM_SETS, RECORDS, _gotoh_prefix_scores, _rand_pair

GATK = (200, -150, 260, 11)


def _mirror_seed(T, Q, seed):
    s_t, s_q, sl = seed
    return len(T) - s_t - sl, len(Q) - s_q - sl, sl


def _random_seed(rng, tl, ql):
    sl = rng.randint(1, min(tl, ql, 12))
    return rng.randint(0, tl - sl), rng.randint(0, ql - sl), sl


def _check_mirror(T, Q, seed, params, band, zdrop, to_qend, adaptive):
    a, ca, la, ra = st.seed_extend(T, Q, seed, *params, band, zdrop, to_qend, adaptive)
    b, cb, lb, rb = st.seed_extend(T[::-1], Q[::-1], _mirror_seed(T, Q, seed), *params, band, zdrop, to_qend, adaptive)
    ctx = (T, Q, seed, params, band, zdrop, to_qend, adaptive)
    assert (la, ra) == (rb, lb), ctx
    assert (a.score, a.seed_score) == (b.score, b.seed_score), ctx
    assert (b.t_beg, b.t_end, b.q_beg, b.q_end) == (len(T) - a.t_end, len(T) - a.t_beg, len(Q) - a.q_end, len(Q) - a.q_beg), ctx
    swap = lambda v: (v & 1) << 1 | v >> 1  # noqa: E731
    assert (b.dropped, b.cigar_from) == (swap(a.dropped), swap(a.cigar_from)), ctx
    assert st.elements(cb) == st.elements(ca)[::-1], ctx
    assert et.cigar_spans(ca) == (a.t_end - a.t_beg, a.q_end - a.q_beg)
    assert 0 <= a.t_beg <= seed[0] and seed[0] + seed[2] <= a.t_end <= len(T) and 0 <= a.q_beg <= seed[1] and seed[1] + seed[2] <= a.q_end <= len(Q)
    return a, ca, la, ra


def test_mirror_identity_on_the_golden_suites_and_on_random_pairs():
    rng = random.Random(21)
    todo = [(g.t, g.q, g.params) for g in RECORDS]
    for _ in range(300):
        todo.append(_rand_pair(rng, rng.randint(1, 80), rng.randint(1, 80), b"AC" if rng.random() < 0.3 else b"ACGT") + (rng.choice(PARAM_SETS),))
    assert len(todo) > 500
    dropped = [0, 0, 0, 0]
    qend = empty = 0
    for T, Q, params in todo:
        seed = _random_seed(rng, len(T), len(Q))
        band = rng.choice((0, 1, 2, 5, 17, 64, 1000))
        zdrop = rng.choice((-1, 0, params[3], 3 * params[2], 40 * params[0]))
        a, _, la, ra = _check_mirror(T, Q, seed, params, band, zdrop, rng.random() < 0.5, rng.random() < 0.5)
        dropped[a.dropped] += 1
        qend += a.cigar_from != 0
        empty += seed[0] == 0 or seed[1] == 0 or seed[0] + seed[2] == len(T) or seed[1] + seed[2] == len(Q)
    assert min(dropped) > 10 and qend > 100 and empty > 30, (dropped, qend, empty)


def test_full_band_without_zdrop_is_best_left_plus_seed_plus_best_right():
    rng = random.Random(4)
    todo = [(g.t, g.q, g.params) for g in RECORDS[::3] if len(g.t) * len(g.q) <= 2500]
    for _ in range(150):
        todo.append(_rand_pair(rng, rng.randint(1, 40), rng.randint(1, 40), b"AC" if rng.random() < 0.4 else b"ACGT") + (rng.choice(PARAM_SETS),))
    assert len(todo) > 250
    both = 0
    for T, Q, params in todo:
        tl, ql = len(T), len(Q)
        s_t, s_q, sl = seed = _random_seed(rng, tl, ql)

        def best(t, q):
            G = _gotoh_prefix_scores(t, q, *params)
            return max(G[i][j] for i in range(len(t) + 1) for j in range(len(q) + 1))

        for adaptive in (False, True):
            a, cigar, la, ra = st.seed_extend(T, Q, seed, *params, tl + ql, -1, False, adaptive)
            want = best(T[:s_t][::-1], Q[:s_q][::-1]) + st.seed_score(T, Q, *seed, params[0], params[1]) + best(T[s_t + sl:], Q[s_q + sl:])
            assert a.score == want, (T, Q, seed, params, a)
            assert (a.dropped, a.cigar_from) == (0, 0)
            assert et.cigar_spans(cigar) == (a.t_end - a.t_beg, a.q_end - a.q_beg)
            assert et.cigar_score(cigar, T[a.t_beg:a.t_end], Q[a.q_beg:a.q_end], *params) == a.score, (T, Q, seed, params, cigar)
        both += la.score > 0 and ra.score > 0
    assert both > 40


def test_every_empty_flank_case():
    T, Q = b"ACGTTGCAAGGCTA", b"ACGTAGCAAGCCTA"
    tl, ql = len(T), len(Q)
    zero, no_target = st.EMPTY_QUERY_FLANK, st.EMPTY_TARGET_FLANK
    assert zero == et.Ext(0, 0, 0, 0, 0, 0, 0, 0) and no_target == et.Ext(0, 0, 0, -0x40000000, -1, 0, 0, 0)
    for to_qend in (False, True):
        ext = lambda seed, T=T, Q=Q: st.seed_extend(T, Q, seed, *GATK, 8, -1, to_qend)  # noqa: E731
        a, c, l, r = ext((3, 0, 4))                    # the seed at the query's start: nothing left to extend
        assert l == zero and (a.q_beg, a.t_beg) == (0, 3) and r.score > 0 and a.cigar_from == (2 if to_qend else 0)
        a, c, l, r = ext((tl - 7, ql - 4, 4))          # ... at the query's end
        assert r == zero and (a.q_end, a.t_end) == (ql, tl - 3) and l.score > 0
        a, c, l, r = ext((0, 3, 4))                    # at the target's start: three query bases have nothing to lie against
        assert l == no_target and (a.t_beg, a.q_beg) == (0, 3) and a.cigar_from & 1 == 0
        a, c, l, r = ext((tl - 4, ql - 7, 4))          # at the target's end
        assert r == no_target and (a.t_end, a.q_end) == (tl, ql - 3) and a.cigar_from & 2 == 0
        a, c, l, r = ext((2, 0, 5), Q=T[2:7])          # the seed is the whole query
        assert (l, r) == (zero, zero) and (a, c) == (st.SeedAln(1000, 2, 7, 0, 5, 1000, 0, 0), "5M")
        a, c, l, r = ext((0, 3, tl), Q=b"GGG" + T + b"CC")   # the seed is the whole window
        assert (l, r) == (no_target, no_target) and (a, c) == (st.SeedAln(200 * tl, 0, tl, 3, 3 + tl, 200 * tl, 0, 0), f"{tl}M")
        a, c, l, r = ext((0, 0, tl), Q=T)              # ... and the whole query as well
        assert (l, r) == (zero, zero) and c == f"{tl}M"
        a, c, l, r = ext((0, 0, 1), T=b"A", Q=b"C")
        assert (a, c) == (st.SeedAln(-150, 0, 1, 0, 1, -150, 0, 0), "1M")


def test_an_inexact_seed():
    T, Q = b"TTTTACGTACGTACGTCCCC", b"TTTTACGAACGTACTTCCCC"
    a, c, l, r = st.seed_extend(T, Q, (4, 4, 12), *GATK, 4, -1)
    assert a.seed_score == 10 * 200 - 2 * 150 and a.score == 18 * 200 - 2 * 150 and c == "20M" and (a.t_beg, a.t_end, a.q_beg, a.q_end) == (0, 20, 0, 20)


def test_m_merges_across_the_seed_and_a_gap_next_to_it_does_not():
    core = b"ACGGTCATTGCAGTCCATGA"
    T = core + b"GATTACA" + core[::-1]
    a, c, l, r = st.seed_extend(T, T, (20, 20, 7), *GATK, 4, -1)
    assert c == "47M" and (l.score, r.score) == (4000, 4000)
    # the query lacks the three target bases in front of the seed and has three more behind it; to-query-end walks from the corner, and
    # the cheapest place for either gap is at the anchor
    Q = core[:17] + b"GATTACA" + b"TTT" + core[::-1]
    Tq = core[:17] + b"GGG" + b"GATTACA" + core[::-1]
    for to_qend in (False, True):
        a, c, l, r = st.seed_extend(Tq, Q, (20, 17, 7), *(1, -4, 1, 1), 6, -1, to_qend)
        els = st.elements(c)
        assert (7, "M") in els and els[els.index((7, "M")) - 1] == (3, "D") and els[els.index((7, "M")) + 1] == (3, "I"), c
        assert c == "17M3D7M3I20M"


def _junk(rng, n, alphabet):
    return bytes(rng.choice(alphabet) for _ in range(n))


def test_both_sides_dropped_one_and_none():
    rng = random.Random(9)
    core_l, core_r, seed = _junk(rng, 60, b"ACGT"), _junk(rng, 60, b"ACGT"), b"GATTACAGATTACA"
    jt, jq = _junk(rng, 200, b"AC"), _junk(rng, 200, b"GT")
    for left_junk in (False, True):
        for right_junk in (False, True):
            T = (jt if left_junk else b"") + core_l + seed + core_r + (jt if right_junk else b"")
            Q = (jq if left_junk else b"") + core_l + seed + core_r + (jq if right_junk else b"")
            s0 = (200 if left_junk else 0) + 60
            for adaptive in (False, True):
                a, c, l, r = st.seed_extend(T, Q, (s0, s0, 14), *GATK, 10, 1000, False, adaptive)
                assert a.dropped == (1 if left_junk else 0) | (2 if right_junk else 0)
                assert (l.dropped, r.dropped) == (int(left_junk), int(right_junk))
                assert c == "134M" and a.score == 134 * 200 and (a.t_beg, a.t_end) == (s0 - 60, s0 + 74)


def test_the_adaptive_flag_reaches_each_side():
    """a drift pair (tests/extend_adaptive_cases.py: 3 000 rows, ten 20-base indels) on either side of the seed at band 64: the fixed
    band loses the path after the third indel on each side, the band that follows it reaches both ends of the query"""
    d = cases.drift_pairs()
    (tr, qr), (tlft, qlft) = d["deletions"], d["insertions"]
    seed = b"GATTACAGATTACAGATTACA"
    T, Q = tlft[::-1] + seed + tr, qlft[::-1] + seed + qr
    s = (len(tlft), len(qlft), len(seed))
    fixed, cf, lf, rf = st.seed_extend(T, Q, s, *GATK, 64, -1, True, False)
    adapt, ca, la, ra = st.seed_extend(T, Q, s, *GATK, 64, -1, True, True)
    assert (la, ra) == (st.side(tlft, qlft, GATK, 64, -1, True, True)[0], st.side(tr, qr, GATK, 64, -1, True, True)[0])
    assert adapt.cigar_from == 3 and (adapt.t_beg, adapt.q_beg, adapt.q_end) == (0, 0, len(Q)) and adapt.t_end == len(T)
    assert adapt.score == (3000 + 2800 + len(seed)) * 200 - 20 * (260 + 19 * 11)  # every base of the shorter flank matched, twenty indels
    assert fixed.score < adapt.score - 200 * 2000 and (lf, rf) != (la, ra)
    els = st.elements(ca)
    assert sum(1 for n, op in els if (n, op) == (20, "D")) == 10 and sum(1 for n, op in els if (n, op) == (20, "I")) == 10
    assert et.cigar_score(ca, T, Q, *GATK) == adapt.score


def test_seeds_on_numpy_bytes_and_bytearrays():
    T, Q = np.frombuffer(b"ACGTACGT", np.uint8), bytearray(b"ACGTACGT")
    assert st.seed_extend(T, Q, (2, 2, 3), *GATK, 3, -1)[1] == "8M"
