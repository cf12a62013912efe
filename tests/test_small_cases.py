"""tests/small_cases.py on the CPU: the restated geometry of the one-wave pair kernel (sw_small_pair.h) pinned at its boundaries and held
against the planner where the library shows it, the restated walk held against the oracle on every pair of the module, and every
case doing what it was built for -- judged from the oracle's CIGARs and scores and from the plain H matrix, no GPU."""
import functools

import numpy as np
import pytest

import oracle_lib as ol
import range_guards as rg
import small_cases as sc
from mgl_amd import _lib

SMALL = 8
SETS = ("rows", "ramps", "runs", "round_ties", "last_cell_ties", "bytes", "span", "fits", "slots")
FULL_WAVE = [127, 128] + list(range(253, 257)) + list(range(379, 385)) + list(range(505, 513))


@functools.lru_cache(maxsize=None)
def oracle(name, k, strategy):
    """the oracle's (offsets, scores, cigars) of batch k of a set"""
    c = sc.cases(name)[k]
    return ol.oracle_align_batch(list(c.targets), list(c.queries), c.params, strategy, nthreads=8)


# ---- the geometry

def test_rows_per_lane_and_lanes_at_every_boundary():
    assert [sc.rows_per_lane(tl) for tl in (1, 64, 65, 128, 129, 256, 257, 384, 385, 512)] == [2, 2, 2, 2, 4, 4, 6, 6, 8, 8]
    assert [sc.lanes(tl) for tl in (1, 2, 3, 63, 64, 65, 126, 127, 128, 129, 130)] == [1, 1, 2, 32, 32, 33, 63, 64, 64, 33, 33]
    assert [sc.lanes(tl) for tl in (252, 253, 256, 257, 378, 379, 384, 385, 504, 505, 512)] == [63, 64, 64, 43, 63, 64, 64, 49, 63, 64, 64]
    assert [tl for tl in range(1, 513) if sc.lanes(tl) == 64] == FULL_WAVE
    assert all(0 <= sc.rows_past(tl) < sc.rows_per_lane(tl) and sc.lanes(tl) <= 64 for tl in range(1, 513))
    assert [sc.rows_past(tl) for tl in (127, 253, 379, 505, 506, 511, 512)] == [1, 3, 5, 7, 6, 1, 0]
    # the rows set: every R, both sides of every full-wave edge, odd lengths, 1 .. 7 rows past tl
    assert {sc.rows_per_lane(tl) for tl in sc.ROWS_TL} == {2, 4, 6, 8}
    assert {sc.rows_past(tl) for tl in sc.ROWS_TL} == set(range(8))
    for lo, hi in ((127, 128), (253, 256), (379, 384), (505, 512)):
        assert {lo - 1, lo, hi} <= set(sc.ROWS_TL) and (hi == 512 or hi + 1 in sc.ROWS_TL)
    assert set(sc.RAMPS_TL) == {128, 256, 384, 512, 127, 253, 379, 505} and all(sc.lanes(tl) == 64 for tl in sc.RAMPS_TL)


def test_column_words_are_odd_against_the_lanes_stride():
    """sw_small_pair.h: the lanes of a step, one column apart, are R/2 - CS or R - CS dwords apart, an odd number: 64 different banks;
    a column holds the rows of whole lanes, and small_lds_bytes' bound on it holds for every tl"""
    for tl in range(1, 513):
        r, nl = sc.rows_per_lane(tl), sc.lanes(tl)
        for wide in (False, True):
            cs = sc.column_words(tl, wide)
            assert sc.lane_stride_words(tl, wide) % 2 == 1, (tl, wide)
            assert nl * r // (1 if wide else 2) <= cs <= (tl + 8 if wide else (tl + 7) // 2 + 1), (tl, wide)
    assert [sc.column_words(tl, False) for tl in (1, 128, 256, 384, 512)] == [2, 64, 129, 192, 257]   # (R / 2 = 1, 1, 2, 3, 4)
    assert [sc.column_words(tl, True) for tl in (1, 128, 255, 512)] == [3, 129, 257, 513]


def test_text_cap_base_and_lds():
    assert [sc.text_cap(100, 50, s) for s in (1, 7, 8, 9, 303, 304, 305, 4000)] == [4, 8, 8, 12, 304, 304, 304, 304]
    assert sc.base(256, 150, *[sc.GATK[k] for k in (0, 2, 3)]) == (200 * 150 - 520) // 2
    assert sc.base(3, 2, 1, 40, 0) == -39 and sc.base(3, 3, 1, 40, 0) == -38           # (C division: towards zero)
    assert sc.lds_bytes(256, 150, 64, False) == 132 * 151 * 4 + 256 + 152 + 64 + 8
    assert sc.lds_bytes(256, 150, 64, True) == 264 * 151 * 4 + 256 + 152 + 64 + 8
    assert sc.supported(512, 150, 1328, *sc.GATK) == (True, False) and sc.supported(513, 1, 64, *sc.GATK)[0] is False
    assert sc.supported(20, 12, 64, 1 << 23, 0, 5, 2)[0] is False and sc.supported(20, 12, 64, 5, -3, 1 << 23, 1 << 23)[0] is False


def test_fill_schedule():
    """masked blocks up to step 64, unmasked ones while s0 + 3 <= ql - 1 -- the first at ql = 68 --, CLAMP blocks up to ql + 63; no
    unmasked or CLAMP block without a full wave"""
    for tl in (1, 100, 126, 129, 300, 400, 504):
        for ql in (1, 68, 150):
            sch = sc.fill_schedule(tl, ql)
            assert {f for _, f in sch} == {"masked"} and [s for s, _ in sch] == list(range(0, ql + sc.lanes(tl) - 1, 4))
    count = lambda tl, ql, form: sum(f == form for _, f in sc.fill_schedule(tl, ql))  # noqa: E731
    for tl in sc.RAMPS_TL:
        for ql in range(1, 200):
            sch = sc.fill_schedule(tl, ql)
            assert [s for s, _ in sch] == list(range(0, ql + 63, 4))
            forms = [f for _, f in sch]
            assert forms == sorted(forms, key=("masked", "unmasked", "clamp").index) and forms[:16] == ["masked"] * 16
            assert count(tl, ql, "unmasked") == max(0, (ql - 64) // 4) and count(tl, ql, "masked") == 16
            assert count(tl, ql, "clamp") == len(sch) - 16 - count(tl, ql, "unmasked") and (count(tl, ql, "clamp") > 0) == (ql > 1)
        assert [count(tl, ql, "unmasked") for ql in (63, 64, 67, 68, 71, 72, 75, 76)] == [0, 0, 0, 1, 1, 2, 2, 3]
    assert {count(128, ql, "unmasked") for ql in sc.RAMPS_QL} == {0, 1, 2, 3} and {ql % 4 for ql in sc.RAMPS_QL if ql >= 60} == {0, 1, 2, 3}
    assert set(range(1, 9)) | set(range(60, 77)) == set(sc.RAMPS_QL)
    assert {1, 2, 3, 4, 5, 150} | set(range(63, 73)) == set(sc.ROWS_QL)


def test_the_planner_at_every_fits_edge():
    """mgl_sw_explain (it plans with a CIGAR slot of 64 bytes, as the fits cases run): sw_small_kernel at the largest query length
    the restated small_supported admits, another kernel one past it; the same for one step past the span at 128 x 300, where the
    32-bit form is beyond LDS"""
    sets, report = sc.built()
    seen = set()
    for c in sets["fits"] + sets["span"]:
        on = report["on_kernel"][c.name]
        max_tl, max_ql = max(map(len, c.targets)), max(map(len, c.queries))
        assert (len(c.targets[0]), len(c.queries[0])) == (max_tl, max_ql)
        p = _lib.explain(n=len(c.targets), max_tl=max_tl, max_ql=max_ql, parameters=c.params, strategy=c.strategies[0])
        assert (p.fill_kernel == SMALL) == on, (c.name, p.fill_kernel)
        assert sc.supported(max_tl, max_ql, 64, *c.params)[0] == on, c.name
        if on and c.name.startswith("fits/tl"):
            assert p.rows == sc.rows_per_lane(max_tl)
        seen.add((c.name.split("/")[1], on))
    assert {(f"tl{tl}", on) for tl in sc.FITS_TL for on in (True, False)} <= seen
    edges = {tl: (sc.largest_ql(tl, sc.GATK), sc.largest_ql(tl, sc.WIDE)) for tl in sc.FITS_TL}
    assert edges[256][1] >= 150 > edges[384][1] and edges[512][0] >= 150, edges     # (256 x 150 in 32 bits is the largest of that kind)
    assert {len(c.queries[0]) for c in sets["fits"] if "staging" in c.name} == set(sc.STAGING_QL)


# ---- the restated recurrence and walk

def test_h_matrix_against_the_full_recurrence():
    rng = np.random.default_rng(5)
    pairs = [(b"A" * 40, b"A" * 33), (b"A" * 30, b"C" * 50), (b"ACGT" * 20, b"AC" * 17), (b"G", b"G"), (b"G", b"T")]
    pairs += [(sc._b(sc._rand(rng, int(rng.integers(1, 90)), sc._ALPHA[:2])), sc._b(sc._rand(rng, int(rng.integers(1, 90)), sc._ALPHA[:2]))) for _ in range(12)]
    for params in (sc.GATK, sc.UNIT, (5, -4, 10, 1), (3, -3, 0, 0), sc.WIDE):
        for strategy in sc.STRATEGIES:
            for t, q in pairs:
                H, _ = sc.h_matrix(t, q, params, strategy)
                assert np.array_equal(H, rg.dp_full(t, q, params, strategy)[0]), (t, q, params, strategy)
                assert sc.score_max(H) == rg.score_max(H)


@pytest.mark.parametrize("name", SETS)
def test_the_walk_restatement_is_the_oracle_s(name):
    """offset, CIGAR and ScoreMax of walk() against the oracle on every pair of the set under every strategy it runs with: walk() can
    be trusted as the definition the tie checks below switch rules in"""
    n = 0
    for k, c in enumerate(sc.cases(name)):
        hs = {}
        for strategy in c.strategies:
            off, score, cg = oracle(name, k, strategy)
            for p, (t, q) in enumerate(zip(c.targets, c.queries)):
                border = strategy in (sc.INDEL, sc.LEADING_INDEL)
                if (p, border) not in hs:
                    hs[p, border] = sc.h_matrix(t, q, c.params, strategy)
                got = sc.walk(t, q, c.params, strategy, HS=hs[p, border])
                assert got == (int(off[p]), cg[p], tuple(int(x) for x in score[p])), (c.name, p, strategy, c.intent[p])
                assert name == "slots" or len(cg[p]) <= c.cigar_stride, (c.name, p, strategy)      # (only the slots set is to overflow)
                n += 1
    assert n >= len(sc.cases(name))


# ---- every case does what it says

def test_every_batch_has_its_anchor():
    sets, report = sc.built()
    for name in SETS:
        assert sets[name], name
        for c in sets[name]:
            assert c.intent[0].kind == "anchor" and len(c.targets) >= 2
            assert (len(c.targets[0]), len(c.queries[0])) == (max(map(len, c.targets)), max(map(len, c.queries))), c.name
            on = report["on_kernel"].get(c.name, True)
            assert sc.supported(len(c.targets[0]), len(c.queries[0]), c.cigar_stride, *c.params)[0] == on, c.name


def test_rows():
    cs, left = sc.cases("rows"), sc.built()[1]["rows_left"]
    # what LDS does not admit: 150 bases in 32 bits against more than 257 rows, and nothing else
    assert left and all(ql == 150 and wide and tl > 257 for tl, ql, wide in left)
    for form, params in (("narrow", sc.GATK), ("wide", sc.WIDE)):
        mine = [c for c in cs if f"/{form}/" in c.name]
        assert all(c.params == params and sc.supported(len(c.targets[0]), len(c.queries[0]), c.cigar_stride, *params)[1] == (form == "wide") for c in mine)
        seen = {(len(t), len(q), it.kind) for c in mine for t, q, it in zip(c.targets[1:], c.queries[1:], c.intent[1:])}
        for tl in sc.ROWS_TL:
            for ql in sc.ROWS_QL:
                if (tl, ql, form == "wide") not in left:
                    assert {(tl, ql, kind) for kind in ("identical", "substitution", "unrelated")} <= seen, (form, tl, ql)
    for c in cs:            # the substitutions: the last row of a lane, the first row of a lane
        rows = [(len(t), it.row) for t, it in zip(c.targets, c.intent) if it.kind == "substitution"]
        for (tl, last), (_, first) in zip(rows[0::2], rows[1::2]):
            r = sc.rows_per_lane(tl)
            assert (last % r == 0 or last == tl) and (first - 1) % r == 0, (tl, last, first)
    k = next(k for k, c in enumerate(cs) if c.name.startswith("rows/narrow/ql70"))
    off, score, cg = oracle("rows", k, sc.SOFTCLIP)
    for p, it in enumerate(cs[k].intent):
        if it.kind == "identical" and len(cs[k].targets[p]) >= 70:
            assert cg[p] == "70M" and off[p] == len(cs[k].targets[p]) - 70


def test_ramps():
    cs = sc.cases("ramps")
    seen = set()
    for k, c in enumerate(cs):
        _, score, _ = oracle("ramps", k, sc.SOFTCLIP)
        for p, it in enumerate(c.intent[1:], 1):
            assert sc.intent_met(c, p, score[p]) is True, (c.name, p, it, tuple(score[p]))
            seen.add((c.name.split("/")[1], len(c.targets[p]), len(c.queries[p]), it.kind))
    for tl in sc.RAMPS_TL:
        for ql in sc.RAMPS_QL:
            assert ("narrow", tl, ql, "last_column") in seen and (ql < 2 or ("narrow", tl, ql, "last_row") in seen)
            assert (("wide", tl, ql, "last_column") in seen) == sc.supported(tl, ql, sc.full_stride(tl, ql), *sc.WIDE)[0]
    assert ("wide", 512, 76, "last_row") in seen and ("wide", 505, 76, "last_column") in seen


def test_runs_and_their_intent_cap():
    """every gap length against every diagonal stretch, in front of it and behind it; the oracle's path under the strategy a run is
    judged by holds exactly that run between exactly those stretches, on the row it was placed on; at most 2 % of the pairs drawn
    may have failed that and been dropped"""
    sets, report = sc.built()
    assert report["runs_made"] == 2 * 3 * 2 * len(sc.RUN_GAPS) * len(sc.RUN_DIAGS)
    assert report["runs_dropped"] <= 0.02 * report["runs_made"], report
    seen = set()
    for k, c in enumerate(sets["runs"]):
        off, _, cg = oracle("runs", k, sc.RUN_JUDGE[c.params])
        for p, it in enumerate(c.intent[1:], 1):
            assert sc.run_intent_met((c.targets[p], c.queries[p], it), cg[p], off[p]), (c.name, p, it, cg[p])
            r = sc.rows_per_lane(len(c.targets[p]))
            if it.kind == "del_start":
                assert it.row % r == 0
            if it.kind == "del_end":
                assert (it.row + it.n - 1) % r == 1
            seen.add((c.params, it.kind, it.n, it.d))
    want = {(params, kind, n, d) for params in sc.RUN_PARAMS for kind in ("del_start", "del_end", "ins") for n in sc.RUN_GAPS
            for x in sc.RUN_DIAGS for d in ((x, sc.RUN_FLANK), (sc.RUN_FLANK, x))}
    assert len(want - seen) == report["runs_dropped"] and seen <= want
    assert {it.col for c in sets["runs"] for it in c.intent if it.kind == "ins"} >= {64, 65, 66, 128, 129, 130, 193}   # the run's first column
    assert all(c.strategies == sc.STRATEGIES for c in sets["runs"])


def test_round_ties():
    """the search's pairs: a later round of 64 gap candidates has to win the tie, or the CIGAR changes; every parameter set has one"""
    cs = sc.cases("round_ties")
    assert {c.params for c in cs} == set(sc.TIE_PARAMS)
    early = sc.RULES._replace(later_round=False)
    for c in cs:
        t, q, (strategy,) = c.targets[1], c.queries[1], c.strategies
        assert len(t) <= 40 and len(q) <= 200
        o = ol.oracle_align(t, q, c.params, strategy)
        right, wrong = sc.walk(t, q, c.params, strategy), sc.walk(t, q, c.params, strategy, early)
        assert right[:2] == (o["offset"], o["cigar"]) and wrong[:2] != right[:2], c.name
        assert max(n for n, op in sc.elements(right[1]) if op in "ID") > 64
    assert sc.ROUND_TIE_BUDGET * 2 * len(sc.TIE_PARAMS) <= sc.ROUND_TIE_LIMIT


def test_last_cell_ties():
    """every rule of the two passes has, at every shape, a pair whose ScoreMax the opposite rule gets wrong, and rd <, ==, > |mqe_t -
    ql| each have a pair whose last row and last column hold the same best score in different cells"""
    sets, report = sc.built()
    assert not report["ties_missing"], report["ties_missing"]
    for k, c in enumerate(sets["last_cell_ties"]):
        _, score, _ = oracle("last_cell_ties", k, sc.SOFTCLIP)
        flips, orders = set(), set()
        for p, it in enumerate(c.intent[1:], 1):
            H, _ = sc.h_matrix(c.targets[p], c.queries[p], c.params, sc.SOFTCLIP)
            assert sc.score_max(H) == tuple(int(x) for x in score[p])
            assert sc.intent_met(c, p, score[p], H) is True, (c.name, p, it)
            flips |= sc.tie_flips(H)
            orders.add(sc.tie_order(H))
        assert flips == set(sc.TIE_RULES) and orders >= set(sc.TIE_ORDERS), (c.name, flips, orders)
    assert {len(c.targets[1]) for c in sets["last_cell_ties"]} == set(sc.TIE_TL) and sc.lanes(sc.TIE_TL[0]) == 64 and sc.lanes(sc.TIE_TL[1]) == 64


def test_bytes():
    cs = sc.cases("bytes")
    assert {sc.rows_per_lane(len(c.targets[1])) for c in cs} == {2, 4, 6, 8}
    for byte, shares in sc.SHARES:
        assert sc.code_bits(byte) == sc.code_bits(shares) and bytes([byte]) not in (b"A", b"C", b"G", b"T")
    assert [sc.code_bits(b) for b in b"ACTG"] == [0, 1, 2, 3]
    for k, c in enumerate(cs):
        _, score, _ = oracle("bytes", k, sc.SOFTCLIP)
        kinds = [it.kind for it in c.intent]
        assert kinds.count("query_byte") == 8 and kinds.count("target_n") == 6 and {"lower_both", "lower_target", "high_equal", "high_unequal", "high_target"} <= set(kinds)
        for p, it in enumerate(c.intent):
            t, q = c.targets[p], c.queries[p]
            tl, lo = len(t), (len(t) - sc.BYTES_QL) // 2
            if it.kind == "query_byte":
                assert set(t) <= set(b"ACGT") and [sc.block_step(lo + j, j, tl) for j in it.col] == [0, 3]
                assert all(q[j - 1] == it.row and sc.code_bits(t[lo + j - 1]) == sc.code_bits(it.row) for j in it.col)
                # two mismatches on an else perfect diagonal: what a byte taken for the base it shares a code with would hide
                assert int(score[p][2]) == c.params[0] * (sc.BYTES_QL - 2) + 2 * c.params[1]
            if it.kind == "target_n":
                assert t.count(b"N") == 1 and t[it.row - 1:it.row] == b"N" and (q.count(b"N") == it.col)
                assert int(score[p][2]) == c.params[0] * sc.BYTES_QL - (0 if it.col else c.params[0] - c.params[1])
            if it.kind in ("lower_both", "high_equal"):
                assert int(score[p][2]) == c.params[0] * sc.BYTES_QL
            if it.kind in ("lower_target", "high_target"):
                assert int(score[p][0]) < 0
            if it.kind.startswith("high"):
                assert min(t) >= 0x80 and (it.kind == "high_target" or min(q) >= 0x80)


def test_span():
    assert sc.span_edge(256, 150, (400, -300, 400, 5), 2) == (400, -300, 470, 5) and rg.small_span(256, 150, 400, -300, 470, 5) == 65000
    for c in sc.cases("span"):
        tl, ql = len(c.targets[0]), len(c.queries[0])
        fits = rg.small_fits_int16(tl, ql, *c.params)
        assert fits == c.name.endswith("edge") and (fits or rg.small_fits_int16(tl, ql, *rg.past(c.params, 2 if tl == 256 else 0, -1)))
        assert {len(t) for t in c.targets} == {tl, tl - 3} and set(c.strategies) == {sc.SOFTCLIP, sc.INDEL}
        assert [it.kind for it in c.intent[1:]] == ["all_match", "all_mismatch", "half", "half"] * 2


def test_slots():
    cs, lengths = sc.cases("slots"), sc.built()[1]["slot_lengths"]
    assert len(lengths) >= 3
    assert {c.cigar_stride for c in cs} == {L + d for L in lengths for d in (-1, 0, 1, 3)} | {7, 9, 513}
    assert any(c.cigar_stride % 4 for c in cs) and any(c.cigar_stride % 4 == 0 for c in cs)
    _, _, cg = oracle("slots", 0, sc.SOFTCLIP)
    assert sorted({len(x) for x in cg[1:]}) == lengths


def test_the_one_pair_subset():
    sub = sc.service_subset()
    assert 100 <= len(sub) <= 200
    assert {sc.rows_per_lane(len(t)) for t, _, _, _, _ in sub} == {2, 4, 6, 8}
    assert {w.split("/")[0] for _, _, _, _, w in sub} == set(SETS) - {"slots"}
    t, q, params, _, _ = sub[-1]
    assert sc.lds_bytes(len(t), len(q), sc.full_stride(len(t), len(q)), not rg.small_fits_int16(len(t), len(q), *params)) > 64 * 1024
