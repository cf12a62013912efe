"""The generators of tests/local_cases.py produce what they claim -- no GPU: measured with the textbook (tests/local_textbook.py)
alone, so that the GPU tests built on them (tests/test_gpu_local_edges.py) cannot become vacuous unnoticed."""
import local_cases as lc
import local_textbook as lt


def test_generators_are_deterministic():
    assert lc.tied_pairs() == lc.tied_pairs() and lc.walk_tie_pairs() == lc.walk_tie_pairs()
    assert lc.seam_gap_pairs(64) == lc.seam_gap_pairs(64) and lc.seam_gap_pairs(32) != lc.seam_gap_pairs(64)
    a, b = lc.guard_edge_tiles(), lc.guard_edge_tiles()
    assert [(x[6], x[7]) for x in a] == [(x[6], x[7]) for x in b] and all((x[5] == y[5]).all() for x, y in zip(a, b))


def test_tied_pairs_tie_in_the_end_cell():
    pairs = lc.tied_pairs()
    lens = {len(p[0]) for p in pairs}
    assert {63, 64, 65, 127, 128, 129} <= lens and {p[2] for p in pairs} == {"dna1", "dna23"}
    strips = rows = crossed = 0
    for t, q, key, o, e in pairs:
        code, mat = lc.scoring(key)
        cells, two_strips, one_row, cross = lc.end_ties(t, q, code, mat, o, e)
        assert cells >= 8, (t, q, cells)
        strips += two_strips
        rows += one_row
        crossed += cross
    assert strips >= 10 and rows >= 10 and crossed >= 10, (strips, rows, crossed)


def test_end_ties_measures_what_it_says():
    code, mat = lt.dna_matrix(1, -1)
    assert lc.end_ties(b"CCGG", b"GGCC", code, mat, 9, 9) == (2, False, False, True)   # (2, 4) and (4, 2)
    assert lc.end_ties(b"CCGG", b"CCGG", code, mat, 9, 9) == (1, False, False, False)
    assert lc.end_ties(b"A", b"AA", code, mat, 9, 9) == (2, False, True, False)
    assert lc.end_ties(b"AAA", b"A", code, mat, 9, 9, rows=2) == (3, True, False, False)
    assert lc.end_ties(b"CG", b"CCG", code, mat, 9, 9)[3] is False                    # (1, 1), (1, 2), (2, 3): columns grow with rows


def test_walk_tie_pairs_tie_in_the_walk():
    pairs = lc.walk_tie_pairs()
    assert {(o, e) for _, _, _, o, e in pairs} >= {(1, 1), (0, 0), (2, 2)} and all(o == e or o == 0 for _, _, _, o, e in pairs)
    df = fe = oe = 0
    for t, q, key, o, e in pairs:
        code, mat = lc.scoring(key)
        a, b, c = lc.walk_ties(t, q, code, mat, o, e)
        df += a > 0
        fe += b > 0
        oe += c > 0
    assert df >= 20 and fe >= 20 and oe >= 20, (df, fe, oe)


def test_seam_gap_pairs_cross_the_seams():
    for rows in (64, 32):
        pairs = lc.seam_gap_pairs(rows)
        assert {(o, e) for _, _, _, o, e, _ in pairs} == {(2, 0), (2, 1), (11, 0), (11, 1)}
        assert len({t for t, *_ in pairs}) == 4  # one target per gap model: the pairs of a model form a tile
        dels = straddle = long_i = 0
        for t, q, key, o, e, kind in pairs:
            code, mat = lc.scoring(key)
            sc, tb, te, qb, qe, cg = lt.local_align_np(t, q, code, mat, o, e)
            if kind == "D":
                dels += 1
                straddle += lc.d_run_straddles(cg, tb, rows)
            else:
                long_i += lc.longest_i_run(cg) > 64
        assert dels >= 40 and straddle >= 0.9 * dels and long_i >= 10, (rows, dels, straddle, long_i)
    assert lc.cigar_runs("3M2D1I4M", 10) == [("M", 3, 11, 13), ("D", 2, 14, 15), ("I", 1, 15, 15), ("M", 4, 16, 19)]
    assert lc.d_run_straddles("60M5D9M", 0, 64) and lc.d_run_straddles("63M2D9M", 0, 64)
    assert not lc.d_run_straddles("64M5D9M", 0, 64) and not lc.d_run_straddles("59M5D9M", 0, 64) and not lc.d_run_straddles("60M5I9M", 0, 64)


def test_guard_edge_tiles_sit_on_the_guard():
    tiles = lc.guard_edge_tiles()
    assert [(x[0], x[1], x[2], x[3] - x[2]) for x in tiles] == [(s, m, L, d) for s, m, L in lc.GUARD_EDGES for d in (0, 1, 3)]
    assert lc.GUARD_EDGES == ((-128, 127, 514), (-8, 120, 544)) and 127 * 514 + 255 == 65533 and 120 * 544 + 255 == 65535
    for smin, smax, L, length, code, mat, t, qs in tiles:
        assert int(mat.min()) == smin and int(mat.max()) == smax and len(t) == length and len(qs) == 128
        assert lt.local_lane_ok(smin, smax, 11, 1, length, length) == (length == L)
        assert smax * (L + 3) > 65535 >= smax * (L + 1)  # L + 3: the first length whose score itself leaves 16 bits
        want = lt.local_scores_np(t, qs, code, mat, 11, 1)
        for slot in (lc.SLOT_LOW, lc.SLOT_HIGH, lc.SLOT_BOTH, lc.SLOT_BOTH + 1):
            assert qs[slot] == t and want[slot] == smax * length
        assert want[lc.SLOT_LOW + 1] == 0 and want[lc.SLOT_HIGH - 1] == 0 and lc.SLOT_LOW % 2 == 0 and lc.SLOT_HIGH % 2 == 1
        assert want[60] == 0 and qs[60] == b"" and (want > 0).sum() >= 120
