"""tests/calls_textbook.py against a second, independent statement of each rule and against cases worked by hand: the insertion table
against one built from the alignments expanded to columns; the events of a site list against maximal runs and per-length tallies; the
genotype against exact rational arithmetic and the figures of the issue (depth 16 at Q = 20)."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import calls_cases as cc  # noqa: E402
import calls_textbook as ctb  # noqa: E402
import describe_cases as dc  # noqa: E402
import pileup_cases as pc  # noqa: E402
import pileup_textbook as ptb  # noqa: E402


# ---- the second statements

def insertions_by_columns(alignments, region_beg, sites, max_ins):
    """every alignment expanded to columns (element, target position or None, query byte); the inserted columns of one element are
    gathered as one string at the last target position in front of them; then the strings are tallied per position"""
    strings = {}
    for pos, query, cigar in alignments:
        cols, t, j = [], pos, 0
        for e, (n, op) in enumerate(cigar):
            for _ in range(n):
                cols.append((e, t if op != "I" else None, query[j] if op != "D" else None))
                t, j = t + (op != "I"), j + (op != "D")
        last, found = pos - 1, {}
        for e, t, b in cols:
            if t is None:
                found.setdefault(e, [last, bytearray()])[1].append(b)
            else:
                last = t
        for at, s in found.values():
            strings.setdefault(at - region_beg, []).append(bytes(s))
    table = []
    for site in sites:
        row = [0] * (6 * max_ins + 1)
        for s in strings.get(site[0], []):
            if len(s) > max_ins:
                row[0] += 1
                continue
            row[len(s)] += 1
            for j, b in enumerate(s):
                row[max_ins + 1 + 5 * j + "ACGT".find(chr(b).upper() if chr(b).upper() in "ACGT" else "?") % 5] += 1
        table.append(row)
    return table


def exact_genotype(r, a, costs):
    """the likelihoods as exact fractions of a phred: PL = floor(x + 1/2) of the difference to the best, the clip, and the ranks"""
    cm, ch, ce = costs
    lik = [Fraction(r * cm + a * ce, 256), Fraction((r + a) * ch, 256), Fraction(a * cm + r * ce, 256)]
    best = min(lik)
    pl = [min(int(x - best + Fraction(1, 2)), 2 ** 31 - 1) for x in lik]
    gt = min(g for g in range(3) if lik[g] == best)
    return gt, min([99] + [pl[g] for g in range(3) if g != gt]), pl[0], tuple(pl)


def events_by_runs(t, n_sites=None):
    """the (pos, kind, len, flags) of a table's calls stated over maximal runs: the active sites are cut into maximal runs of deletion
    sites at consecutive positions; a run gives ONE call at its first site, as long as the run and at most max_del"""
    n = t.n_sites if n_sites is None else n_sites
    sites = t.sites[:min(max(n, 0), len(t.sites))]
    length = len(t.counts[0])
    run_at, s = {}, 0
    while s < len(sites):
        if not sites[s].flags & 4:
            s += 1
            continue
        e = s
        while e + 1 < len(sites) and sites[e + 1].flags & 4 and sites[e + 1].pos == sites[e].pos + 1:
            e += 1
        run_at[s] = e - s + 1
        s = e + 1
    out = []
    for s, x in enumerate(sites):
        if not 0 <= x.pos < length:
            continue
        if x.flags & 2 and t.ref[x.pos:x.pos + 1].upper() in (b"A", b"C", b"G", b"T") and x.alt in (0, 1, 2, 3):
            out.append((x.pos, 1, 1, 0))
        if s in run_at:
            out.append((x.pos, 2, min(run_at[s], t.max_del), int(run_at[s] > t.max_del)))
        if x.flags & 8 and t.ins is not None:
            words = t.ins[s][1:t.max_ins + 1]
            if max(words) > 0:
                out.append((x.pos, 3, 1 + words.index(max(words)), 0))
    return out


# ---- the insertion table

def flat(cases, t_start=None):
    starts = np.cumsum([0] + [len(c.t) for c in cases[:-1]]) if t_start is None else t_start
    return pc.alignments(cases, [int(s) for s in starts])


def test_insertions_against_columns_on_random_alignments():
    rng = np.random.default_rng(21)
    cases = [dc.case(*dc.random_alignment(rng, 9, b"ACGTNacgt", max_len=6)) for _ in range(40)]
    als = flat(cases)
    total = sum(len(c.t) for c in cases)
    assert sum(op == "I" for _, _, cg in als for _, op in cg) > 40
    for region_beg, max_ins in ((0, 1), (0, 3), (17, 6), (0, 64)):
        sites = [cc.site(p) for p in range(-1, total - region_beg) if p % 3 != 1]
        want = insertions_by_columns(als, region_beg, sites, max_ins)
        assert ctb.insertions(als, region_beg, sites, max_ins) == want
        assert any(r[0] for r in want) == (max_ins < 6) and any(any(r[1:]) for r in want)
    with pytest.raises(ValueError):
        ctb.insertions(als, 0, [], 0)
    with pytest.raises(ValueError):
        ctb.insertions(als, 0, [], 65)


def test_insertions_hand_worked():
    # 4M 2I 4M at position 10: the insertion "gN" stands behind position 13; and a leading I behind position 9
    als = [(10, b"ACGTgNACGT", [(4, "M"), (2, "I"), (4, "M")]), (10, b"TTTACGT", [(3, "I"), (4, "M")]), (10, b"ACGTCACGT", [(4, "M"), (1, "I"), (4, "M")])]
    sites = [cc.site(4), cc.site(8, 0), cc.site(50)]
    got = ctb.insertions(als, 5, sites, 2)                     # W = 13: word 0, lengths 1 and 2, two columns of five channels
    assert got == [[1] + [0] * 12,                             # TTT is longer than max_ins: word 0 and no column
                   [0, 1, 1] + [0, 1, 1, 0, 0] + [0, 0, 0, 0, 1],    # C | g, N: the site's flags do not matter
                   [0] * 13]
    again = ctb.insertions(als, 5, sites, 2, got)
    assert again is got and got[1][:3] == [0, 2, 2]
    got[0][0] = ptb.MASK
    assert ctb.insertions(als[1:2], 5, sites, 2, got)[0][0] == 0   # modulo 2^32


def test_the_shared_insertion_cases_hold_what_they_promise():
    rng = np.random.default_rng(22)
    for k in cc.SITE_LIST_SIZES:
        cases, sites = cc.site_list_case(rng, k)
        assert len(sites) == k and [s.pos for s in sites] == sorted({s.pos for s in sites})
        got = ctb.insertions(flat(cases), 0, sites, 8)
        assert got == insertions_by_columns(flat(cases), 0, sites, 8)
        assert sum(sum(r[:9]) for r in got) == min(k, 3)
        if k >= 3:
            at = [s.pos for s in sites].index(cc.MIDDLE)
            assert got[0][3] == 1 and got[at][2] == 1 and got[-1][4] == 1 and 0 < at < k - 1
    for max_ins in (1, 64):
        cases, sites = cc.length_cases(rng, max_ins)
        got = ctb.insertions(flat(cases), 0, sites, max_ins)
        assert got == insertions_by_columns(flat(cases), 0, sites, max_ins)
        assert sum(r[0] for r in got) == 1 and sum(r[max_ins] for r in got) >= 2 and got[-1][1] == 1
    for binary in (False, True):
        cases, sites = cc.seam_case(rng, binary)
        assert len(cases[0].cigar) == 1100 and [op for _, op in cases[0].cigar[62:67]] == ["I"] * 5 == [op for _, op in cases[0].cigar[510:515]]
        got = ctb.insertions(flat(cases), 0, sites, 3)
        assert got == insertions_by_columns(flat(cases), 0, sites, 3) and sum(sum(r[:4]) for r in got) == 10
    cases, sites = cc.odd_bytes_case()
    row = ctb.insertions(flat(cases), 0, sites, 16)[0]
    assert row[16] == 1 and [row[17 + 5 * j:22 + 5 * j].index(1) for j in range(16)] == [0, 1, 2, 3, 4, 4, 4, 4, 4, 4, 4, 4, 0, 1, 2, 3]


# ---- the genotype

def test_genotype_costs():
    from mgl_amd import smithwaterman as sw

    c = sw.genotype_costs(20)
    assert tuple(c) == (11, 6341, 778) and (c.cost_match, c.cost_error, c.cost_het) == (11, 6341, 778) and sw.genotype_costs() == c
    assert ctb.genotype_costs(20) == cc.Q20 == (11, 778, 6341)
    for q in (3, 10, 20, 30, 37, 60):
        cm, ch, ce = ctb.genotype_costs(q)
        assert (cm, ch, ce) == ctb.phred_costs(q) and 1 <= cm < ch < ce <= 1 << 20, q
    assert ctb.genotype_costs(60)[0] == 1                     # -2560 log10(1 - 1e-6) rounds to 0: the floor of 1


def test_genotypes_worked_by_hand():
    for r, a, costs, gt, pl, gq in cc.GENOTYPES:
        assert ctb.genotype(r, a, costs) == (gt, gq, pl[0], pl) == exact_genotype(r, a, costs), (r, a, costs)
    # the issue's figures spelled out: r = a = 8 at Q = 20
    l0, l1 = 8 * 11 + 8 * 6341, 16 * 778
    assert (l0, l1) == (50816, 12448) and (l0 - l1 + 128) // 256 == 150
    assert (16 * 6341 - 16 * 11 + 128) // 256 == 396 and (16 * 778 - 16 * 11 + 128) // 256 == 48
    assert [g[5] for g in cc.GENOTYPES[-3:]] == [98, 99, 99] and [g[4][1] for g in cc.GENOTYPES[-3:]] == [98, 99, 100]


def test_genotype_against_exact_arithmetic():
    rng = np.random.default_rng(23)
    for _ in range(3000):
        r, a = (int(rng.integers(0, 1 << int(rng.integers(1, 33)))) for _ in range(2))
        cm = int(rng.integers(1, 1 << int(rng.integers(1, 19))))
        ch = cm + int(rng.integers(1, 1 << 18))
        ce = min(ch + int(rng.integers(1, 1 << 19)), 1 << 20)
        assert ctb.genotype(r, a, (cm, ch, ce)) == exact_genotype(r, a, (cm, ch, ce)), (r, a, cm, ch, ce)
    for bad in ((0, 1, 2), (1, 1, 2), (1, 2, 2), (3, 2, 1), (1, 2, (1 << 20) + 1)):
        with pytest.raises(ValueError):
            ctb.check(4, 4, bad)
    for max_ins, max_del in ((0, 1), (65, 1), (1, 0), (1, 4097)):
        with pytest.raises(ValueError):
            ctb.check(max_ins, max_del, cc.Q20)
    ctb.check(1, 1, (1, 2, 3)), ctb.check(64, 4096, (1 << 20) - 2 + np.arange(3))


# ---- the events

def shape(calls):
    return [(c.pos, c.kind, c.len, c.flags) for c in calls]


def test_each_kind_alone_and_together():
    t = cc.kinds_table()
    calls, rows = cc.calls_textbook(t)
    assert shape(calls) == events_by_runs(t) == [(3, 1, 1, 0), (7, 2, 1, 0), (11, 3, 2, 0), (15, 1, 1, 0), (15, 2, 1, 0), (15, 3, 2, 0), (23, 2, 1, 0), (35, 1, 1, 0)]
    by = {(c.pos, c.kind): (c, r) for c, r in zip(calls, rows)}
    c = by[3, 1][0]
    assert (c.ref, c.alt, c.depth, c.ref_count, c.alt_count, c.gt, c.pl0, c.pl1, c.pl2, c.gq, c.qual, c.reserved) == (0, 1, 16, 8, 8, 1, 150, 0, 150, 99, 150, 0)
    c = by[7, 2][0]
    assert (c.ref, c.alt, c.depth, c.ref_count, c.alt_count, c.gt) == (0, -1, 16, 8, 8, 1)
    c, r = by[11, 3]
    assert (c.ref, c.alt, c.depth, c.ref_count, c.alt_count, c.gt, r) == (0, -1, 16, 7, 9, 1, b"CT\0\0")   # r = depth - the insertions
    assert [(by[15, k][0].ref_count, by[15, k][0].alt_count) for k in (1, 2, 3)] == [(2, 6), (2, 8), (9, 7)] and by[15, 3][1] == b"AN\0\0"
    c = by[23, 2][0]
    assert (c.ref, c.ref_count, c.alt_count) == (4, 5, 7)     # an N reference counts plane 4
    assert (by[35, 1][0].ref, by[35, 1][0].alt, by[35, 1][0].ref_count) == (3, 0, 8)
    assert all(r == bytes(4) for (p, k), (c, r) in by.items() if k != 3)
    # without the table of insertions there is no insertion call and everything else stands
    none, _ = cc.calls_textbook(t._replace(ins=None))
    assert none == [c for c in calls if c.kind != 3]


def test_deletion_runs():
    t = cc.runs_table(5)
    calls, _ = cc.calls_textbook(t)
    assert shape(calls) == events_by_runs(t)
    assert [(c.len, c.flags) for c in calls if c.kind == 2] == [(1, 0), (2, 0), (5, 0), (5, 1), (5, 1), (2, 0), (2, 0), (2, 0), (2, 0), (2, 0)]
    assert all((c.ref_count, c.alt_count) in ((4, 12), (4, 8)) for c in calls if c.kind == 2)   # the counts of the run's FIRST position
    whole, _ = cc.calls_textbook(t, len(t.sites))
    assert [c.len for c in whole][-1] == 4 and shape(whole) == events_by_runs(t, len(t.sites))
    for n in range(len(t.sites) + 1):                         # the run is cut wherever the active sites end
        assert shape(cc.calls_textbook(t, n)[0]) == events_by_runs(t, n)
    for max_del in (1, 2, 4, 6, 11, 12):
        u = t._replace(max_del=max_del)
        assert shape(cc.calls_textbook(u)[0]) == events_by_runs(u)
    t = cc.block_seam_table()
    calls, rows = cc.calls_textbook(t)
    assert shape(calls) == events_by_runs(t) and len(calls) == 600 + 1 + 3
    assert [(c.pos, c.len) for c in calls if c.kind == 2] == [(500, 11)] and [c.pos for c in calls if c.kind == 3] == [505, 506, 1198]


def test_insertion_lengths_and_columns_on_ties():
    t = cc.insertion_ties_table()
    calls, rows = cc.calls_textbook(t)
    assert shape(calls) == events_by_runs(t) == [(2, 3, 2, 0), (4, 3, 3, 0), (8, 3, 4, 0), (10, 3, 1, 0), (12, 3, 2, 0)]
    assert rows == [b"CT\0\0", b"TGC\0", b"AAAA", b"A\0\0\0", b"NT\0\0"]
    assert [(c.ref_count, c.alt_count, c.depth) for c in calls] == [(6, 5, 16), (6, 7, 16), (6, 10, 16), (0, ptb.CLIP, 3), (0, 9, 16)]
    assert calls[3].gt == 2 and calls[3].pl0 == ptb.CLIP


def test_genotypes_in_tables_and_n_sites():
    for t, rows in cc.genotype_tables():
        calls, _ = cc.calls_textbook(t)
        assert [(c.gt, (c.pl0, c.pl1, c.pl2), c.gq, c.qual) for c in calls] == [(g[3], g[4], g[5], g[4][0]) for g in rows]
        assert [(c.ref_count, c.alt_count) for c in calls] == [(min(g[0], ptb.CLIP), min(g[1], ptb.CLIP)) for g in rows]
        assert cc.calls_textbook(t, 0) == ([], []) and cc.calls_textbook(t, -3) == ([], []) and cc.calls_textbook(t, 1 << 40) == (calls, _)
