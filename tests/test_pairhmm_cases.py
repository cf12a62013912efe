"""What the constructed PairHMM cases (pairhmm_cases.py) reach, checked without a GPU: every kernel instantiation and
every rows-per-lane variant of pairhmm_kernels.hip according to variant(), which mirrors the host's choice; rescue cases
clear of MIN_ACCEPTED on both sides; the border columns carrying the sum; sizes.  test_gpu_pairhmm_edges.py runs the
same cases on the device."""
import numpy as np
import pytest

import pairhmm_cases as pc
import pairhmm_oracle_lib as pol

# The seam grids as the kernels' seams dictate them: read lengths around every multiple of the group width G up to G Kmax
# (and, on 64 lanes, the first reads of two and of three stripes), and the first read beyond what 21 and 32 lanes take.
TABLE = {
    16: (1, 2, 15, 16, 17, 31, 32, 33, 48, 49),
    21: (1, 2, 20, 21, 22, 41, 42, 43, 62, 63, 64, 83, 84, 85, 104, 105, 106),
    32: (1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 159, 160, 161),
    64: (1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 258, 511, 512, 513),
}
ALL_FLOAT = {("pairhmm_float_kernel", 0)} | {("pairhmm_float%d_kernel" % g, k) for g in (21, 32) for k in (4, 5)} | \
            {("pairhmm_float64_kernel", k) for k in (1, 2, 3, 4)}
ALL_DOUBLE = {("pairhmm_double_kernel", 0)} | {("pairhmm_double64_kernel", k) for k in (1, 2, 3, 4)}


def _orders(rows, call):
    c = pc.grid_call(rows, call)
    p = pc.permuted(c)
    return [c, p] + pc.cuts(p, rows)


def _reach(rows, use_double):
    """{(kernel, KMAX)} and {(lanes, K)} over every call and order of one grid."""
    kernels, ks = set(), set()
    for call in range(len(pc.GRID_CALL_MAX[rows])):
        for c in _orders(rows, call):
            v = pc.variant(c.n, c.max_read, c.max_hap, rows, use_double, c.R)
            if not use_double:
                kernels.add((v.float_kernel, v.float_kmax))
                ks |= {(v.float_rows, k) for k in v.float_k}
            else:
                kernels.add((v.double_kernel, v.double_kmax))
                ks |= {(v.double_rows, k) for k in v.double_k}
    return kernels, ks


def test_grids_hold_the_table():
    assert pc.GRID_R == TABLE
    for rows, rs in TABLE.items():
        g = pc.grid(rows)
        hs = (1, 2, 3, 4, 5, 7, 8, 9, rows - 1, rows, rows + 1, rows + 7, rows + 8, rows + 9, 2 * rows + 1)
        cells = sorted(zip(g.R.tolist(), g.H.tolist(), g.kind))
        assert cells == sorted((r, h, k) for r in rs for h in hs for k in ("prefix", "suffix"))
        # the calls together hold every pair, and the R-major order gives the groups of a wave one read length
        seen = np.concatenate([pc.grid_call(rows, c).idx for c in range(len(pc.GRID_CALL_MAX[rows]))])
        assert set(seen.tolist()) == set(range(g.n))
        assert (np.diff(g.R) >= 0).all()
        pw = 64 // rows
        p = pc.permuted(g)
        mixed_waves = sum(len(set(p.R[w:w + pw].tolist())) > 1 for w in range(0, p.n, pw))
        assert pw == 1 or mixed_waves > 0.8 * (p.n // pw)
        for m, c in enumerate(pc.cuts(p, rows), 1):
            assert c.n % pw == m and c.n > p.n - 2 * pw


@pytest.mark.parametrize("rows", [16, 21, 32, 64])
def test_each_grid_reaches_its_instantiations(rows):
    """The third column of the table: without this grid's row the instantiations below are not launched by any grid."""
    fk, fks = _reach(rows, False)
    dk, dks = _reach(rows, True)
    if rows == 16:
        assert fk == {("pairhmm_float_kernel", 0)} and dk == {("pairhmm_double_kernel", 0)}
        assert fks == {(16, 1)} and dks == {(16, 1)}
        # reads of one, two, three and four stripes of 16 rows
        assert {-(-int(r) // 16) for r in pc.grid(16).R} == {1, 2, 3, 4}
    elif rows in (21, 32):
        name = "pairhmm_float%d_kernel" % rows
        # the read beyond rows x 5 falls back to one pair per wave (pairhmm_capi.cpp:192-193)
        assert fk == {(name, 4), (name, 5), ("pairhmm_float64_kernel", 2 if rows == 21 else 3)}
        assert {k for g, k in fks if g == rows} == {2, 3, 4, 5}
        # K is the wave's: in the permuted order short reads ride in waves of 3, 4 and 5 rows per lane
        c = pc.permuted(pc.grid_call(rows, 1))
        v = pc.variant(c.n, c.max_read, c.max_hap, rows, False, c.R)
        pw = 64 // rows
        riders = {k for w, k in enumerate(v.float_k) if c.R[w * pw:(w + 1) * pw].min() <= rows}
        assert riders >= {3, 4, 5}
    else:
        assert fk == {("pairhmm_float64_kernel", k) for k in (1, 2, 3, 4)}
        assert dk == {("pairhmm_double64_kernel", k) for k in (1, 2, 3, 4)}
        assert fks == dks == {(64, 1), (64, 2), (64, 3), (64, 4)}
        assert {-(-int(r) // 256) for r in pc.grid(64).R} == {1, 2, 3}  # stripes of 64 lanes x 4 rows


def test_case_sets_reach_every_instantiation():
    fk, dk = set(), set()
    for rows in TABLE:
        fk |= _reach(rows, False)[0]
        dk |= _reach(rows, True)[0]
    assert fk == ALL_FLOAT and dk == ALL_DOUBLE
    assert len(fk) + len(dk) == 14  # every __global__ instantiation of pairhmm_kernels.hip


def _launched(lc):
    """[(kernel, KMAX, LDS bytes)] of one LDS case's call: the float pass and the double pass that follows it."""
    c = lc.case
    v = pc.variant(c.n, c.max_read, c.max_hap, lc.rows, lc.use_double, c.R)
    out = [(v.double_kernel, v.double_kmax, pc.lds_bytes(c.max_hap, v.double_rows, 8))]
    if not lc.use_double:
        out.append((v.float_kernel, v.float_kmax, pc.lds_bytes(c.max_hap, v.float_rows, 4)))
    return out


def test_lds_cases_cross_every_edge():
    cases = {lc.name: lc for lc in pc.lds_cases()}
    plain, above = set(), set()
    for lc in cases.values():
        assert lc.case.max_hap <= pc.max_haplotype_len()
        assert all(int(r) <= 40 for r, h in zip(lc.case.R, lc.case.H) if h == lc.case.max_hap)
        for kernel, kmax, lds in _launched(lc):
            assert lds <= pc.LDS_MAX, lc.name
            (above if lds > pc.LDS_PLAIN else plain).add((kernel, kmax))
    # every instantiation is launched with more than 64 KiB (the function attribute), and at the last plain length
    assert above == ALL_FLOAT | ALL_DOUBLE
    assert plain == ALL_FLOAT | ALL_DOUBLE
    for name, lc in cases.items():
        part = name.split("/")
        if part[1] != "plain":
            continue
        kind, rows = part[2].rstrip("0123456789"), int(part[2].lstrip("floatdube"))
        elem = 4 if kind == "float" else 8
        fit = pc.max_fit(rows, elem, pc.LDS_PLAIN)
        assert pc.lds_bytes(fit, rows, elem) <= pc.LDS_PLAIN < pc.lds_bytes(fit + 1, rows, elem)
        assert lc.case.max_hap in (fit, fit + 1)
        mine = [l for k, m, l in _launched(lc) if k.startswith("pairhmm_%s%s_" % (kind, "" if rows == 16 else rows))]
        assert len(mine) == 1 and (mine[0] > pc.LDS_PLAIN) == (lc.case.max_hap == fit + 1), name
    # four float rings of 16 lanes fill the CU; one base more and the float pass runs on 64 lanes
    fit = pc.max_fit(16, 4, pc.LDS_MAX)
    assert {k for k, m, l in _launched(cases["lds/cu/float16/float/h%d" % fit])} == {"pairhmm_float_kernel", "pairhmm_double64_kernel"}
    assert {k for k, m, l in _launched(cases["lds/cu/float16/float/h%d" % (fit + 1)])} == {"pairhmm_float64_kernel", "pairhmm_double64_kernel"}
    # four double rings: the rescue leaves the 16 lanes, the float pass stays
    fit = pc.max_fit(16, 8, pc.LDS_MAX)
    assert {k for k, m, l in _launched(cases["lds/cu/double16/float/h%d" % fit])} == {"pairhmm_float_kernel", "pairhmm_double_kernel"}
    assert {k for k, m, l in _launched(cases["lds/cu/double16/float/h%d" % (fit + 1)])} == {"pairhmm_float_kernel", "pairhmm_double64_kernel"}
    assert [k for k, m, l in _launched(cases["lds/cu/double16/double/h%d" % fit])] == ["pairhmm_double_kernel"]
    assert [k for k, m, l in _launched(cases["lds/cu/double16/double/h%d" % (fit + 1)])] == ["pairhmm_double64_kernel"]
    for mode in ("float", "double"):
        assert cases["lds/longest/" + mode].case.max_hap == pc.max_haplotype_len()
    assert pc.lds_bytes(pc.max_haplotype_len(), 64, 8) <= pc.LDS_MAX < pc.lds_bytes(pc.max_haplotype_len() + 1, 64, 8)


def _float_sums(case):
    return np.array([case.forward_float(k) for k in range(case.n)])


def test_no_flag_depends_on_rounding():
    """Every pair of every case has its float sum outside [1e-30, 1e-26]; the rescue cases lie on both sides of 1e-28."""
    below = above = 0
    for rows in (16, 21, 32, 64):
        lists = [pc.grid(rows), pc.mixed(rows)] + pc.rescue_cases(rows)
        for c in lists:
            v = _float_sums(c)
            assert not ((v >= pc.BAND[0]) & (v <= pc.BAND[1])).any(), c.name
            if c.name.startswith("rescue"):
                below += int((v < 1e-28).sum())
                above += int((v >= 1e-28).sum())
                want = {"all": c.n, "none": 0}.get(c.name.split("/")[1])
                assert want is None or int((v < 1e-28).sum()) == want
        solo = pc.rescue_cases(rows)[0]
        pw = 64 // rows
        flagged = _float_sums(solo) < 1e-28
        waves = flagged.reshape(-1, pw)
        # wave 2 pos holds one flagged pair at group position pos, wave 2 pos + 1 none
        assert [tuple(np.flatnonzero(w)) for w in waves] == [t for pos in range(pw) for t in ((pos,), ())]
        long_ = pc.rescue_cases(rows)[1]
        assert sorted(long_.R[_float_sums(long_) < 1e-28].tolist()) == [100, 170, 300]
    assert below > 0 and above > 0
    for lc in pc.lds_cases():
        v = _float_sums(lc.case)
        assert not ((v >= pc.BAND[0]) & (v <= pc.BAND[1])).any(), lc.name
        assert (v < 1e-28).sum() == 1  # the read that needs the rescue


def test_sweep_list_turns_the_loop():
    s = pc.sweep()
    turn = pc.SWEEP_GRID * 64
    assert s.n == turn + 64 + 3 and s.max_read <= 12 and s.max_hap <= 12
    assert len(s.read_off) - 1 == 12 and len(s.hap_off) - 1 == 12
    flagged = s.pair_read >= 6   # the pool's flagged reads; sweep() checks each of them against each haplotype
    assert set(np.flatnonzero(flagged).tolist()) == set(s.flagged_at.tolist())
    assert {0, 63, 64, turn - 1, turn, s.n - 1} <= set(s.flagged_at.tolist())
    assert 100 < flagged.sum() < 400
    for rows, kernel in ((64, "pairhmm_double64_kernel"), (16, "pairhmm_double_kernel")):
        v = pc.variant(s.n, s.max_read, s.max_hap, rows, False)
        assert v.double_kernel == kernel
    # the 16-lane rescue skips a wave by ballot: waves with none, one and more flagged pairs all occur
    per_wave = flagged[:s.n - s.n % 4].reshape(-1, 4).sum(axis=1)
    assert {0, 1} <= set(per_wave.tolist())


def test_border_columns_carry_the_sum():
    """16-lane grid: without the haplotype's last base (suffix reads) or first base (prefix reads) log10 moves by more
    than 1e-3, a hundred times the tolerance of the GPU test: no kernel that drops a border column can pass it."""
    g = pc.grid(16)
    n = only_n = 0
    for k in range(g.n):
        hap = g.hap(int(g.pair_hap[k]))
        if len(hap) < 2:
            continue
        rd = g.read(int(g.pair_read[k]))
        if len(rd[0]) == 1 and rd[0] not in (b"A", b"C", b"G", b"T"):
            # a one-row read of N matches every column, one of another odd byte none: H equal terms of INITIAL / H, whatever H
            only_n += 1
            continue
        full, _ = pol.log10_likelihood(hap, *rd, use_double=True)
        cut, _ = pol.log10_likelihood(hap[:-1] if g.kind[k] == "suffix" else hap[1:], *rd, use_double=True)
        assert abs(full - cut) > 1e-3, (k, g.kind[k], full, cut)
        n += 1
    assert n + only_n == g.n - 2 * len(pc.GRID_R[16]) and only_n <= 20


def test_tracks_differ_on_every_row_and_odd_bytes_occur():
    for rows in (16, 21, 32, 64):
        g = pc.grid(rows)
        zeros = tops = 0
        first_last = set()
        for r in range(len(g.read_off) - 1):
            bases, *tracks = (np.frombuffer(t, np.uint8) for t in g.read(r))
            R = len(bases)
            for n, t in enumerate(tracks):
                # (the GCP of rows that can only be inserted is 0 or 1 with either top bit)
                assert R < 16 or len(set(t.tolist())) > (min(R, 64) // 4 if n < 3 else 2)
                tops += int((t > 127).sum())
                zeros += int((t & 127 == 0).sum())
            if R >= 16:
                assert len({tuple(tr[i] for tr in tracks) for i in range(R)}) > 0.9 * R
            first_last |= {("row1", int(tracks[0][0]) & 127), ("rowR", int(tracks[(len(pc.special_rows(R, rows)) - 1) // 2 % 4][R - 1]) & 127)}
            for where, b in (("read1", bases[0]), ("readR", bases[-1])):
                first_last.add((where, int(b)))
        assert zeros > 100 and tops > 1000
        assert ("row1", 127) in first_last and {("rowR", 0), ("rowR", 127)} & first_last
        for where in ("read1", "readR"):
            assert {(where, ord("N")), (where, 0), (where, 255)} <= first_last
        hap_ends = {(int(g.haps[g.hap_off[h]]), int(g.haps[g.hap_off[h + 1] - 1])) for h in range(len(g.hap_off) - 1)}
        assert any(a == ord("N") for a, b in hap_ends) and any(b == ord("N") for a, b in hap_ends)
        assert ((g.haps >= ord("a")) & (g.haps <= ord("t"))).any()


def test_mixed_waves_are_mixed():
    for rows in (16, 21, 32):
        m = pc.mixed(rows)
        pw = 64 // rows
        big = 48 if rows == 16 else rows * 5
        waves = [(m.R[w:w + pw].tolist(), m.H[w:w + pw].tolist()) for w in range(0, m.n, pw)]
        for pos in range(pw):
            r, h = waves[pos]
            assert r[pos] == big and h[pos] == 330 and all(x == 1 for i, x in enumerate(r) if i != pos)
            r, h = waves[pw + pos]
            assert r[pos] == 1 and h[pos] == 1 and all(x == big for i, x in enumerate(r) if i != pos)
            ns = [int(ord("N") in m.hap(int(x))) for x in m.pair_hap[(2 * pw + pos) * pw:(2 * pw + pos + 1) * pw]]
            assert ns == [int(i == pos) for i in range(pw)]
            r, h = waves[3 * pw + pos]
            assert r[pos] == 48 and all(x == 5 for i, x in enumerate(r) if i != pos)
        if rows != 16:
            v = pc.variant(m.n, m.max_read, m.max_hap, rows, False, m.R)
            assert v.float_kmax == 5 and set(v.float_k[:2 * pw]) == {5}  # the lone (1, 1) pair takes K = 5: four virtual rows


def test_sizes():
    limit = pc.max_haplotype_len()
    lists = [pc.sweep()] + [lc.case for lc in pc.lds_cases()]
    for rows in (16, 21, 32, 64):
        lists += [pc.grid(rows), pc.mixed(rows)] + pc.rescue_cases(rows)
    for c in lists:
        assert c.n <= pc.MAX_PAIRS, c.name
        assert c.max_read <= 520 and c.max_hap <= limit, c.name
    for rows in (16, 21, 32, 64):
        g = pc.grid(rows)
        assert g.max_read <= 513 and g.max_hap <= 140 and g.n <= 520


def test_variant_follows_the_per_batch_choice():
    """rows = 0, the cases the comment in run_device names (pairhmm_capi.cpp:168-190)."""
    v = pc.variant(1_600_000, 150, 300, 0, False)
    assert (v.float_kernel, v.float_kmax, v.double_kernel, v.double_kmax) == ("pairhmm_float32_kernel", 5, "pairhmm_double64_kernel", 3)
    v = pc.variant(1_600_000, 100, 250, 0, False)
    assert (v.float_kernel, v.float_kmax) == ("pairhmm_float21_kernel", 5)
    v = pc.variant(800, 150, 300, 0, False)
    assert (v.float_kernel, v.float_kmax) == ("pairhmm_float64_kernel", 3)
    v = pc.variant(40, 40, 90, 0, False)
    assert (v.float_kernel, v.double_kernel) == ("pairhmm_float_kernel", "pairhmm_double_kernel")
    v = pc.variant(40, 40, 90, 0, True)
    assert v.float_kernel is None and v.double_kernel == "pairhmm_double_kernel"
