"""mgl_sw_extend_seed_batch_device on the GPU, bit-exact against the textbook (tests/seed_extend_textbook.py) on every output -- the eight
fields of the record, both side records, CIGAR bytes, length, status -- with the flank lengths on the strip seams of the kernels
underneath, every empty flank, every status, a chunked batch and the long suite's 10 kb pair."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import extend_adaptive_cases as cases  # noqa: E402
import extend_textbook as et  # noqa: E402
import golden_io  # noqa: E402
import seed_extend_textbook as stb  # noqa: E402

pytestmark = pytest.mark.gpu

GATK = (200, -150, 260, 11)
PARAM_SETS = [GATK, (3, -1, 4, 3), (1, -4, 6, 1)]  # GATK's and two of tests/test_gpu_banded.py's: gext near gopen, a dear mismatch
FLANKS = (0, 1, 63, 64, 65, 128, 129)             # the strip seams of the extension kernels
BANDS = (0, 1, 31, 64, 200)


@pytest.fixture(scope="module")
def aligner():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mgl_amd import smithwaterman as sw

    a = sw.MicrosoftSmithWaterman(0)
    assert a.load()
    yield a
    a.close()


@functools.lru_cache(maxsize=None)
def _want(T, Q, seed, params, band, zdrop, to_qend, adaptive):
    """the textbook's (SeedAln, cigar, left Ext, right Ext), computed once per case"""
    return stb.seed_extend(T, Q, seed, *params, band, zdrop, to_qend, adaptive)


def _check(aligner, Ts, Qs, seeds, band, zdrop, params=GATK, to_qend=False, adaptive=False):
    """every output of a batch against the textbook; -> the textbook's results"""
    from mgl_amd import _lib

    res, left, right, st = aligner.extend_seed(Ts, Qs, seeds, band, zdrop, params, to_qend, adaptive_band=adaptive, return_sides=True, return_status=True)
    assert aligner.timing().fill_kernel == (14 if adaptive else 13) == (_lib.KERNEL_EXTEND_ADAPTIVE if adaptive else _lib.KERNEL_EXTEND)
    want = [_want(T, Q, tuple(s), params, band, zdrop, to_qend, adaptive) for T, Q, s in zip(Ts, Qs, seeds)]
    for k, (aln, cigar, l, r) in enumerate(want):
        got = (int(st[k]), stb.SeedAln(*(int(res[c][k]) for c in range(8))), res.cigars[k], int(res.cigar_len[k]), et.Ext(*map(int, left[k])), et.Ext(*map(int, right[k])))
        assert got == (0, aln, cigar, len(cigar), l, r), (k, Ts[k], Qs[k], seeds[k], params, band, zdrop, to_qend, adaptive)
    return want


def _seeded_pair(rng, lt, lq, sl, rt, rq, alphabet=b"ACGT", exact=True):
    """a window and a query around a seed of sl bases: flanks of (lt, lq) bases in front of it and (rt, rq) behind, each query flank a
    noisy copy of its target flank that starts (left: ends) at the seed"""
    tl_, ql_ = cases.noisy_pair(rng, lt, lq, alphabet) if lt and lq else (cases.seq(rng, lt), cases.seq(rng, lq))
    tr_, qr_ = cases.noisy_pair(rng, rt, rq, alphabet) if rt and rq else (cases.seq(rng, rt), cases.seq(rng, rq))
    seed_t = cases.seq(rng, sl)
    seed_q = bytearray(seed_t)
    if not exact and sl > 2:
        seed_q[sl // 2] = ord("N")
    return tl_[::-1] + seed_t + tr_, ql_[::-1] + bytes(seed_q) + qr_, (lt, lq, sl)


@functools.lru_cache(maxsize=None)
def _geometry_batch():
    """flank lengths on, one short of and one past the strip seams, every one of them on either side and next to three others; the
    query's flank a base shorter, as long or a base longer, or empty next to a target flank that is not (and the reverse); seeds of 1
    and 50 bases; the windows of 1 to 4 bases"""
    rng = np.random.default_rng(31)
    Ts, Qs, seeds = [], [], []
    n = 0
    for a, lt in enumerate(FLANKS):
        for step in (0, 2, 5):
            rt = FLANKS[(a + step) % len(FLANKS)]
            lq = max(0, lt + (n % 3) - 1) if n % 5 else (0 if lt else 3)
            rq = max(0, rt + ((n // 3) % 3) - 1) if n % 7 else (0 if rt else 2)
            T, Q, s = _seeded_pair(rng, lt, lq, (1, 50)[n & 1], rt, rq, b"AC" if n % 4 == 3 else b"ACGT", exact=n % 6 != 0)
            Ts.append(T)
            Qs.append(Q)
            seeds.append(s)
            n += 1
    for T, Q, s in ((b"A", b"A", (0, 0, 1)), (b"A", b"C", (0, 0, 1)), (b"AC", b"GAC", (0, 1, 2)), (b"ACG", b"C", (1, 0, 1)), (b"ACGT", b"ACGT", (1, 1, 2)),
                    (b"ACGT", b"AGGT", (3, 3, 1)), (b"ACGT", b"TACGTA", (0, 1, 4))):
        Ts.append(T)
        Qs.append(Q)
        seeds.append(s)
    assert len(Ts) == 28 and max(len(T) for T in Ts) >= 129 + 1 + 129 and min(len(T) for T in Ts) == 1
    return Ts, Qs, seeds


@pytest.mark.parametrize("to_qend", (False, True))
@pytest.mark.parametrize("adaptive", (False, True))
@pytest.mark.parametrize("pk", range(len(PARAM_SETS)))
def test_flank_lengths_seeds_bands_and_flags(aligner, pk, adaptive, to_qend):
    """the full product: every geometry at every band with every Z-drop mode, under each parameter set and both flags"""
    Ts, Qs, seeds = _geometry_batch()
    params = PARAM_SETS[pk]
    o = params[2]
    dropped = [0, 0, 0, 0]
    qend = 0
    for band in BANDS:
        for zdrop in (-1, 2 * o, 40 * o):  # off, tight, loose
            want = _check(aligner, Ts, Qs, seeds, band, zdrop, params, to_qend=to_qend, adaptive=adaptive)
            for w in want:
                dropped[w[0].dropped] += 1
                qend += w[0].cigar_from != 0
    assert dropped[0] > 20 and dropped[1] + dropped[2] + dropped[3] > 10 and (qend > 10 if to_qend else qend == 0), (dropped, qend)


def _status_batch():
    """about 90 pairs of up to 300 bases with random seeds, and among them every way to be refused"""
    rng = np.random.default_rng(17)
    Ts, Qs, seeds = [], [], []
    for k in range(90):
        lt, rt = int(rng.integers(0, 140)), int(rng.integers(0, 140))
        lq, rq = max(0, lt + int(rng.integers(-3, 4))), max(0, rt + int(rng.integers(-3, 4)))
        if k in (30, 31):  # a seed with nothing to extend: the whole of both sequences, and an empty flank of either kind on each side
            lt, lq, rt, rq = ((0, 0, 0, 0), (5, 0, 0, 4))[k - 30]
        T, Q, s = _seeded_pair(rng, lt, lq, int(rng.integers(1, 20)), rt, rq, exact=bool(k % 4))
        Ts.append(T)
        Qs.append(Q)
        seeds.append(s)
    Ts[5], Qs[5] = cases.noisy_pair(rng, 14000, 6000)
    seeds[5] = (100, 50, 30)  # its right side fits no slot of the 1 MiB workspace
    return Ts, Qs, seeds


WIDE_11 = 301  # pair 11's length as the call states it: above a max_tl of 300, and under a larger bound a window that runs into pair 12
BAD = {7: "target length 0", 9: "query length 0", 11: "target above max_tl", 13: "sl = 0", 15: "seed past the window's end", 17: "seed past the query's end",
       19: "st < 0", 21: "sq < 0", 23: "sl < 0"}


def _device_call(al, Ts, Qs, seeds, band, zdrop, stride, max_tl, max_ql, params=GATK, to_qend=True, adaptive=False, binary=False, score_only=False,
                 sides=True):
    """the tensor form on inputs broken as BAD says, canaries behind every output; -> numpy arrays (aln, left, right, cigar rows, lengths, status)"""
    dev = torch.device("cuda", 0)
    n = len(Ts)
    g = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    tl, ql = np.array([len(t) for t in Ts], np.int32), np.array([len(q) for q in Qs], np.int32)
    toff, qoff = np.concatenate([[0], np.cumsum(tl)[:-1]]).astype(np.int64), np.concatenate([[0], np.cumsum(ql)[:-1]]).astype(np.int64)
    sd = np.array(seeds, np.int32)
    tl[7], ql[9], tl[11] = 0, 0, WIDE_11
    sd[13, 2] = 0
    sd[15, 0] = tl[15] - sd[15, 2] + 1
    sd[17, 1] = ql[17] - sd[17, 2] + 1
    sd[19, 0], sd[21, 1], sd[23, 2] = -1, -1, -5
    td, qd = g(np.frombuffer(b"".join(Ts) + b"\0" * 400, np.uint8).copy()), g(np.frombuffer(b"".join(Qs) + b"\0" * 8, np.uint8).copy())
    rec = lambda: torch.full((n + 1, 8), -77, dtype=torch.int32, device=dev)  # noqa: E731
    out = (rec(), rec() if sides else None, rec() if sides else None, torch.full(((n + 1) * stride,), 0xEE, dtype=torch.uint8, device=dev),
           torch.full((n + 1,), -77, dtype=torch.int32, device=dev), torch.full((n + 1,), -77, dtype=torch.int32, device=dev))
    al.extend_seed_device(td, g(toff), g(tl), qd, g(qoff), g(ql), g(sd[:, 0].copy()), g(sd[:, 1].copy()), g(sd[:, 2].copy()), max_tl, max_ql, band, zdrop,
                          params, to_qend, stride, binary, score_only, out=(out[0][:n], out[1], out[2], out[3], out[4], out[5]), adaptive_band=adaptive,
                          sides=sides)
    torch.cuda.synchronize()
    assert al.timing().fill_kernel == (14 if adaptive else 13)
    return [None if x is None else x.cpu().numpy() for x in out]


def _check_outputs(outs, want, n, stride, statuses, binary=False):
    """outs against the textbook's results where `statuses[k]` is 0 or overflow, all-zero otherwise; canaries behind every row and array"""
    from mgl_amd import _lib

    aln, left, right, cg, ln, st = outs
    cg = cg.reshape(n + 1, stride)
    assert ln[n] == -77 and st[n] == -77 and (aln[n] == -77).all() and (cg[n] == 0xEE).all()
    assert left is None or ((left[n] == -77).all() and (right[n] == -77).all())
    seen = set()
    for k in range(n):
        w_aln, w_cigar, w_l, w_r = want[k] if want[k] else (None, "", None, None)
        size = 4 * len(stb.elements(w_cigar)) if binary else len(w_cigar)
        status = statuses[k] if statuses[k] else (_lib.ERR_CIGAR_OVERFLOW if size > (stride & ~3 if binary else stride) else 0)
        seen.add(status)
        assert st[k] == status, (k, st[k], status)
        if status:
            assert ln[k] == 0 and (aln[k] == 0).all() and (cg[k] == 0xEE).all(), k
            assert left is None or ((left[k] == 0).all() and (right[k] == 0).all()), k
        else:
            assert ln[k] == size and tuple(aln[k]) == tuple(w_aln), (k, aln[k], w_aln)
            assert left is None or (tuple(left[k]) == tuple(w_l) and tuple(right[k]) == tuple(w_r)), k
            text = et.cigar_binary_to_text(cg[k, :ln[k]].view("<u4")) if binary else cg[k, :ln[k]].tobytes().decode()
            assert text == w_cigar and (cg[k, ln[k]:] == 0xEE).all(), k  # nothing at or beyond cigar_len
    return seen


def test_statuses_canaries_chunks_score_only_binary_and_optional_outputs(aligner):
    from mgl_amd import _lib
    from mgl_amd import smithwaterman as sw

    Ts, Qs, seeds = _status_batch()
    n, band, zdrop = len(Ts), 20, 2000
    bad, unsup = _lib.ERR_BAD_ARG, _lib.ERR_UNSUPPORTED
    want = [None if (k in BAD or k == 5) else _want(Ts[k], Qs[k], seeds[k], GATK, band, zdrop, True, False) for k in range(n)]
    lens = sorted(len(w[1]) for w in want if w)
    stride = lens[len(lens) // 2]  # the median CIGAR fits its row exactly; a stride one below, and it is one byte too long
    exact = [k for k in range(n) if want[k] and len(want[k][1]) == stride]
    assert exact and stride >= 8 and lens[0] < stride - 1 and lens[-1] > stride

    # ---- a context of its own with the smallest workspace there is, 1 MiB, and bounds that make a pair's staging 20 kB: the batch
    # goes in chunks, and pair 5 (14 000 x 6 000, the seed near its start) has a right side that fits no slot
    small_ws = sw.MicrosoftSmithWaterman(0)
    try:
        small_ws.set_workspace(1 << 20)
        outs_small = _device_call(small_ws, Ts, Qs, seeds, band, zdrop, stride, 14000, 6000)
        assert small_ws.timing().dp_launches >= 4  # two per chunk
    finally:
        small_ws.close()
    statuses = [bad if k in BAD else 0 for k in range(n)]
    small_statuses = list(statuses)
    small_statuses[5], small_statuses[11] = unsup, 0  # (max_tl = 14 000 admits pair 11's 301 bases)
    want_small = list(want)
    at11 = sum(len(t) for t in Ts[:11])
    T11 = b"".join(Ts)[at11:at11 + WIDE_11]
    want_small[11] = _want(T11, Qs[11], seeds[11], GATK, band, zdrop, True, False)
    seen = _check_outputs(outs_small, want_small, n, stride, small_statuses)
    assert seen == {0, bad, _lib.ERR_CIGAR_OVERFLOW, unsup}

    # ---- the default workspace, one chunk, max_tl = 300 (pairs 5 and 11 are above it): the same results
    statuses[5] = bad
    outs = _device_call(aligner, Ts, Qs, seeds, band, zdrop, stride, 300, 6000)
    assert aligner.timing().dp_launches == 2
    _check_outputs(outs, want, n, stride, statuses)
    for a, b in zip(outs, outs_small):
        same = [k for k in range(n) if k not in (5, 11)]
        assert (a.reshape(n + 1, -1)[same] == b.reshape(n + 1, -1)[same]).all()
    # one byte less: the pairs that fitted exactly overflow, and nothing else changes
    outs1 = _device_call(aligner, Ts, Qs, seeds, band, zdrop, stride - 1, 300, 6000)
    _check_outputs(outs1, want, n, stride - 1, statuses)
    assert all(outs[5][k] == 0 and outs1[5][k] == _lib.ERR_CIGAR_OVERFLOW for k in exact)

    # ---- without the side records, and score-only with no CIGAR arrays written
    outs2 = _device_call(aligner, Ts, Qs, seeds, band, zdrop, stride, 300, 6000, sides=False)
    _check_outputs(outs2, want, n, stride, statuses)
    aln3, left3, right3, cg3, ln3, st3 = _device_call(aligner, Ts, Qs, seeds, band, zdrop, stride, 300, 6000, score_only=True)
    for k in range(n):
        if statuses[k]:
            assert st3[k] == statuses[k] and (aln3[k] == 0).all() and (left3[k] == 0).all() and (right3[k] == 0).all()
        else:  # (an overflow cannot happen)
            assert st3[k] == 0 and (tuple(aln3[k]), tuple(left3[k]), tuple(right3[k])) == (tuple(want[k][0]), tuple(want[k][2]), tuple(want[k][3])), k
    assert (cg3 == 0xEE).all() and (ln3[:n] == 0).all() and ln3[n] == -77

    # ---- binary CIGAR: the text's elements
    outs4 = _device_call(aligner, Ts, Qs, seeds, band, zdrop, 4 * 20 + 3, 300, 6000, binary=True)
    seen = _check_outputs(outs4, want, n, 4 * 20 + 3, statuses, binary=True)
    assert seen == {0, bad, _lib.ERR_CIGAR_OVERFLOW} and (outs4[5][:n] == 0).sum() > 20

    # ---- outside the range guard (gopen above 2^24): a pair with a side to extend is unsupported, a seed alone is not
    huge = (200, -150, (1 << 24) + 1, 11)
    outs5 = _device_call(aligner, Ts, Qs, seeds, band, zdrop, stride, 300, 6000, params=huge)
    alone = lambda s, T, Q: (s[0] == 0 or s[1] == 0) and (s[0] + s[2] == len(T) or s[1] + s[2] == len(Q))  # noqa: E731
    want5 = [w and (_want(Ts[k], Qs[k], seeds[k], huge, band, zdrop, True, False) if alone(seeds[k], Ts[k], Qs[k]) else None) for k, w in enumerate(want)]
    assert sum(1 for w in want5 if w) == 2
    _check_outputs(outs5, want5, n, stride, [statuses[k] or (0 if want5[k] else unsup) for k in range(n)])


def test_both_flags_on_the_status_batch_through_the_list_form(aligner):
    """the list form raises on a pair's status unless it is asked for; with both flags on, the well-formed pairs of the batch"""
    from mgl_amd import _lib

    Ts, Qs, seeds = _status_batch()
    keep = [k for k in range(len(Ts)) if k != 5][:40]
    Ts, Qs, seeds = [Ts[k] for k in keep], [Qs[k] for k in keep], [seeds[k] for k in keep]
    _check(aligner, Ts, Qs, seeds, 20, 2000, GATK, True, True)
    with pytest.raises(_lib.MglSwError):
        aligner.extend_seed(Ts, Qs, [(0, 0, 0)] + seeds[1:], 20, 2000)
    res = aligner.extend_seed(Ts, Qs, seeds, 20, 2000, score_only=True)
    assert res.cigars is None and [int(x) for x in res.score] == [_want(T, Q, s, GATK, 20, 2000, False, False)[0].score for T, Q, s in zip(Ts, Qs, seeds)]


def _middle_seed(t, q, sl=50, anchor=16):
    """a seed of sl bases near the middle of q: it starts where a 16-mer of q has its one exact copy in t and has at most five mismatches"""
    mid = len(q) // 2
    for d in range(0, 2000):
        for p in (mid - d, mid + d):
            u = t.find(q[p:p + anchor])
            if u >= 0 and t.find(q[p:p + anchor], u + 1) < 0 and abs(u - p) < 1500 and sum(t[u + k] == q[p + k] for k in range(sl)) >= sl - 5:
                return u, p, sl
    raise AssertionError("no anchor")


def test_a_10_kb_pair_at_band_512_from_a_seed_in_its_middle_with_and_without_junk_ends(aligner):
    recs = [g for g in golden_io.load("long") if len(g.t) >= 9000 and len(g.q) >= 9000]
    assert recs
    g = recs[0]
    seed = _middle_seed(g.t, g.q)
    for adaptive in (False, True):
        (aln, cigar, l, r), = _check(aligner, [g.t], [g.q], [seed], 512, 400 * 11, g.params, True, adaptive)
        assert aln.dropped == 0 and aln.t_beg < 500 and aln.t_end > 9000 and et.cigar_score(cigar, g.t[aln.t_beg:aln.t_end], g.q[aln.q_beg:aln.q_end], *g.params) == aln.score
    rng = np.random.default_rng(12)
    junk = lambda ab: np.frombuffer(ab, np.uint8)[rng.integers(2, size=3000)].tobytes()  # noqa: E731
    t, q = junk(b"AC") + g.t + junk(b"AC"), junk(b"GT") + g.q + junk(b"GT")
    (aln, cigar, l, r), = _check(aligner, [t], [q], [(seed[0] + 3000, seed[1] + 3000, 50)], 512, 400 * 11, g.params)
    assert aln.dropped == 3 and aln.t_beg >= 3000 and aln.t_end <= 3000 + len(g.t) and aln.t_end - aln.t_beg > 8500
