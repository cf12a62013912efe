"""mgl_sw_align_chain_batch_device on the GPU, bit-exact against the textbook (tests/chain_textbook.py) on every output -- the eight fields
of the record, both side records, the gap scores, CIGAR bytes, length, status -- with the gap and flank lengths on the strip seams of
the kernels underneath, chains beyond one and two waves' worth of anchors, every way to be refused, overflow at the byte, slot reuse,
and the tie to the seed entry and to the long suite's 10 kb pair."""
import functools
import hashlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import banded_textbook as bt  # noqa: E402
import chain_textbook as ct  # noqa: E402
import extend_adaptive_cases as cases  # noqa: E402
import extend_textbook as et  # noqa: E402
import golden_io  # noqa: E402
import seed_extend_textbook as stb  # noqa: E402
from chain_cases import chain_pair  # noqa: E402

pytestmark = pytest.mark.gpu

GATK = (200, -150, 260, 11)
PARAM_SETS = [GATK, (3, -1, 4, 3), (1, -4, 6, 1)]  # GATK's and two of tests/test_gpu_banded.py's: gext near gopen, a dear mismatch
SIZES = (0, 1, 63, 64, 65, 129)                    # gap lengths: the strip seams of the fill, a last strip of one row
FLANKS = (0, 1, 64, 65)
BANDS = (0, 1, 31, 200)


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
def _want(T, Q, anchors, params, band, zdrop, to_qend, adaptive):
    """the textbook's (ChainAln, cigar, left Ext, right Ext, gap scores), computed once per case"""
    return ct.chain_align(T, Q, anchors, *params, band, zdrop, to_qend, adaptive)


def _tuples(chain):
    return tuple(tuple(int(x) for x in a) for a in chain)


def _check(aligner, Ts, Qs, chains, band, zdrop, params=GATK, to_qend=False, adaptive=False):
    """every output of a batch against the textbook, every status 0; -> the textbook's results"""
    from mgl_amd import _lib

    res, left, right, gs, st = aligner.align_chain(Ts, Qs, chains, band, zdrop, params, to_qend, adaptive_band=adaptive, return_sides=True, return_gap_scores=True,
                                                   return_status=True)
    t = aligner.timing()
    assert t.fill_kernel == (14 if adaptive else 13) == (_lib.KERNEL_EXTEND_ADAPTIVE if adaptive else _lib.KERNEL_EXTEND) and t.dp_launches == 3
    assert not st.any(), st  # by construction: no refusal can hide a mismatch
    want = [_want(T, Q, _tuples(c), params, band, zdrop, to_qend, adaptive) for T, Q, c in zip(Ts, Qs, chains)]
    at = 0
    for k, (aln, cigar, l, r, gaps) in enumerate(want):
        got = (ct.ChainAln(*(int(res[c][k]) for c in range(8))), res.cigars[k], int(res.cigar_len[k]), et.Ext(*map(int, left[k])), et.Ext(*map(int, right[k])),
               [int(x) for x in gs[at:at + len(gaps)]])
        assert got == (aln, cigar, len(cigar), l, r, gaps), (k, Ts[k], Qs[k], chains[k], params, band, zdrop, to_qend, adaptive)
        at += len(gaps)
    assert at == len(gs)
    return want


@functools.lru_cache(maxsize=None)
def _geometry_batch():
    """every pair (gt, gq) of SIZES as a gap -- (1, 65) and (129, 63) among them --, two to a chain of three anchors of 1 and 20 bases
    with flanks of 0, 1, 64, 65 around it; chains of 1, 2, 65 and 130 anchors (beyond one and two waves' worth), the long ones over small
    gaps of every kind in windows of a few thousand bases; windows of one to four bases"""
    rng = np.random.default_rng(41)
    Ts, Qs, chains = [], [], []
    combos = [(a, b) for a in SIZES for b in SIZES]
    assert (1, 65) in combos and (129, 63) in combos and len(combos) == 36
    for n in range(18):
        gaps = [combos[n], combos[35 - n]]
        fl = [FLANKS[(n + x) % 4] for x in range(4)]
        lq, rq = (max(0, fl[0] + (n % 3) - 1) if n % 5 else (0 if fl[0] else 3)), (max(0, fl[2] + ((n // 3) % 3) - 1) if n % 7 else (0 if fl[2] else 2))
        T, Q, c = chain_pair(rng, (fl[0], lq, fl[2], rq), gaps, [(1, 20)[(n + x) & 1] for x in range(3)], b"AC" if n % 4 == 3 else b"ACGT", exact=n % 6 != 0)
        Ts.append(T), Qs.append(Q), chains.append(c)
    small = [(0, 0), (1, 1), (0, 2), (3, 0), (2, 3), (5, 4), (1, 0), (7, 7)]
    for K, fl in ((1, (64, 65, 65, 64)), (2, (0, 0, 1, 1)), (65, (1, 0, 0, 1)), (130, (65, 64, 64, 66)), (130, (0, 0, 0, 0))):
        T, Q, c = chain_pair(rng, fl, [small[(x + K) % len(small)] for x in range(K - 1)], [(1, 20)[(x // 3) & 1] for x in range(K)], exact=K != 65)
        Ts.append(T), Qs.append(Q), chains.append(c)
    for T, Q, c in ((b"A", b"A", [(0, 0, 1)]), (b"AC", b"GC", [(0, 0, 1), (1, 1, 1)]), (b"ACGT", b"AT", [(0, 0, 1), (3, 1, 1)]), (b"ACG", b"TACGTA", [(0, 1, 1), (2, 3, 1)])):
        Ts.append(T), Qs.append(Q), chains.append(c)
    assert sorted({len(c) for c in chains}) == [1, 2, 3, 65, 130] and 1500 < max(len(T) for T in Ts) < 5000
    return Ts, Qs, chains


@pytest.mark.parametrize("to_qend", (False, True))
@pytest.mark.parametrize("adaptive", (False, True))
@pytest.mark.parametrize("pk", range(len(PARAM_SETS)))
def test_gap_sizes_chain_lengths_flanks_bands_and_flags(aligner, pk, adaptive, to_qend):
    """the full product: every geometry at every band with the Z-drop off and tight, under each parameter set and both flags"""
    Ts, Qs, chains = _geometry_batch()
    params = PARAM_SETS[pk]
    dropped, qend = [0, 0, 0, 0], 0
    for band in BANDS:
        for zdrop in (-1, 2 * params[2]):
            for w in _check(aligner, Ts, Qs, chains, band, zdrop, params, to_qend=to_qend, adaptive=adaptive):
                dropped[w[0].dropped] += 1
                qend += w[0].cigar_from != 0
    assert dropped[0] > 20 and dropped[1] + dropped[2] + dropped[3] > 5 and (qend > 10 if to_qend else qend == 0), (dropped, qend)


def _status_batch():
    """48 chains of 1 to 6 anchors over gaps of up to 65 bases, one of 40 anchors (what the sum guard refuses at a gopen of 2^24), and
    among them every way to be refused"""
    rng = np.random.default_rng(19)
    Ts, Qs, chains = [], [], []
    for k in range(48):
        K = 40 if k == 27 else 1 + k % 6
        gaps = [(int(rng.integers(0, 66)), int(rng.integers(0, 66))) if K < 40 else (int(rng.integers(0, 4)), int(rng.integers(0, 4))) for _ in range(K - 1)]
        lt, rt = int(rng.integers(0, 70)), int(rng.integers(0, 70))
        fl = (lt, max(0, lt + int(rng.integers(-2, 3))), rt, max(0, rt + int(rng.integers(-2, 3))))
        if k == 30:
            fl = (5, 0, 0, 4)
        if k == UNSUP_GAP:
            gaps[1] = (129, 5)  # above the max_gap_tl of 66 that the calls state
        T, Q, c = chain_pair(rng, fl, gaps, [int(rng.integers(1, 21)) for _ in range(K)], exact=bool(k % 4))
        Ts.append(T), Qs.append(Q), chains.append(c)
    return Ts, Qs, chains


BAD = {7: "target length 0", 9: "query length 0", 11: "overlapping anchors", 14: "crossing anchors", 15: "anchor past the window's end", 17: "anchor past the query's end",
       19: "K = 0", 21: "the CSR descends", 22: "a range that shares an anchor with pair 20's", 23: "sl = 0", 29: "st < 0", 33: "target above max_tl"}
UNSUP_GAP, UNSUP_SUM = 26, 27
MAX_GAP = (66, 66)


def _device_call(al, Ts, Qs, chains, band, zdrop, stride, max_tl, max_ql, params=GATK, to_qend=True, adaptive=False, binary=False, score_only=False, sides=True,
                 max_gap=MAX_GAP, broken=True):
    """the tensor form on inputs broken as BAD says, canaries behind every output; -> numpy arrays (aln, left, right, gap scores, cigar
    rows, lengths, status) and the anchor range of every pair as the call saw it"""
    dev = torch.device("cuda", 0)
    n = len(Ts)
    g = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    tl, ql = np.array([len(t) for t in Ts], np.int32), np.array([len(q) for q in Qs], np.int32)
    toff, qoff = np.concatenate([[0], np.cumsum(tl)[:-1]]).astype(np.int64), np.concatenate([[0], np.cumsum(ql)[:-1]]).astype(np.int64)
    chains = [[list(a) for a in c] for c in chains]
    if broken:
        assert all(len(chains[k]) >= 3 for k in (11, 14)) and len(chains[20]) >= 1
        chains[19] = []                                                                 # K = 0
        tl[7], ql[9], tl[33] = 0, 0, max_tl + 1
        chains[11][1][0] = chains[11][0][0] + chains[11][0][2] - 1                     # anchor 1 starts inside anchor 0 on the target
        chains[14][1][1], chains[14][2][1] = chains[14][2][1], chains[14][1][1]         # anchors 1 and 2 cross on the query
        chains[15][-1][0] = int(tl[15]) - chains[15][-1][2] + 1
        chains[17][-1][1] = int(ql[17]) - chains[17][-1][2] + 1
        chains[23][0][2] = 0
        chains[29][0][0] = -1
    start = np.zeros(n + 1, np.int64)
    np.cumsum([len(c) for c in chains], out=start[1:])
    flat = np.array([a for c in chains for a in c], np.int32)
    total = len(flat)
    if broken:
        # start[22] steps back below start[21] by one: pair 21's range descends, and pair 22's begins on pair 20's last anchor
        start[22] = start[21] - 1
    td, qd = g(np.frombuffer(b"".join(Ts) + b"\0" * 400, np.uint8).copy()), g(np.frombuffer(b"".join(Qs) + b"\0" * 8, np.uint8).copy())
    rec = lambda: torch.full((n + 1, 8), -77, dtype=torch.int32, device=dev)  # noqa: E731
    out = (rec(), rec() if sides else None, rec() if sides else None, torch.full((total + 1,), -77, dtype=torch.int32, device=dev),
           torch.full(((n + 1) * stride,), 0xEE, dtype=torch.uint8, device=dev), torch.full((n + 1,), -77, dtype=torch.int32, device=dev),
           torch.full((n + 1,), -77, dtype=torch.int32, device=dev))
    al.align_chain_device(td, g(toff), g(tl), qd, g(qoff), g(ql), g(start), g(flat[:, 0].copy()), g(flat[:, 1].copy()), g(flat[:, 2].copy()), max_tl, max_ql,
                          max_gap[0], max_gap[1], band, zdrop, params, to_qend, stride, binary, score_only,
                          out=(out[0][:n], out[1], out[2], out[3][:total], out[4], out[5], out[6]), adaptive_band=adaptive, sides=sides, gap_scores=True)
    torch.cuda.synchronize()
    assert al.timing().fill_kernel == (14 if adaptive else 13)
    return [None if x is None else x.cpu().numpy() for x in out], start


def _check_outputs(outs, start, want, n, stride, statuses, binary=False, score_only=False):
    """outs against the textbook's results where `statuses[k]` is 0 or overflow, all-zero otherwise; canaries behind every row and array"""
    from mgl_amd import _lib

    aln, left, right, gs, cg, ln, st = outs
    cg = cg.reshape(n + 1, stride)
    assert ln[n] == -77 and st[n] == -77 and (aln[n] == -77).all() and (cg[n] == 0xEE).all() and gs[-1] == -77
    assert left is None or ((left[n] == -77).all() and (right[n] == -77).all())
    seen = set()
    gap_want = np.zeros(len(gs) - 1, np.int64)
    for k in range(n):
        w_aln, w_cigar, w_l, w_r, w_gaps = want[k] if want[k] else (None, "", None, None, None)
        size = 0 if score_only else 4 * len(stb.elements(w_cigar)) if binary else len(w_cigar)
        status = statuses[k] if statuses[k] else (_lib.ERR_CIGAR_OVERFLOW if size > (stride & ~3 if binary else stride) else 0)
        seen.add(status)
        assert st[k] == status, (k, st[k], status)
        if status:
            assert ln[k] == 0 and (aln[k] == 0).all() and (cg[k] == 0xEE).all(), k
            assert left is None or ((left[k] == 0).all() and (right[k] == 0).all()), k
        else:
            assert ln[k] == size and tuple(aln[k]) == tuple(w_aln), (k, aln[k], w_aln)
            assert left is None or (tuple(left[k]) == tuple(w_l) and tuple(right[k]) == tuple(w_r)), k
            gap_want[start[k]:start[k + 1]] = w_gaps
            if not score_only:
                text = et.cigar_binary_to_text(cg[k, :ln[k]].view("<u4")) if binary else cg[k, :ln[k]].tobytes().decode()
                assert text == w_cigar and (cg[k, ln[k]:] == 0xEE).all(), k  # nothing at or beyond cigar_len
    assert (gs[:-1] == gap_want).all()  # 0 behind a last anchor, for a refused pair's anchors and for anchors of no pair
    return seen


def test_statuses_canaries_overflow_slot_reuse_score_only_and_binary(aligner):
    from mgl_amd import _lib
    from mgl_amd import smithwaterman as sw

    Ts, Qs, chains = _status_batch()
    n, band, zdrop = len(Ts), 20, 2000
    bad, unsup, over = _lib.ERR_BAD_ARG, _lib.ERR_UNSUPPORTED, _lib.ERR_CIGAR_OVERFLOW
    good = lambda k: k not in BAD and k != UNSUP_GAP  # noqa: E731
    want = [_want(Ts[k], Qs[k], _tuples(chains[k]), GATK, band, zdrop, True, False) if good(k) else None for k in range(n)]
    lens = sorted(len(w[1]) for w in want if w)
    stride = min((x for x in lens if x % 4), key=lambda x: abs(x - lens[len(lens) // 2]))  # the CIGAR length nearest the median that is no multiple of four
    exact = [k for k in range(n) if want[k] and len(want[k][1]) == stride]
    assert exact and stride % 4 and stride >= 8 and lens[0] < stride - 1 and lens[-1] > stride
    statuses = [bad if k in BAD else unsup if k == UNSUP_GAP else 0 for k in range(n)]
    max_tl, max_ql = max(len(T) for T in Ts), max(len(Q) for Q in Qs)

    # ---- the default workspace: every status, canaries, the median CIGAR fits its row exactly
    outs, start = _device_call(aligner, Ts, Qs, chains, band, zdrop, stride, max_tl, max_ql)
    assert aligner.timing().dp_launches == 3
    seen = _check_outputs(outs, start, want, n, stride, statuses)
    assert seen == {0, bad, over, unsup}
    # one byte less: the pairs that fitted exactly overflow, and nothing else changes
    outs1, _ = _device_call(aligner, Ts, Qs, chains, band, zdrop, stride - 1, max_tl, max_ql)
    _check_outputs(outs1, start, want, n, stride - 1, statuses)
    assert all(outs[6][k] == 0 and outs1[6][k] == over for k in exact)

    # ---- slot reuse: a context of its own with the smallest workspace there is, 1 MiB, and gap bounds that make a fill slot larger
    # than what the staging leaves: every gap of the batch goes through the one slot, and the results are the same
    small_ws = sw.MicrosoftSmithWaterman(0)
    try:
        small_ws.set_workspace(1 << 20)
        outs_small, _ = _device_call(small_ws, Ts, Qs, chains, band, zdrop, stride, max_tl, max_ql, max_gap=(4000, 4000))
    finally:
        small_ws.close()
    small_statuses = list(statuses)
    small_statuses[UNSUP_GAP] = 0  # (the bounds admit its gap of 129 bases now)
    want_small = list(want)
    want_small[UNSUP_GAP] = _want(Ts[UNSUP_GAP], Qs[UNSUP_GAP], _tuples(chains[UNSUP_GAP]), GATK, band, zdrop, True, False)
    _check_outputs(outs_small, start, want_small, n, stride, small_statuses)
    same = [k for k in range(n) if k != UNSUP_GAP]
    for x in (0, 1, 2, 4, 5, 6):  # (the gap scores are per anchor: _check_outputs has compared them)
        assert (outs[x].reshape(n + 1, -1)[same] == outs_small[x].reshape(n + 1, -1)[same]).all()

    # ---- without the side records, and score-only with no CIGAR byte written
    outs2, _ = _device_call(aligner, Ts, Qs, chains, band, zdrop, stride, max_tl, max_ql, sides=False)
    _check_outputs(outs2, start, want, n, stride, statuses)
    outs3, _ = _device_call(aligner, Ts, Qs, chains, band, zdrop, stride, max_tl, max_ql, score_only=True)
    _check_outputs(outs3, start, want, n, stride, statuses, score_only=True)
    assert (outs3[4] == 0xEE).all()

    # ---- binary CIGAR in rows that do not start on a multiple of four: the text's elements
    counts = sorted(len(stb.elements(w[1])) for w in want if w)
    bstride = 4 * counts[len(counts) // 2] + 3  # the median number of elements fits exactly
    outs4, _ = _device_call(aligner, Ts, Qs, chains, band, zdrop, bstride, max_tl, max_ql, binary=True)
    seen = _check_outputs(outs4, start, want, n, bstride, statuses, binary=True)
    assert seen == {0, bad, over, unsup} and (outs4[6][:n] == 0).sum() >= len(counts) // 2 > 10 and counts[-1] > bstride // 4

    # ---- the sum guard: at a gopen of 2^24 every segment alone passes the range guard, and the chain of 40 anchors does not pass the sum
    huge = (200, -150, 1 << 24, 11)
    assert all(ct.chain_sum_ok(len(Ts[k]), len(Qs[k]), len(chains[k]), *bt.normalize(*huge)) == (k != UNSUP_SUM) for k in range(n))
    want5 = [_want(Ts[k], Qs[k], _tuples(chains[k]), huge, band, -1, True, False) if good(k) and k != UNSUP_SUM else None for k in range(n)]
    statuses5 = list(statuses)
    statuses5[UNSUP_SUM] = unsup
    outs5, _ = _device_call(aligner, Ts, Qs, chains, band, -1, 400, max_tl, max_ql, params=huge)
    _check_outputs(outs5, start, want5, n, 400, statuses5)
    assert statuses[UNSUP_SUM] == 0 and outs[6][UNSUP_SUM] in (0, over)


def test_one_anchor_is_the_seed_entry_byte_for_byte(aligner):
    rng = np.random.default_rng(23)
    Ts, Qs, chains = [], [], []
    for k in range(40):
        lt, rt = FLANKS[k % 4] + (k // 8), FLANKS[(k // 4) % 4] + (k % 3)
        T, Q, c = chain_pair(rng, (lt, max(0, lt + k % 3 - 1), rt, max(0, rt + (k // 3) % 3 - 1)), [], [(1, 20, 50)[k % 3]], exact=bool(k % 5))
        Ts.append(T), Qs.append(Q), chains.append(c)
    dev = torch.device("cuda", 0)
    g = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    n = len(Ts)
    max_tl, max_ql = max(len(T) for T in Ts), max(len(Q) for Q in Qs)
    for binary, stride, adaptive, to_qend in ((False, 41, False, True), (True, 4 * 9 + 2, True, False)):
        (aln, left, right, gs, cg, ln, st), start = _device_call(aligner, Ts, Qs, chains, 31, 1500, stride, max_tl, max_ql, to_qend=to_qend, adaptive=adaptive,
                                                                 binary=binary, broken=False)
        tl, ql = np.array([len(t) for t in Ts], np.int32), np.array([len(q) for q in Qs], np.int32)
        toff, qoff = np.concatenate([[0], np.cumsum(tl)[:-1]]).astype(np.int64), np.concatenate([[0], np.cumsum(ql)[:-1]]).astype(np.int64)
        sd = np.array([c[0] for c in chains], np.int32)
        td, qd = g(np.frombuffer(b"".join(Ts) + b"\0" * 8, np.uint8).copy()), g(np.frombuffer(b"".join(Qs) + b"\0" * 8, np.uint8).copy())
        out = (torch.full((n, 8), -77, dtype=torch.int32, device=dev), torch.full((n + 1, 8), -77, dtype=torch.int32, device=dev),
               torch.full((n + 1, 8), -77, dtype=torch.int32, device=dev), torch.full(((n + 1) * stride,), 0xEE, dtype=torch.uint8, device=dev),
               torch.full((n + 1,), -77, dtype=torch.int32, device=dev), torch.full((n + 1,), -77, dtype=torch.int32, device=dev))
        aligner.extend_seed_device(td, g(toff), g(tl), qd, g(qoff), g(ql), g(sd[:, 0].copy()), g(sd[:, 1].copy()), g(sd[:, 2].copy()), max_tl, max_ql, 31, 1500, GATK,
                                   to_qend, stride, binary, False, out=out, adaptive_band=adaptive, sides=True)
        torch.cuda.synchronize()
        s_aln, s_left, s_right, s_cg, s_ln, s_st = [x.cpu().numpy() for x in out]
        assert (aln[:n] == s_aln).all() and (left == s_left).all() and (right == s_right).all() and (cg == s_cg).all() and (ln == s_ln).all() and (st == s_st).all()
        assert (st[:n] == 0).sum() > 10 and set(st[:n]) <= {0, 2} and (gs[:-1] == 0).all()


def _golden_chain(g, every=200, sl=20):
    """exact anchors of sl bases about every `every` target bases on the golden path of a long pair"""
    off, ez, cigar = bt.banded_align_np(g.t, g.q, *g.params, g.strategy, 512)
    assert "sha1:" + hashlib.sha1(cigar.encode()).hexdigest() == g.cigar and off == g.offset  # band 512 holds the golden path
    (i, j), els = bt.path_cells(len(g.t), len(g.q), g.strategy, off, cigar)
    anchors = []
    for op, n in els:
        if op == "M":
            x = 0
            while x + sl <= n:
                if (not anchors or i + x >= anchors[-1][0] + every) and g.t[i + x:i + x + sl] == g.q[j + x:j + x + sl]:
                    anchors.append((i + x, j + x, sl))
                    x += sl
                else:
                    x += 1
            i, j = i + n, j + n
        elif op == "I":
            j += n
        else:
            i += n
    return anchors


def test_the_10_kb_pair_chained_through_anchors_on_its_golden_path_at_band_64(aligner):
    recs = [g for g in golden_io.load("long") if len(g.t) >= 9000 and len(g.q) >= 9000 and g.strategy != bt.IGNORE]
    assert recs
    g = recs[0]
    anchors = _golden_chain(g)
    assert 30 <= len(anchors) <= 51
    for adaptive in (False, True):
        (aln, cigar, l, r, gaps), = _check(aligner, [g.t], [g.q], [anchors], 64, 400 * 11, g.params, True, adaptive)
        assert aln.dropped == 0 and aln.t_beg < 300 and aln.t_end > 9700 and et.cigar_score(cigar, g.t[aln.t_beg:aln.t_end], g.q[aln.q_beg:aln.q_end], *g.params) == aln.score
