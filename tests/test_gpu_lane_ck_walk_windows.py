"""sw_dp16_lane_ck_kernel, pass 2: for ASCII input the walks compare the bases of the CALLER's arrays -- aligned 16-byte blocks, a
funnel shift by the low four bits of the window's address (SeqBlocks, sw_dp16_lane_ck.hip) -- instead of the wave's staged copies;
2-bit input and MGL_SW_DEBUG_WALK_STAGED=1 keep the staged windows.  The shapes are the smallest at which the loader can go wrong:
walks whose first 64-base window starts in front of the sequence (I, J < 64 and < 16), ends exactly at 64, or needs a second
iteration; sequences that start at every byte of a 16-byte block and arrays that end with their last pair; gaps at every distance
from a kept row and next to a block's left edge, so that the edge check's 16-base window decides; bytes outside ACGT inside a
window.  Everything is compared with the oracle byte for byte, and where a case is about the loader with the staged form too."""
import numpy as np
import pytest

import oracle_lib as ol
from mgl_amd import smithwaterman as sw

pytestmark = pytest.mark.gpu

GATK = (200, -150, 260, 11)
OTHER = (25, -50, 110, 6)  # no folded diagonal: the unfolded kernels
LANE16_CK = 7
CK = 32  # LANE_CK_COLS: query columns per recomputed block
TLS, QLS = (64, 80, 97), (17, 33, 63, 64, 65, 70)
ACGT = np.frombuffer(b"ACGT", np.uint8)


def _batch(tl, ql, seed, n, outside=True):
    """Reads cut from their targets with a few substitutions and, two in three, one gap whose place runs through every column
    and whose row therefore through every distance from a kept row; unrelated pairs; with `outside`, bytes that are no ACGT
    inside the aligned part: N in the read, a against A, N in the target alone and N against N."""
    rng = np.random.default_rng(seed)
    ts, qs, gaps = [], [], []
    for k in range(n):
        t = ACGT[rng.integers(0, 4, tl)].copy()
        s = int(rng.integers(0, max(1, tl - ql + 1))) if tl >= ql else 0
        src = np.concatenate([t[s:], ACGT[rng.integers(0, 4, ql + 24)]])
        gap = None
        if k % 3 != 2 and ql > 8:
            at, g = 2 + (k * 7) % (ql - 4), 1 + k % 5
            if k % 3 == 0:  # bases of the target missing from the read: the walk goes up g rows at column `at`
                src = np.concatenate([src[:at], src[at + g:]])
                gap = (s + at + g, at)  # the cell below the gap: (row, column), 1-based
            else:  # foreign bases in the read: the walk goes left g columns
                src = np.concatenate([src[:at], ACGT[rng.integers(0, 4, g)], src[at:]])
                gap = (s + at, at + g)
        q = src[:ql].copy()
        if k % 11 == 3:
            q = ACGT[rng.integers(0, 4, ql)]
            gap = None
        elif k % 4 == 1:
            q[int(rng.integers(0, ql))] = ACGT[int(rng.integers(0, 4))]
        if outside and k % 8 == 6:  # a read with N and lower case against a clean target
            q[int(rng.integers(0, ql))] = ord("N")
            j = int(rng.integers(0, ql))
            q[j] = q[j] | 0x20
        if outside and k % 16 == 7 and gap is None and k % 11 != 3:  # N in the target (its wave compares bytes), against N and against a base
            j = int(rng.integers(0, min(ql, tl - s) - 1))
            t[s + j] = t[s + j + 1] = q[j] = ord("N")
        ts.append(t.tobytes())
        qs.append(q.tobytes())
        gaps.append(gap)
    return ts, qs, gaps


@pytest.fixture()
def lane():
    a = sw.MicrosoftSmithWaterman(0)
    a.set_lane_kernel(2)
    yield a
    a.close()


_want = {}


def _oracle(key, ts, qs, params, strategy):
    k = (key, params, strategy)
    if k not in _want:
        _want[k] = ol.oracle_align_batch(ts, qs, params, strategy, nthreads=8)
    return _want[k]


def _same(res, want, what):
    off, sc, cg = want
    assert (np.asarray(res.offsets) == off).all(), what
    assert (np.asarray(res.scores) == sc).all(), what
    assert list(res.cigars) == list(cg), what


def _both_forms(lane, monkeypatch, key, ts, qs, params, strategy, **kw):
    """the caller's arrays and, with the debug switch, the staged copies: each against the oracle (so also against each other)"""
    want = _oracle(key, ts, qs, params, strategy)
    for staged in ("0", "1"):
        monkeypatch.setenv("MGL_SW_DEBUG_WALK_STAGED", staged)
        res = lane.align_batch(ts, qs, params, strategy, **kw)
        assert lane.timing().fill_kernel == LANE16_CK, (key, params, strategy)
        _same(res, want, (key, params, strategy, "staged" if staged == "1" else "caller's arrays"))
    monkeypatch.delenv("MGL_SW_DEBUG_WALK_STAGED")


@pytest.mark.parametrize("tl", TLS)
def test_geometries(lane, monkeypatch, tl):
    """Every window shape: ql = 17 (every window starts in front of the read; the first one of the target too where the read lies
    at its start), 33 and 63 (the first 64-base window starts in front), 64 (it starts at the read's first base), 65 and 70 (a
    second iteration, whose window starts in front).  Odd and even pair counts from 129 to 385.
    A launch of ONE geometry takes this kernel where 32-row strips suit the target (tl = 64); targets of 80 and 97 rows reach it in
    a grouped launch -- the six geometries in one batch, whole waves of each (the rest of each geometry goes through the
    eight-pairs-per-wave kernel) -- where the strips are 32 rows whatever the target."""
    counts = (129, 385, 130, 257, 131, 200)
    if tl == 64:
        for n, ql in zip(counts, QLS):
            ts, qs, _ = _batch(tl, ql, tl * 1000 + ql, n)
            _both_forms(lane, monkeypatch, (tl, ql), ts, qs, GATK, ol.SOFTCLIP)
            _both_forms(lane, monkeypatch, (tl, ql), ts, qs, GATK, ol.INDEL)
        return
    ts, qs = [], []
    for n, ql in zip(counts, QLS):
        t1, q1, _ = _batch(tl, ql, tl * 1000 + ql, n)
        ts += t1
        qs += q1
    order = np.random.default_rng(tl).permutation(len(ts))
    ts, qs = [ts[k] for k in order], [qs[k] for k in order]
    assert len(ts) >= 1024  # (the library sorts batches of 1 024 pairs and more)
    monkeypatch.setenv("MGL_SW_DEBUG_LANE_GROUP_MIN", "128")
    a = sw.MicrosoftSmithWaterman(0)
    a.set_small_kernel(1)  # (a batch this small would go to the one-wave-per-pair kernel)
    try:
        for strategy in (ol.SOFTCLIP, ol.INDEL):
            _both_forms(a, monkeypatch, ("grouped", tl), ts, qs, GATK, strategy, cigar_stride=256)
    finally:
        a.close()


def test_gaps_at_every_distance(lane, monkeypatch):
    """125 x 70, 385 pairs: the cell below (right of) a gap lies 1, 15, 16 and 17 rows below a kept row -- rows 16 m + 1, 16 m + 15,
    16 m + 16 = the kept row itself, 16 m + 17 -- and in the first column right of a block's left edge, where the stuck walk's
    16-base window (PathWalk::edge_apply) decides whether the block on this side is recomputed.  All four strategies, parameters
    that fold and parameters that do not."""
    tl, ql = 125, 70
    ts, qs, gaps = _batch(tl, ql, 97070, 385, outside=False)
    rows = {(g[0] - 1) % 16 + 1 for g in gaps if g}
    assert {1, 15, 16} <= rows and any(g and g[0] > 17 and (g[0] - 1) % 16 == 0 for g in gaps), sorted(rows)
    assert any(g and g[1] % CK == 1 and g[1] > CK for g in gaps) and any(g and g[1] % CK == 0 for g in gaps)
    for strategy in ol.STRATEGIES:
        _both_forms(lane, monkeypatch, "gaps", ts, qs, GATK, strategy)
    _both_forms(lane, monkeypatch, "gaps", ts, qs, OTHER, ol.SOFTCLIP)


def _device_run(lane, td, t_off, qd, q_off, tl, ql, params, strategy, kt, kq, cigar_stride=160):
    """the device-resident entry on arrays whose first byte stands at offset kt (kq) of a 16-byte block and whose last byte is the
    last pair's"""
    import torch
    from mgl_amd import device_batch as db

    dev = torch.device("cuda", 0)
    tbuf = torch.zeros(len(td) + kt, dtype=torch.uint8, device=dev)
    qbuf = torch.zeros(len(qd) + kq, dtype=torch.uint8, device=dev)
    assert tbuf.data_ptr() % 16 == 0 and qbuf.data_ptr() % 16 == 0
    tv, qv = tbuf[kt:], qbuf[kq:]
    tv.copy_(torch.from_numpy(td))
    qv.copy_(torch.from_numpy(qd))
    assert tv.data_ptr() % 16 == kt and qv.data_ptr() % 16 == kq
    b = db.DeviceBatch(tv, torch.from_numpy(t_off).to(dev), qv, torch.from_numpy(q_off).to(dev), tl, ql, cigar_stride, uniform=True)
    b.run(lane, params, strategy)
    torch.cuda.synchronize()
    assert lane.timing().fill_kernel == LANE16_CK
    assert not b.status.any().item()
    return b.offsets.cpu().numpy(), b.scores.cpu().numpy(), b.cigar_strings()


def test_every_alignment_and_exact_arrays(lane, monkeypatch):
    """125 x 70, 129 pairs, device resident: both arrays with the first pair's first byte at every offset 0 .. 15 of a 16-byte
    block (offset 0: at the allocation's first byte; the queries' offset is 5 kt + 3 mod 16), the arrays exactly as long as their pairs -- the last pair ends at the
    array's last byte, the first block of the first pair and the last block of the last one are the clamped ones.  With lengths
    of 125 and 70 the pairs inside the array start at every offset anyway; here the array's two ends do."""
    tl, ql, n = 125, 70, 129
    ts, qs, _ = _batch(tl, ql, 1597070, n)
    td, qd = np.frombuffer(b"".join(ts), np.uint8).copy(), np.frombuffer(b"".join(qs), np.uint8).copy()
    t_off, q_off = np.arange(n + 1, dtype=np.int64) * tl, np.arange(n + 1, dtype=np.int64) * ql
    off, sc, cg = _oracle("align", ts, qs, GATK, ol.SOFTCLIP)
    for kt in range(16):
        kq = (5 * kt + 3) % 16  # every offset once
        for staged in ("0", "1") if kt in (0, 15) else ("0",):
            monkeypatch.setenv("MGL_SW_DEBUG_WALK_STAGED", staged)
            got = _device_run(lane, td, t_off, qd, q_off, tl, ql, GATK, ol.SOFTCLIP, kt, kq)
            assert (got[0] == off).all() and (got[1] == sc).all() and got[2] == list(cg), (kt, kq, staged)
    assert sorted((5 * kt + 3) % 16 for kt in range(16)) == list(range(16))


def test_bases_outside_acgt(lane, monkeypatch):
    """N against N matches and a against A does not (test_lane_kernel_bases_outside_acgt), now inside the windows the walks
    check: a perfect read but for one such byte, so that the window holding it decides whether the stretch adds up."""
    tl, ql, n = 125, 65, 131
    rng = np.random.default_rng(8065)
    ts, qs = [], []
    for k in range(n):
        t = ACGT[rng.integers(0, 4, tl)].copy()
        s = int(rng.integers(0, tl - ql + 1))
        q = t[s:s + ql].copy()
        j = (k * 5) % ql
        if k % 4 == 0:
            t[s + j] = q[j] = ord("N")  # equal bytes: a match
        elif k % 4 == 1:
            q[j] = q[j] | 0x20  # a against A: a mismatch
        elif k % 4 == 2:
            t[s + j] = ord("N")  # N against a base
        else:
            q[j] = ord("N")
        ts.append(t.tobytes())
        qs.append(q.tobytes())
    for strategy in (ol.SOFTCLIP, ol.INDEL):
        _both_forms(lane, monkeypatch, "outside", ts, qs, GATK, strategy)
    sc = _oracle("outside", ts, qs, GATK, ol.SOFTCLIP)[1]  # (ScoreMax: the third field is the best score)
    assert sc[0][2] == ql * GATK[0] and sc[1][2] < ql * GATK[0], "the oracle itself: N against N is a match, a against A is none"


def test_other_launches(lane, monkeypatch):
    """The same pairs as 2-bit input (the staged windows, unchanged), through the unfolded kernels, with a CIGAR stride that is no
    multiple of four (the scatter kernels), and in a grouped launch of two geometries."""
    from mgl_amd import device_batch as db

    tl, ql = 125, 70
    ts, qs, _ = _batch(tl, ql, 2097070, 385, outside=False)
    tb, qb = db.pack2bit(b"".join(ts)), db.pack2bit(b"".join(qs))
    t_start, q_start = np.arange(len(ts), dtype=np.int64) * tl, np.arange(len(qs), dtype=np.int64) * ql
    for params in (GATK, OTHER):
        res = lane.align_packed_2bit(tb, tl * len(ts), t_start, None, qb, ql * len(qs), q_start, None, tl, ql, params, ol.INDEL)
        assert lane.timing().fill_kernel == LANE16_CK
        _same(res, _oracle("other", ts, qs, params, ol.INDEL), "2-bit")
        _both_forms(lane, monkeypatch, "other", ts, qs, params, ol.INDEL)
        _both_forms(lane, monkeypatch, "other", ts, qs, params, ol.LEAD_INDEL, cigar_stride=250)
    monkeypatch.setenv("MGL_SW_DEBUG_LANE_GROUP_MIN", "128")
    gt, gq = [], []
    for g_tl, g_ql in ((97, 70), (64, 33)):
        t1, q1, _ = _batch(g_tl, g_ql, 31 * g_tl + g_ql, 513)  # (the library sorts batches of 1 024 pairs and more)
        gt += t1
        gq += q1
    order = np.random.default_rng(5).permutation(len(gt))
    gt, gq = [gt[k] for k in order], [gq[k] for k in order]
    a = sw.MicrosoftSmithWaterman(0)
    a.set_small_kernel(1)
    try:
        res = a.align_batch(gt, gq, GATK, ol.SOFTCLIP, cigar_stride=256)
        assert a.timing().fill_kernel == LANE16_CK
        _same(res, _oracle("grouped", gt, gq, GATK, ol.SOFTCLIP), "grouped")
    finally:
        a.close()
