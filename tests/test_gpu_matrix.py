"""Substitution-matrix ("protein") scoring, SURVEY.md section 8f rank 4 / BASELINE configs[4].  The reference has no
such path, so NO parity with it is claimed: the GPU is compared (bit-exactly) with the CPU restatement's own
extension (oracle swo_*_matrix), and that extension with an independent textbook DP written here."""
import numpy as np
import pytest

import oracle_lib as ol
from mgl_amd import device_batch, protein, smithwaterman as sw


def textbook(t, q, code, mat, o, e, indel):
    """Affine-gap DP straight from the recurrence (no zero floor, mgl's borders): returns H as a numpy array."""
    tl, ql = len(t), len(q)
    NEG = -10 ** 9
    H = np.zeros((tl + 1, ql + 1), dtype=np.int64)
    E = np.full((tl + 2, ql + 1), NEG, dtype=np.int64)  # E[i][j]: gap entering (i, j) from above
    F = np.full((tl + 1, ql + 2), NEG, dtype=np.int64)  # F[i][j]: gap entering (i, j) from the left
    b = lambda k: (-o - (k - 1) * e) if (indel and k > 0) else 0
    for j in range(ql + 1):
        H[0][j] = b(j)
        E[1][j] = H[0][j] - o
    for i in range(1, tl + 1):
        H[i][0] = b(i)
        F[i][1] = H[i][0] - o
        for j in range(1, ql + 1):
            diag = H[i - 1][j - 1] + int(mat[code[t[i - 1]], code[q[j - 1]]])
            H[i][j] = max(diag, F[i][j], E[i][j])
            E[i + 1][j] = max(H[i][j] - o, E[i][j] - e)
            F[i][j + 1] = max(H[i][j] - o, F[i][j] - e)
    return H


def oracle_matrix_batch(ts, qs, code, mat, o, e, strategy, stride):
    import ctypes as C

    td, toff = sw.concat(ts)
    qd, qoff = sw.concat(qs)
    n = len(ts)
    off = np.zeros(n, np.int32); sc = np.zeros((n, 6), np.int32); cg = np.zeros(n * stride, np.uint8); ln = np.zeros(n, np.int32)
    L = ol.oracle()
    L.swo_align_batch_matrix.argtypes = [C.c_int] + [C.c_void_p] * 6 + [C.c_int] * 4 + [C.c_void_p] * 3 + [C.c_int, C.c_void_p]
    rc = L.swo_align_batch_matrix(n, td.ctypes.data, toff.ctypes.data, qd.ctypes.data, qoff.ctypes.data, code.ctypes.data,
                                  mat.ctypes.data, o, e, strategy, 4, off.ctypes.data, sc.ctypes.data, cg.ctypes.data, stride,
                                  ln.ctypes.data)
    assert rc == 0
    return off, sc, [cg[k * stride: k * stride + ln[k]].tobytes().decode() for k in range(n)]


def test_restatement_extension_against_textbook():
    """CPU only: last-column / last-row maxima of the extension equal those of the textbook DP."""
    rng = np.random.default_rng(2)
    code, mat = protein.blosum62()
    for trial in range(40):
        tl, ql = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        t = protein.random_proteins(rng, 1, tl)[0].tobytes()
        q = protein.random_proteins(rng, 1, ql)[0].tobytes()
        for strategy in ol.STRATEGIES:
            indel = strategy in (ol.INDEL, ol.LEAD_INDEL)
            H = textbook(t, q, code, mat, 11, 1, indel)
            _, sc, _ = oracle_matrix_batch([t], [q], code, mat, 11, 1, strategy, 4 * (tl + ql) + 16)
            mqe, mqe_t, mx = int(sc[0][0]), int(sc[0][1]), int(sc[0][2])
            col = H[1:, ql]
            assert mqe == col.max() and mqe_t == max(i + 1 for i in range(tl) if col[i] == col.max())
            assert mx == max(col.max(), H[tl, 1:].max())


def _asymmetric_matrix(rng, lo=-128, hi=127):
    """A random int8 matrix over [lo, hi] that reaches both ends and is far from symmetric (row = target code, column = query code)."""
    mat = rng.integers(lo, hi + 1, (32, 32))
    mat[3, 17], mat[17, 3], mat[29, 8], mat[8, 29] = lo, hi, hi, lo
    assert (mat != mat.T).sum() > 800
    return mat.astype(np.int8)


def _all_codes(rng):
    """A byte -> code table that uses all 32 codes, eight bytes each, in random order."""
    return rng.permutation(np.arange(256) % 32).astype(np.uint8)


def _maxima(H, tl, ql):
    col = H[1:, ql]
    return int(col.max()), max(i + 1 for i in range(tl) if col[i] == col.max()), int(max(col.max(), H[tl, 1:].max()))


def test_restatement_extension_orientation_against_textbook():
    """CPU only: the extension reads matrix[code[t]][code[q]] (row = target) -- asymmetric matrices over all of int8, code tables over
    all 32 codes, sequences of arbitrary bytes, gap penalties with o == e and e == 0 -- and the check can see a transposition."""
    rng = np.random.default_rng(23)
    transposed_differs = 0
    for trial in range(32):
        mat, code = _asymmetric_matrix(rng), _all_codes(rng)
        o, e = [(127, 1), (5, 5), (9, 0), (0, 0), (40, 3), (1, 1), (128, 0), (3, 2)][trial % 8]
        tl, ql = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        t, q = rng.integers(0, 256, tl).astype(np.uint8).tobytes(), rng.integers(0, 256, ql).astype(np.uint8).tobytes()
        for strategy in ol.STRATEGIES:
            indel = strategy in (ol.INDEL, ol.LEAD_INDEL)
            H = textbook(t, q, code, mat, o, e, indel)
            _, sc, _ = oracle_matrix_batch([t], [q], code, mat, o, e, strategy, 4 * (tl + ql) + 16)
            assert (int(sc[0][0]), int(sc[0][1]), int(sc[0][2])) == _maxima(H, tl, ql), (trial, strategy)
            transposed_differs += _maxima(textbook(t, q, code, mat.T, o, e, indel), tl, ql) != _maxima(H, tl, ql)
    assert transposed_differs >= 96   # (the power of this test: a reader of mat[q][t] fails most cases, not one)


@pytest.mark.gpu
def test_blosum62_batches_bit_exact():
    import torch

    rng = np.random.default_rng(4)
    code, mat = protein.blosum62()
    a = sw.MicrosoftSmithWaterman(0)
    assert a.load()
    for strategy, (o, e) in zip(ol.STRATEGIES, [(11, 1), (10, 2), (5, 5), (12, 1)]):
        ts, qs = [], []
        for k in range(300):
            tl, ql = int(rng.integers(1, 700)), int(rng.integers(1, 400))
            t = protein.random_proteins(rng, 1, tl)[0]
            if k % 3 and tl > 20:   # a diverged homologue of part of the target
                s = int(rng.integers(0, tl - 10)); q = t[s:s + ql].copy()
                mut = rng.random(len(q)) < 0.3
                q[mut] = protein.random_proteins(rng, 1, int(mut.sum()))[0] if mut.any() else q[mut]
                if len(q) > 8: q = np.delete(q, rng.integers(0, len(q), size=2))
            else:
                q = protein.random_proteins(rng, 1, ql)[0]
            if k % 17 == 0: q = np.concatenate([q, np.frombuffer(b"BZX*ux", np.uint8)])   # ambiguity codes, lower case, junk
            ts.append(t.tobytes()); qs.append(q.tobytes())
        td, toff = sw.concat(ts); qd, qoff = sw.concat(qs)
        stride = 2 * 800
        b = device_batch.from_host(td, toff, qd, qoff, "cuda:0", cigar_stride=stride)
        protein.run_matrix(b, a, code, mat, o, e, strategy)
        torch.cuda.synchronize()
        assert int((b.status != 0).sum()) == 0
        off, sc, cg = oracle_matrix_batch(ts, qs, code, mat, o, e, strategy, stride)
        assert (b.offsets.cpu().numpy() == off).all()
        assert (b.scores.cpu().numpy() == sc).all()
        assert b.cigar_strings() == cg
    # one geometry per block of eight pairs: the packed-int16 kernel with the table S - max S in LDS, all strategies
    for strategy, (o, e) in zip(ol.STRATEGIES, [(11, 1), (10, 2), (7, 3), (12, 1)]):
        ts, qs = [], []
        for g in range(40):
            tl, ql = int(rng.integers(20, 500)), int(rng.integers(33, 330))
            for k in range(8):
                t = protein.random_proteins(rng, 1, tl)[0]
                if k % 2 and tl > ql:
                    s0 = int(rng.integers(0, tl - ql + 1)); q = t[s0:s0 + ql].copy()
                    mut = rng.random(ql) < 0.35
                    q[mut] = protein.random_proteins(rng, 1, int(mut.sum()))[0] if mut.any() else q[mut]
                else:
                    q = protein.random_proteins(rng, 1, ql)[0]
                ts.append(t.tobytes()); qs.append(q.tobytes())
        td, toff = sw.concat(ts); qd, qoff = sw.concat(qs)
        b = device_batch.from_host(td, toff, qd, qoff, "cuda:0", cigar_stride=1200)
        protein.run_matrix(b, a, code, mat, o, e, strategy, grouped=True)
        torch.cuda.synchronize()
        assert a.timing().packed16 == 1 and int((b.status != 0).sum()) == 0
        off, sc, cg = oracle_matrix_batch(ts, qs, code, mat, o, e, strategy, 1200)
        assert (b.offsets.cpu().numpy() == off).all() and (b.scores.cpu().numpy() == sc).all() and b.cigar_strings() == cg
        protein.run_matrix(b, a, code, mat, o, e, strategy, grouped=False)   # the same pairs through the int32 kernel
        torch.cuda.synchronize()
        assert a.timing().packed16 == 0
        assert (b.offsets.cpu().numpy() == off).all() and (b.scores.cpu().numpy() == sc).all() and b.cigar_strings() == cg
    # a DNA match / mismatch matrix reproduces the reference's scoring exactly
    dcode = np.zeros(256, np.uint8)
    for k, ch in enumerate(b"ACGT"): dcode[ch] = k + 1
    dmat = np.full((32, 32), -75, np.int8)   # int8 range: (100, -75) instead of (200, -150)
    for k in range(1, 5): dmat[k, k] = 100
    gs = [g for g in __import__("golden_io").load("window")[:64]]
    ts = [g.t for g in gs]; qs = [g.q for g in gs]
    td, toff = sw.concat(ts); qd, qoff = sw.concat(qs)
    b = device_batch.from_host(td, toff, qd, qoff, "cuda:0", cigar_stride=512)
    protein.run_matrix(b, a, dcode, dmat, 130, 6, ol.SOFTCLIP)
    torch.cuda.synchronize()   # the host entry below runs on the context's own stream and shares its workspace
    ref = a.align_batch(ts, qs, (100, -75, 130, 6), ol.SOFTCLIP, cigar_stride=512)
    assert (b.offsets.cpu().numpy() == ref.offsets).all() and (b.scores.cpu().numpy() == ref.scores).all()
    assert b.cigar_strings() == list(ref.cigars)
    # a 2 000-residue query takes the one-pair-per-wave variant of the matrix kernel
    long_t = protein.random_proteins(rng, 1, 2500)[0]
    long_q = np.concatenate([long_t[300:1500], protein.random_proteins(rng, 1, 800)[0]])
    b = device_batch.from_host(*sw.concat([long_t.tobytes()] * 3), *sw.concat([long_q.tobytes()] * 3), "cuda:0", cigar_stride=8192)
    protein.run_matrix(b, a, code, mat, 11, 1, ol.SOFTCLIP)
    torch.cuda.synchronize()
    off, sc, cg = oracle_matrix_batch([long_t.tobytes()] * 3, [long_q.tobytes()] * 3, code, mat, 11, 1, ol.SOFTCLIP, 8192)
    assert (b.offsets.cpu().numpy() == off).all() and (b.scores.cpu().numpy() == sc).all() and b.cigar_strings() == cg
    # too long a query for the matrix kernel's LDS carve
    long_q = protein.random_proteins(rng, 1, 5000)[0].tobytes()
    b = device_batch.from_host(*sw.concat([long_q]), *sw.concat([long_q]), "cuda:0")
    with pytest.raises(Exception) as ex:
        protein.run_matrix(b, a, code, mat)
    assert "too long" in str(ex.value)
    a.close()


def _tiles(rng, shapes, last_count):
    """Tiles of 128 pairs that share their target (the last one `last_count` pairs): queries of one length per tile, diverged
    fragments of the target, unrelated sequences, ambiguity codes, lower case and junk bytes among them."""
    ts, qs = [], []
    for k, (tl, ql) in enumerate(shapes):
        t = protein.random_proteins(rng, 1, tl)[0]
        for p in range(last_count if k == len(shapes) - 1 else 128):
            if p % 3 and tl >= ql:
                s0 = int(rng.integers(0, tl - ql + 1)); q = t[s0:s0 + ql].copy()
                mut = rng.random(ql) < 0.3
                if mut.any(): q[mut] = protein.random_proteins(rng, 1, int(mut.sum()))[0]
            else:
                q = protein.random_proteins(rng, 1, ql)[0]
            if p % 19 == 0 and ql >= 6: q[-6:] = np.frombuffer(b"BZX*u!", np.uint8)
            ts.append(t.tobytes()); qs.append(q.tobytes())
    return ts, qs


def _shared_batch(ts, qs, dev, stride):
    """IndexedBatch over ONE copy of each tile's target: pair k points at its tile's target (the promise of MGL_SW_FLAG_SHARED_TARGET)."""
    import torch

    tdata, t_start, t_len, seen = [], [], [], {}
    pos = 0
    for k, t in enumerate(ts):
        key = (k // 128, t)
        if key not in seen:
            seen[key] = pos; tdata.append(np.frombuffer(t, np.uint8)); pos += len(t)
        t_start.append(seen[key]); t_len.append(len(t))
    qd, qoff = sw.concat(qs)
    return protein.IndexedBatch(torch.from_numpy(np.concatenate(tdata)).to(dev), torch.tensor(t_start, dtype=torch.int64, device=dev),
                                torch.tensor(t_len, dtype=torch.int32, device=dev), torch.from_numpy(qd).to(dev),
                                torch.from_numpy(qoff[:-1].copy()).to(dev), torch.from_numpy(np.diff(qoff).astype(np.int32)).to(dev),
                                max(len(t) for t in ts), max(len(q) for q in qs), stride)


@pytest.mark.gpu
def test_tiles_that_share_their_target_bit_exact(monkeypatch):
    """MGL_SW_FLAG_SHARED_TARGET (sw_dp16_lane_matrix.hip): tiles of 128 pairs on one target, two pairs per lane, the scores of a column out
    of the strip's profile -- against the CPU restatement's extension, every strategy, strips that end inside a target, queries of 1 .. 301
    residues, a short last tile with an odd pair count; a grid of five wave slots (the tiles outnumber them: the counter, twice on one
    context); parameters the byte table cannot hold (the flag is then read as the grouped promise); a tile that breaks the promise."""
    import torch

    rng = np.random.default_rng(11)
    code, mat = protein.blosum62()
    dev = torch.device("cuda", 0)
    shapes = [(1, 1), (5, 3), (31, 4), (32, 5), (33, 7), (63, 33), (64, 150), (65, 301), (100, 2), (257, 64), (700, 300), (96, 299), (40, 40), (333, 130)]
    a = sw.MicrosoftSmithWaterman(0)
    for strategy, (o, e) in zip(ol.STRATEGIES, [(11, 1), (10, 2), (5, 5), (12, 1)]):
        ts, qs = _tiles(rng, shapes, 77)
        b = _shared_batch(ts, qs, dev, 1024)
        off, sc, cg = oracle_matrix_batch(ts, qs, code, mat, o, e, strategy, 1024)
        for slots in (None, "5", "5"):
            if slots: monkeypatch.setenv("MGL_SW_DEBUG_LANE_SLOTS", slots)
            b.offsets.fill_(-7); b.scores.fill_(-7); b.status.fill_(-7)
            protein.run_matrix(b, a, code, mat, o, e, strategy, shared_target=True)
            torch.cuda.synchronize()
            monkeypatch.delenv("MGL_SW_DEBUG_LANE_SLOTS", raising=False)
            assert a.fill_kernel_name(a.timing()) == "sw_dp16_lane_matrix_kernel"
            assert int((b.status != 0).sum()) == 0
            assert (b.offsets.cpu().numpy() == off).all() and (b.scores.cpu().numpy() == sc).all() and b.cigar_strings() == cg
        # MGL_SW_FLAG_SCORE_ONLY: the same six fields without flags, regions or walk
        b.scores.fill_(-7); b.offsets.fill_(-7); b.cigar_len.fill_(-7)
        protein.run_matrix(b, a, code, mat, o, e, strategy, shared_target=True, score_only=True)
        torch.cuda.synchronize()
        assert a.fill_kernel_name(a.timing()) == "sw_dp16_lane_matrix_kernel"
        assert (b.scores.cpu().numpy() == sc).all() and int(b.offsets.abs().sum()) == 0 and int(b.cigar_len.abs().sum()) == 0 and int((b.status != 0).sum()) == 0
        # MGL_SW_FLAG_BINARY_CIGAR: BAM-style uint32 elements, the same elements in the same order as the text
        protein.run_matrix(b, a, code, mat, o, e, strategy, shared_target=True, binary_cigar=True)
        torch.cuda.synchronize()
        raw, ln = b.cigars.cpu().numpy(), b.cigar_len.cpu().numpy()
        for k in range(0, len(cg), 37):
            el = np.frombuffer(raw[k, : ln[k]].tobytes(), dtype="<u4")
            assert "".join(f"{int(v) >> 4}{'MIDNS'[int(v) & 15]}" for v in el) == cg[k]
        a.check()
    # gap penalties under which an entry S + e + o is negative: the byte table cannot hold them, the batch takes the packed kernel
    ts, qs = _tiles(rng, shapes[3:9], 128)
    b = _shared_batch(ts, qs, dev, 1024)
    protein.run_matrix(b, a, code, mat, 2, 1, ol.SOFTCLIP, shared_target=True)
    torch.cuda.synchronize()
    assert a.fill_kernel_name(a.timing()) == "sw_dp16_kernel"
    off, sc, cg = oracle_matrix_batch(ts, qs, code, mat, 2, 1, ol.SOFTCLIP, 1024)
    assert (b.offsets.cpu().numpy() == off).all() and (b.scores.cpu().numpy() == sc).all() and b.cigar_strings() == cg
    # a broken promise: one pair of tile 2 points one residue further into the targets, one pair of tile 4 has a shorter query -- those two
    # tiles are NOT computed (MGL_SW_ERR_BAD_ARG for their pairs), the others are right
    ts, qs = _tiles(rng, [(64, 50)] * 6, 128)
    b = _shared_batch(ts, qs, dev, 512)
    b.t_off[2 * 128 + 77] += 1
    b.q_len[4 * 128 + 5] -= 1
    b.status.fill_(0)
    protein.run_matrix(b, a, code, mat, 11, 1, ol.SOFTCLIP, shared_target=True)
    torch.cuda.synchronize()
    st = b.status.cpu().numpy().reshape(6, 128)
    assert (st[[2, 4]] == 1).all() and (st[[0, 1, 3, 5]] == 0).all()
    off, sc, cg = oracle_matrix_batch(ts, qs, code, mat, 11, 1, ol.SOFTCLIP, 512)
    good = np.repeat(np.array([1, 1, 0, 1, 0, 1], bool), 128)
    assert (b.offsets.cpu().numpy()[good] == off[good]).all() and (b.scores.cpu().numpy()[good] == sc[good]).all()
    assert [c for c, g in zip(b.cigar_strings(), good) if g] == [c for c, g in zip(cg, good) if g]
    # a caller whose max_tl is smaller than a tile's target: that tile does not fit its region and is refused the same way
    ts, qs = _tiles(rng, [(40, 30), (90, 30), (40, 30)], 128)
    b = _shared_batch(ts, qs, dev, 512)
    b.max_tl = 64
    protein.run_matrix(b, a, code, mat, 11, 1, ol.SOFTCLIP, shared_target=True)
    torch.cuda.synchronize()
    st = b.status.cpu().numpy().reshape(3, 128)
    assert (st[1] == 1).all() and (st[[0, 2]] == 0).all()
    a.close()


@pytest.mark.gpu
def test_database_search_layout_every_pair_where_it_says():
    """mgl_amd.protein.DatabaseSearch: 136 queries against 9 database sequences -- tiles of 128 per sequence (longest first), 8 queries beyond
    whole tiles, two sequences too long for the tile class -- every (d, q) found by where() and equal to the CPU restatement's extension."""
    import torch

    rng = np.random.default_rng(5)
    code, mat = protein.blosum62()
    lens = np.array([60, 333, 41, 700, 129, 64, 1200, 95, 256])
    db_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    db = protein.random_proteins(rng, 1, int(db_off[-1]))[0]
    Q, QL = 136, 70
    queries = protein.random_proteins(rng, Q, QL)
    for q in range(0, Q, 3):   # diverged fragments of database sequences
        d = int(rng.integers(0, len(lens)))
        if lens[d] >= QL:
            s0 = int(rng.integers(0, lens[d] - QL + 1)); frag = db[db_off[d] + s0: db_off[d] + s0 + QL].copy()
            mut = rng.random(QL) < 0.3
            frag[mut] = protein.random_proteins(rng, 1, int(mut.sum()))[0]
            queries[q] = frag
    ds = protein.DatabaseSearch(db, db_off, queries, torch.device("cuda", 0), cigar_stride=1024, shared_max_tl=512)
    assert ds.shared.n == 7 * 128 and ds.rest.n == 7 * 8 and ds.long.n == 2 * Q and ds.shared_max_tl == 512
    a = sw.MicrosoftSmithWaterman(0)
    ds.run(a, code, mat, 11, 1, ol.SOFTCLIP)
    torch.cuda.synchronize()
    ts = [db[db_off[d]:db_off[d + 1]].tobytes() for d in range(len(lens)) for q in range(Q)]
    qs = [queries[q].tobytes() for d in range(len(lens)) for q in range(Q)]
    off, sc, cg = oracle_matrix_batch(ts, qs, code, mat, 11, 1, ol.SOFTCLIP, 1024)
    host = {id(b): (b.offsets.cpu().numpy(), b.scores.cpu().numpy(), b.status.cpu().numpy(), b.cigar_strings()) for b in ds.batches()}
    seen = set()
    for d in range(len(lens)):
        for q in range(Q):
            b, p = ds.where(d, q)
            o_, s_, st_, c_ = host[id(b)]
            k = d * Q + q
            assert (id(b), p) not in seen and st_[p] == 0 and o_[p] == off[k] and (s_[p] == sc[k]).all() and c_[p] == cg[k], (d, q)
            seen.add((id(b), p))
    assert len(seen) == len(lens) * Q == sum(b.n for b in ds.batches())
    a.close()


# ---- every matrix kernel on inputs that are not mild: asymmetric full-range matrices, hot padding codes, ties, the range guards

def _dp16_range_ok(tl, ql, smax, smin, o, e):
    """dp16_range_ok (sw_dp16.hip) restated: can every stored value of a tl x ql problem be held in 16 bits?"""
    top = smax * min(tl, ql) + e * (tl + ql)
    low = -3 * o - (smax - smin) - 2 * e - 64
    return smax > 0 and o >= e and 32767 - top + low >= -32768 and smax - smin <= 30000 and o <= 10000 and e <= 5000 and smax + 2 * e <= 30000


def _query_of(rng, t, ql, letters):
    """A query of ql residues: every other one a mutated fragment of t with one residue deleted and one inserted, else random."""
    if rng.random() < 0.5 or len(t) < 4:
        return rng.choice(letters, ql)
    s0 = int(rng.integers(0, max(1, len(t) - ql - 1)))
    q = t[s0:s0 + ql + 1].copy()
    mut = rng.random(len(q)) < 0.2
    q[mut] = rng.choice(letters, int(mut.sum()))
    q = np.insert(np.delete(q, rng.integers(0, len(q))), rng.integers(0, len(q)), rng.choice(letters))
    return np.concatenate([q, rng.choice(letters, ql)])[:ql]


def _blocks(rng, letters, geoms, per, last=None):
    """`per` pairs for each (tl, ql) of geoms (the last geometry `last` pairs), the pairs of a geometry on ONE target."""
    ts, qs = [], []
    for k, (tl, ql) in enumerate(geoms):
        t = rng.choice(letters, tl)
        for _ in range(last if (last and k == len(geoms) - 1) else per):
            ts.append(t.tobytes()); qs.append(_query_of(rng, t, ql, letters).astype(np.uint8).tobytes())
    return ts, qs


def _stride(ts, qs):
    return (4 * (max(len(t) for t in ts) + max(len(q) for q in qs)) + 16 + 3) // 4 * 4


def _oracle_unique(ts, qs, code, mat, o, e, strategy, stride):
    """oracle_matrix_batch once per DISTINCT pair (the tiles repeat theirs)."""
    keys = {}
    idx = np.array([keys.setdefault(p, len(keys)) for p in zip(ts, qs)])
    off, sc, cg = oracle_matrix_batch([t for t, _ in keys], [q for _, q in keys], code, mat, o, e, strategy, stride)
    return off[idx], sc[idx], [cg[k] for k in idx]


def _run(a, kind, ts, qs, code, mat, o, e, strategy, stride, **kw):
    """One call on a fresh batch whose outputs are poisoned first: kind "mixed" (no promise), "grouped" or "shared" (tiles of 128)."""
    import torch

    if kind == "shared":
        b = _shared_batch(ts, qs, torch.device("cuda", 0), stride)
    else:
        b = device_batch.from_host(*sw.concat(ts), *sw.concat(qs), "cuda:0", cigar_stride=stride)
    for x in (b.offsets, b.scores, b.cigar_len, b.status):
        x.fill_(-7)
    protein.run_matrix(b, a, code, mat, o, e, strategy, grouped=kind == "grouped", shared_target=kind == "shared", **kw)
    torch.cuda.synchronize()
    return b, a.fill_kernel_name(a.timing())


def _assert_exact(b, ref, what):
    off, sc, cg = ref
    assert int((b.status != 0).sum()) == 0, what
    assert (b.scores.cpu().numpy() == sc).all(), what
    assert (b.offsets.cpu().numpy() == off).all(), what
    assert b.cigar_strings() == cg, what


def _assert_binary_cigar(b, cg, what):
    raw, ln = b.cigars.cpu().numpy(), b.cigar_len.cpu().numpy()
    for k in range(len(cg)):
        el = np.frombuffer(raw[k, : ln[k]].tobytes(), dtype="<u4")
        assert "".join(f"{int(v) >> 4}{'MIDNS'[int(v) & 15]}" for v in el) == cg[k], (what, k)


def _every_matrix_path(a, rng, code, mat, letters, o, e, strategy, mixed_geoms, geoms, long_geoms, shared_kernel="sw_dp16_lane_matrix_kernel",
                       flags=False, negate=False):
    """One drawn set of pairs through each matrix kernel, each bit-exact against the oracle, each kernel named:
    a mixed batch (int32 sw_dp_kernel), blocks of eight of one geometry with the grouped promise (packed sw_dp16_kernel) and the same
    pairs without it (int32), queries of 2 000 residues and more (one pair per wave, sw_dp64_kernel), tiles of 128 pairs on one target
    (`shared_kernel`).  ``flags``: score-only and binary-CIGAR calls of the mixed and grouped batches too; ``negate``: every call again
    with -o / -e (the entry normalises their signs)."""
    legs = [("mixed", "mixed", _blocks(rng, letters, mixed_geoms, 1), "sw_dp_kernel", 0),
            ("grouped", "grouped", _blocks(rng, letters, geoms, 8), "sw_dp16_kernel", 1),
            ("long", "mixed", _blocks(rng, letters, long_geoms, 1), "sw_dp64_kernel", 0),
            ("shared", "shared", _blocks(rng, letters, geoms, 128, last=77), shared_kernel, None)]
    legs.insert(2, ("grouped pairs, no promise", "mixed", legs[1][2], "sw_dp_kernel", 0))
    for name, kind, (ts, qs), kernel, packed in legs:
        assert len({(len(t), len(q)) for t, q in zip(ts, qs)}) > 1   # (one geometry would make the batch uniform: the packed kernel)
        if kind != "mixed":
            assert _dp16_range_ok(max(map(len, ts)), max(map(len, qs)), int(mat.max()), int(mat.min()), abs(o), abs(e))
        stride = _stride(ts, qs)
        ref = _oracle_unique(ts, qs, code, mat, o, e, strategy, stride)
        what = (name, strategy, o, e)
        for sign in ((1, -1) if negate else (1,)):
            b, k = _run(a, kind, ts, qs, code, mat, sign * o, sign * e, strategy, stride)
            assert k == kernel and (packed is None or a.timing().packed16 == packed), (what, sign, k)
            _assert_exact(b, ref, (what, sign))
        if flags and kind != "shared":
            b, k = _run(a, kind, ts, qs, code, mat, o, e, strategy, stride, score_only=True)
            assert k == kernel, (what, "score only", k)
            assert (b.scores.cpu().numpy() == ref[1]).all() and int((b.status != 0).sum()) == 0, (what, "score only")
            if packed:   # the packed kernel skips flags and walk ...
                assert int(b.offsets.abs().sum()) == 0 and int(b.cigar_len.abs().sum()) == 0, (what, "score only")
            else:        # ... every other kernel runs the full path
                _assert_exact(b, ref, (what, "score only"))
            b, k = _run(a, kind, ts, qs, code, mat, o, e, strategy, stride, binary_cigar=True)
            assert k == kernel and int((b.status != 0).sum()) == 0, (what, "binary", k)
            assert (b.scores.cpu().numpy() == ref[1]).all() and (b.offsets.cpu().numpy() == ref[0]).all(), (what, "binary")
            _assert_binary_cigar(b, ref[2], (what, "binary"))


_ALL_BYTES = np.arange(256, dtype=np.uint8)


@pytest.mark.gpu
def test_asymmetric_full_range_matrix_every_kernel():
    """A random asymmetric matrix over all of int8 (row = target code) and a code table over all 32 codes, sequences of arbitrary bytes,
    through every matrix kernel; gap penalties with o + e = 128 keep every S + o + e inside the shared-target kernel's byte table
    (0 .. 255, both ends reached), o == e and e == 0 among them; score-only and binary CIGARs on the int32 and grouped kernels; the same
    calls with negative gap penalties."""
    rng = np.random.default_rng(31)
    a = sw.MicrosoftSmithWaterman(0)
    geoms = [(1, 1), (5, 3), (31, 4), (33, 17), (64, 150), (65, 160), (200, 64), (190, 159)]   # (inside the 16-bit guard at 64 / 64)
    for strategy, (o, e) in zip(ol.STRATEGIES, [(127, 1), (64, 64), (128, 0), (100, 28)]):
        mat, code = _asymmetric_matrix(rng), _all_codes(rng)
        for c in range(32):   # a positive diagonal: fragments of the target align over long paths
            mat[c, c] = int(rng.integers(40, 128))
        assert int(mat.min()) + o + e == 0 and int(mat.max()) + o + e == 255
        mixed = [(int(rng.integers(1, 700)), int(rng.integers(1, 400))) for _ in range(48)]
        _every_matrix_path(a, rng, code, mat, _ALL_BYTES, o, e, strategy, mixed, geoms, [(2300, 2001), (700, 2047), (65, 2003)],
                           flags=True, negate=True)
    a.close()


@pytest.mark.gpu
def test_hot_padding_rows_every_kernel():
    """Row 0 and column 0 of the matrix at +127, then at -128, under a code table that maps NO byte to code 0 -- the code the kernels
    pad rows and columns outside a pair with: a padded cell that reached a maximum or a decision would change a result.  Query lengths
    that are no multiple of 2, 8, 16 or 32; targets that end a row before, on and a row after the ends of 16-, 32- and 64-row strips."""
    rng = np.random.default_rng(37)
    a = sw.MicrosoftSmithWaterman(0)
    tls, qls = [31, 32, 33, 63, 64, 65, 95, 97], [1, 3, 7, 13, 33, 45, 99, 301]
    geoms = [(31, 1), (32, 3), (33, 7), (63, 13), (64, 33), (65, 45), (95, 99), (97, 301), (33, 301), (65, 1)]
    mixed = [(tl, ql) for tl in tls for ql in qls]
    long_geoms = [(2047, 2001), (97, 2003), (65, 2005)]
    for hot, (o, e) in ((127, (11, 1)), (-128, (127, 1))):
        code = (1 + rng.integers(0, 31, 256)).astype(np.uint8)
        for strategy in ol.STRATEGIES:
            mat = _asymmetric_matrix(rng, -6, 11)
            mat[0, :] = hot
            mat[:, 0] = hot
            _every_matrix_path(a, rng, code, mat, _ALL_BYTES, o, e, strategy, mixed, geoms, long_geoms)
    a.close()


@pytest.mark.gpu
def test_ties_every_kernel():
    """Two letters, matrix entries in {-1, +1} and in {0, 2}, small gap penalties: maxima tie everywhere, the ScoreMax tie rules decide.
    Gap penalties 0 / 0 put an entry S + o + e below zero: the shared-target call falls back to the grouped promise."""
    rng = np.random.default_rng(41)
    a = sw.MicrosoftSmithWaterman(0)
    code = np.zeros(256, np.uint8)
    code[ord("A")], code[ord("B")] = 5, 9
    letters = np.frombuffer(b"AB", np.uint8)
    geoms = [(1, 1), (7, 5), (31, 9), (33, 33), (64, 20), (97, 130), (200, 61)]
    for values, gaps in (((-1, 1), [(1, 1), (2, 1), (0, 0)]), ((0, 2), [(1, 1), (2, 1)])):
        for o, e in gaps:
            for strategy in ol.STRATEGIES:
                mat = rng.choice(np.array(values, np.int8), (32, 32))
                mixed = [(int(rng.integers(1, 300)), int(rng.integers(1, 200))) for _ in range(48)]
                kernel = "sw_dp16_lane_matrix_kernel" if values[0] + o + e >= 0 else "sw_dp16_kernel"
                _every_matrix_path(a, rng, code, mat, letters, o, e, strategy, mixed, geoms, [(301, 2001), (64, 2003)], shared_kernel=kernel)
    a.close()


@pytest.mark.gpu
def test_16bit_guard_edges_grouped_and_shared_target():
    """The largest geometry the 16-bit guard admits, and one more, through the grouped packed kernel and the shared-target kernel: W-W
    scores 127 (the steepest rise: at 502 x 502 the best score is 63 754, far outside int16 -- only the kernels' baseline keeps it
    representable), W against C -128 (the steepest fall), o = 127, e = 1, every strategy (INDEL: the lowest borders).  At n the 16-bit
    kernel runs and is exact, at n + 1 the int32 kernel does.  Then a rectangle, tl = 3 ql, where min(tl, ql) is what binds."""
    rng = np.random.default_rng(43)
    a = sw.MicrosoftSmithWaterman(0)
    code, mat = protein.blosum62()
    mat = mat.copy()
    W, Cy = protein.AMINO.index("W"), protein.AMINO.index("C")
    mat[W, W], mat[W, Cy], mat[Cy, W] = 127, -128, -90
    o, e, smax, smin = 127, 1, 127, -128
    assert int(mat.max()) == smax and int(mat.min()) == smin and 0 <= smin + o + e and smax + o + e <= 255
    n = max(k for k in range(1, 2000) if _dp16_range_ok(k, k, smax, smin, o, e))
    assert n == 502 and not _dp16_range_ok(n + 1, n + 1, smax, smin, o, e)
    r = max(k for k in range(1, 2000) if _dp16_range_ok(3 * k, k, smax, smin, o, e))
    homo = lambda ch, k: np.full(k, ord(ch), np.uint8)

    def diverged(t, k):
        q = t[:k].copy()
        mut = rng.random(k) < 0.25
        q[mut] = protein.random_proteins(rng, 1, int(mut.sum()))[0]
        return np.insert(np.delete(q, k // 3), 2 * k // 3, ord("W"))

    for tl, ql, fits in ((n, n, True), (n + 1, n + 1, False), (3 * r, r, True), (3 * r + 3, r + 1, False)):
        assert _dp16_range_ok(tl, ql, smax, smin, o, e) == fits
        prot = protein.random_proteins(rng, 1, tl)[0]
        prot[rng.random(tl) < 0.3] = ord("W")
        # blocks of eight (grouped): rise, fall, the other fall, a diverged pair, a W-rich pair, C against C, random
        tq = [(homo("W", tl), homo("W", ql)), (homo("W", tl), homo("C", ql)), (homo("C", tl), homo("W", ql)), (prot, diverged(prot, ql)),
              (homo("W", tl), diverged(prot, ql)), (homo("C", tl), homo("C", ql)), (prot, protein.random_proteins(rng, 1, ql)[0]),
              (prot, homo("W", ql))]
        gts, gqs = [t.tobytes() for t, _ in tq], [q.tobytes() for _, q in tq]
        # tiles of 128 (shared target): the W homopolymer, then the W-rich protein, against the queries above
        sts = [tq[0][0].tobytes()] * 128 + [prot.tobytes()] * 128
        sqs = [tq[k % 4][1].tobytes() if k < 128 else [diverged(prot, ql).tobytes(), gqs[7], gqs[6], gqs[1]][k % 4] for k in range(256)]
        for strategy in ol.STRATEGIES:
            for kind, ts, qs in (("grouped", gts, gqs), ("shared", sts, sqs)):
                stride = _stride(ts, qs)
                ref = _oracle_unique(ts, qs, code, mat, o, e, strategy, stride)
                if kind == "grouped" and tl == n:
                    assert int(ref[1][0][2]) == 127 * n   # (the W homopolymers' best score)
                b, k = _run(a, kind, ts, qs, code, mat, o, e, strategy, stride)
                kernel = ("sw_dp16_kernel" if kind == "grouped" else "sw_dp16_lane_matrix_kernel") if fits else "sw_dp_kernel"
                assert k == kernel and (kind == "shared" or a.timing().packed16 == int(fits)), (tl, ql, kind, strategy, k)
                _assert_exact(b, ref, (tl, ql, kind, strategy))
    a.close()


@pytest.mark.gpu
def test_shared_target_byte_table_edges():
    """S + o + e reaching 0 and 255 at once (-128 / 127 with o = 127, e = 1) runs the shared-target kernel, exactly; one step past
    either end (o = 126: -1; o = 128: 256; o = 127, e = 0: -1) the flag is read as the grouped promise, exactly."""
    rng = np.random.default_rng(47)
    a = sw.MicrosoftSmithWaterman(0)
    geoms = [(31, 7), (33, 45), (65, 99), (97, 13)]
    for strategy in ol.STRATEGIES:
        mat, code = _asymmetric_matrix(rng), _all_codes(rng)
        ts, qs = _blocks(rng, _ALL_BYTES, geoms, 128, last=51)
        stride = _stride(ts, qs)
        for o, e, kernel in ((127, 1, "sw_dp16_lane_matrix_kernel"), (126, 1, "sw_dp16_kernel"), (128, 1, "sw_dp16_kernel"), (127, 0, "sw_dp16_kernel")):
            b, k = _run(a, "shared", ts, qs, code, mat, o, e, strategy, stride)
            assert k == kernel, (o, e, strategy, k)
            _assert_exact(b, _oracle_unique(ts, qs, code, mat, o, e, strategy, stride), (o, e, strategy))
    a.close()


@pytest.mark.gpu
def test_shared_target_without_status_array_computes_every_pair():
    """MGL_SW_FLAG_SHARED_TARGET with no status array: the layout of a broken promise (a pair one residue further into the targets,
    a pair with a shorter query) cannot be reported, so the library runs the batch without the promise -- every pair equals the
    oracle, none keeps the poisoned values it had before the call."""
    import torch

    rng = np.random.default_rng(53)
    code, mat = protein.blosum62()
    a = sw.MicrosoftSmithWaterman(0)
    ts, qs = _tiles(rng, [(64, 50)] * 6, 128)
    b = _shared_batch(ts, qs, torch.device("cuda", 0), 512)
    b.t_off[2 * 128 + 77] += 1
    b.q_len[4 * 128 + 5] -= 1
    ts[2 * 128 + 77] = ts[2 * 128 + 77][1:] + bytes([ts[3 * 128][0]])   # (the targets lie back to back: the next tile's first residue)
    qs[4 * 128 + 5] = qs[4 * 128 + 5][:-1]
    for x in (b.offsets, b.scores, b.cigar_len, b.status):
        x.fill_(-7)
    protein.run_matrix(b, a, code, mat, 11, 1, ol.SOFTCLIP, shared_target=True, null_status=True)
    torch.cuda.synchronize()
    off, sc, cg = oracle_matrix_batch(ts, qs, code, mat, 11, 1, ol.SOFTCLIP, 512)
    assert (b.scores.cpu().numpy() == sc).all() and (b.offsets.cpu().numpy() == off).all() and b.cigar_strings() == cg
    assert int((b.status != -7).sum()) == 0   # (no status array: nothing written there)
    assert a.fill_kernel_name(a.timing()) == "sw_dp_kernel"
    a.close()
