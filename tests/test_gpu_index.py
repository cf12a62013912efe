"""mgl_sw_index_build_device on the GPU: the exported entries bit for bit tests/index_textbook.py's build_index, and get_info.

The sizes the build works in (mgl_amd/csrc/sw_index.h, sw_seed.h): a workgroup sketches SEED_BLOCK = 1024 k-mer positions with the w - 1
positions to either side; the block counts are summed INDEX_SCAN_THREADS = 256 blocks a step; the bucket table is over the top
min(2k, 24, max(10, ceil(log2 M))) bits of a key."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import index_textbook as itb  # noqa: E402
import seed_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

SEED_BLOCK, SCAN = 1024, 256


@pytest.fixture(scope="module")
def aligner():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mgl_amd import smithwaterman as sw

    a = sw.MicrosoftSmithWaterman(0)
    assert a.load()
    yield a
    a.close()


def _bucket_bits(m, k):
    bits = 10
    while bits < 24 and (1 << bits) < m:
        bits += 1
    return min(bits, 2 * k)


def _same(index, R, k, w):
    """the index's export and info against the textbook -> M"""
    want = itb.build_index(R, k, w)
    keys, pos = index.export()
    torch.cuda.synchronize()
    keys, pos = keys.cpu().numpy(), pos.cpu().numpy()
    assert keys.dtype == np.uint32 and pos.dtype == np.int32 and len(keys) == len(pos) == len(want)
    bad = [i for i, (key, p) in enumerate(want) if keys[i] != key or pos[i] != p]
    assert not bad, (k, w, len(R), bad[:5])
    info = index.info
    assert (info.ref_len, info.entries, info.k, info.w) == (len(R), len(want), k, w)
    assert info.bytes == 8 * len(want) + 4 * ((1 << _bucket_bits(len(want), k)) + 1)
    return len(want)


def _check(al, R, k, w):
    with al.build_index(R, k, w) as index:
        return _same(index, R, k, w)


@pytest.mark.parametrize("k,w", [(15, 10), (4, 1), (16, 32), (11, 5)])
def test_reference_lengths_around_k_the_window_and_the_sketched_block(aligner, k, w):
    rng = np.random.default_rng(10 * k + w)
    long = cases.rand_seq(rng, 2 * SEED_BLOCK + k + 1)
    lengths = {k - 1, k, k + 1, k + w - 1, k + w}
    for m in (SEED_BLOCK, 2 * SEED_BLOCK):  # bases, and k-mer positions, around one block and two
        lengths |= {m + d for d in (-1, 0, 1)} | {m + k - 1 + d for d in (-1, 0, 1)}
    counts = [_check(aligner, long[:n], k, w) for n in sorted(lengths)]
    assert counts[0] == 0 and counts[1] == 1 and counts[-1] > SEED_BLOCK // (w + 1)


def test_a_reference_over_many_workgroups(aligner):
    R = cases.rand_seq(np.random.default_rng(70), 70001)
    assert _check(aligner, R, 15, 10) > 10000


@pytest.mark.parametrize("w", [1, 10, 32])
def test_a_stray_byte_at_and_beside_every_seam(aligner, w):
    k = 15
    rng = np.random.default_rng(w)
    for shift in (-k, -1, 0, 1):  # the N's k-mers end at, cross and begin at the seam
        R = bytearray(cases.rand_seq(rng, 3 * SEED_BLOCK + 100))
        for seam in (SEED_BLOCK, 2 * SEED_BLOCK, 3 * SEED_BLOCK):
            R[seam + shift] = ord("N")
        _check(aligner, bytes(R), k, w)
    R = bytearray(cases.rand_seq(rng, 2 * SEED_BLOCK + 100))
    R[SEED_BLOCK - 40:SEED_BLOCK + 40] = b"n" * 80  # windows without a valid position on either side of a seam
    _check(aligner, bytes(R), k, w)


def test_equal_keys_homopolymers_two_letter_repeats_and_the_first_and_last_bucket(aligner):
    assert _check(aligner, b"A" * 3000, 15, 10) == 3000 - 14 - 9  # equal hashes: each of the nk - w + 1 windows selects its first position
    assert _check(aligner, b"AC" * 1500, 15, 10) > 1000
    assert _check(aligner, b"AC" * 1500, 6, 4) > 1000
    for base, key in ((b"A", 0), (b"T", 0xFFFFFFFF)):  # k = 16: all 32 bits of the key
        with aligner.build_index(base * 2100, 16, 1) as index:
            assert _same(index, base * 2100, 16, 1) == 2085
            keys, pos = (x.cpu().numpy() for x in index.export())
            assert (keys == key).all() and (pos == np.arange(2085)).all()
    assert _check(aligner, b"A" * 1100 + b"N" + b"T" * 1100, 16, 5) > 400
    # k = 4: 8 key bits, fewer than the table's 10
    R = cases.rand_seq(np.random.default_rng(4), 5000)
    assert _check(aligner, R, 4, 1) == 4997 and _check(aligner, R, 4, 7) > 500


def test_an_index_without_entries(aligner):
    for R in (b"N" * 3000, b"ACGTNACGTN" * 200, b"acgt" * 600, b"ACG"):
        assert _check(aligner, R, 5, 3) == 0


def test_the_block_count_scan_across_its_step(aligner):
    # w = 1, k = 4: every valid position is an entry; SCAN blocks of SEED_BLOCK positions and a little of the next step
    R = bytearray(cases.rand_seq(np.random.default_rng(256), SCAN * SEED_BLOCK + 1500))
    R[SCAN * SEED_BLOCK - 2] = ord("N")
    assert _check(aligner, bytes(R), 4, 1) == len(R) - 3 - 4


def test_export_and_get_info_refuse_bad_arguments_on_both_sides_of_their_edge(aligner):
    import ctypes as C

    from mgl_amd import _lib

    L, dev, PAD, CANARY = _lib.lib(), torch.device("cuda", 0), 16, -777
    R = cases.rand_seq(np.random.default_rng(9), 2500)
    want = itb.build_index(R, 11, 5)
    m = len(want)
    stream = torch.cuda.current_stream(dev).cuda_stream
    with aligner.build_index(R, 11, 5) as index:
        assert m > 100 and index.info.entries == m
        arrays = lambda: [torch.full((m + 2 * PAD,), CANARY, dtype=torch.int32, device=dev) for _ in range(2)]  # noqa: E731
        keys, pos = arrays()
        export = lambda k, p, cap: L.mgl_sw_index_export_device(index.handle, stream, k, p, cap)  # noqa: E731
        # capacity M - 1 and 0, below 0, either output null, a null index: refused, and not one entry written
        for k, p, cap in ((keys.data_ptr(), pos.data_ptr(), m - 1), (keys.data_ptr(), pos.data_ptr(), 0), (keys.data_ptr(), pos.data_ptr(), -1),
                          (None, pos.data_ptr(), m), (keys.data_ptr(), None, m), (None, None, m + PAD)):
            assert export(k, p, cap) == _lib.ERR_BAD_ARG, cap
        assert L.mgl_sw_index_export_device(None, stream, keys.data_ptr(), pos.data_ptr(), m) == _lib.ERR_BAD_ARG
        torch.cuda.synchronize()
        assert bool((keys == CANARY).all()) and bool((pos == CANARY).all())
        # capacity M and M + 16: the M entries, and everything behind them untouched
        for cap in (m, m + PAD):
            keys, pos = arrays()
            assert export(keys.data_ptr(), pos.data_ptr(), cap) == _lib.OK
            torch.cuda.synchronize()
            k, p = keys.cpu().numpy(), pos.cpu().numpy()
            assert (k[:m].view(np.uint32) == [e[0] for e in want]).all() and (p[:m] == [e[1] for e in want]).all()
            assert (k[m:] == CANARY).all() and (p[m:] == CANARY).all()
        # get_info: a null output with a live handle, a null handle with an output
        info = _lib.IndexInfo()
        assert L.mgl_sw_index_get_info(index.handle, None) == _lib.ERR_BAD_ARG
        assert L.mgl_sw_index_get_info(None, C.byref(info)) == _lib.ERR_BAD_ARG
        assert L.mgl_sw_index_get_info(index.handle, C.byref(info)) == _lib.OK and (info.entries, info.ref_len, info.k, info.w) == (m, 2500, 11, 5)
    # an index without entries: any capacity from 0 on, nothing written
    with aligner.build_index(b"N" * 300, 11, 5) as empty:
        keys, pos = [torch.full((PAD,), CANARY, dtype=torch.int32, device=dev) for _ in range(2)]
        assert L.mgl_sw_index_export_device(empty.handle, stream, keys.data_ptr(), pos.data_ptr(), 0) == _lib.OK
        assert L.mgl_sw_index_export_device(empty.handle, stream, keys.data_ptr(), pos.data_ptr(), -1) == _lib.ERR_BAD_ARG
        torch.cuda.synchronize()
        assert bool((keys == CANARY).all()) and bool((pos == CANARY).all())


def test_two_indexes_alive_at_once_on_one_context(aligner):
    rng = np.random.default_rng(2)
    R1, R2 = cases.rand_seq(rng, 3000), cases.rand_seq(rng, 4100, b"ACG")
    one = aligner.build_index(R1, 15, 10)
    two = aligner.build_index(torch.from_numpy(np.frombuffer(R2, np.uint8).copy()).cuda(), 11, 5)
    try:
        assert _same(one, R1, 15, 10) != _same(two, R2, 11, 5)
        assert _same(one, R1, 15, 10) > 0
        assert one.ref.device.type == "cuda" and bytes(one.ref.cpu().numpy()) == R1
    finally:
        one.close()
        assert _same(two, R2, 11, 5) > 0
        two.close()
        two.close()  # (a closed index closes again harmlessly)
