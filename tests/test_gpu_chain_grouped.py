"""mgl_sw_chain_anchors_grouped_batch_device on the GPU: every output bit for bit tests/contig_textbook.py's chain_batch_grouped,
canaries of 16 entries behind every array.  Rows at every ring size, a group change at every position around the ring's seams, groups
that alternate, all -1, all equal (also against the entry without groups), pred in a workspace slot, refused and empty reads,
the optional arrays absent, an empty batch."""
import functools
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_dp_cases as cases  # noqa: E402
import contig_textbook as gtb  # noqa: E402
from mgl_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

PAD = 16
NAMES = ("chain_start", "chain_t", "chain_q", "chain_len", "score", "f", "pred", "status")
SIZES = (0, 1, 2, 63, 64, 65, 127, 128, 129, 4097)
SEAMS = tuple(range(60, 69)) + tuple(range(124, 133))
PARAMS = (64,) + cases.RING


@pytest.fixture(scope="module")
def aligner():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mgl_amd import smithwaterman as sw

    a = sw.MicrosoftSmithWaterman(0)
    assert a.load()
    yield a
    a.close()


def _g(x, dt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=dt))).to(torch.device("cuda", 0))


def _upload(batch):
    t_lens, q_lens, start, ct, cq, cl = batch
    return (_g(t_lens, np.int32), _g(q_lens, np.int32), _g(start, np.int64), _g(ct, np.int32), _g(cq, np.int32), _g(cl, np.int32))


def _run(al, batch, groups, max_cand, params, optional=True):
    """one call into arrays that are CANARY everywhere and PAD entries longer than their capacity -> the whole arrays, as numpy;
    ``groups`` None: the entry without groups"""
    dev = torch.device("cuda", 0)
    n, total = len(batch[0]), len(batch[3])
    sizes = (n + 1, total, total, total, n, total, total, n)
    full = [torch.full((size + PAD,), cases.CANARY, dtype=torch.int64 if k == 0 else torch.int32, device=dev) for k, size in enumerate(sizes)]
    views = [None if not optional and k in (5, 6, 7) else x[:size] for k, (x, size) in enumerate(zip(full, sizes))]
    al.chain_anchors_device(*_upload(batch), max_cand, params[0], params[1:3], *params[3:], out=tuple(views),
                            group=None if groups is None else _g(groups, np.int32))
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in full]


def _expected(batch, groups, max_cand, params):
    t_lens, q_lens, start, ct, cq, cl = batch
    n, total = len(t_lens), len(ct)
    want = gtb.chain_batch_grouped(t_lens, q_lens, start, ct, cq, cl, groups, min(max_cand, total), *params)

    def arr(size, values, dtype=np.int32):
        a = np.full(size + PAD, cases.CANARY, dtype)
        for i, v in enumerate(values):
            if v is not None:
                a[i] = v
        return a
    return (arr(n + 1, want[0], np.int64), arr(total, want[1]), arr(total, want[2]), arr(total, want[3]), arr(n, want[4]), arr(total, want[5]),
            arr(total, want[6]), arr(n, want[7]))


def _compare(got, want, skip=()):
    for k, name in enumerate(NAMES):
        if k not in skip:
            bad = np.flatnonzero(got[k] != want[k])
            assert bad.size == 0, (name, bad[:8], got[k][bad[:8]], want[k][bad[:8]])


@functools.lru_cache(maxsize=None)
def _ring_rows():
    """-> (the batch, per pattern its groups): every size; rows of 200 for the seams"""
    rng = np.random.default_rng(77)
    reads = [cases.random_read(rng, n) for n in SIZES] + [cases.random_read(rng, 200) for _ in SEAMS]
    batch = cases.csr(reads)
    lens = [len(r[2]) for r in reads]
    seam = [[0] * min(c, n) + [1] * max(n - c, 0) for n in lens[:len(SIZES)] for c in (n // 2,)] + [[0] * c + [1] * (200 - c) for c in SEAMS]
    flat = lambda rows: [g for r in rows for g in r]  # noqa: E731
    patterns = {
        "a change at every seam": flat(seam),
        "alternating": flat([[i % 2 for i in range(n)] for n in lens]),
        "three interleaved and -1": flat([[(i % 4) - 1 for i in range(n)] for n in lens]),
        "all -1": flat([[-1] * n for n in lens]),
        "all equal": flat([[5] * n for n in lens]),
        "random": rng.integers(-1, 3, sum(lens)).tolist(),
    }
    return batch, patterns


@pytest.mark.parametrize("pattern", ["a change at every seam", "alternating", "three interleaved and -1", "all -1", "all equal", "random"])
def test_ring_sizes_and_seams(aligner, pattern):
    batch, patterns = _ring_rows()
    groups = patterns[pattern]
    want = _expected(batch, groups, 4097, PARAMS)
    got = _run(aligner, batch, groups, 4097, PARAMS)
    _compare(got, want)
    n, total = len(batch[0]), len(batch[3])
    assert (got[7][:n] == 0).all()
    pred = got[6][:total]
    g = np.asarray(groups)
    linked = np.flatnonzero(pred >= 0)
    start = np.repeat(np.asarray(batch[2][:-1]), np.diff(batch[2]))
    assert (g[linked] == g[start[linked] + pred[linked]]).all() and (g[linked] >= 0).all()
    if pattern == "all -1":
        assert linked.size == 0 and (got[5][:total] == np.asarray(batch[5])).all() and (np.diff(got[0][:n + 1]) == (np.diff(batch[2]) > 0)).all()
    elif pattern == "all equal":  # the entry without groups, bit for bit
        _compare(got, _run(aligner, batch, None, 4097, PARAMS))
        assert linked.size > total // 2
    elif pattern == "a change at every seam":
        assert linked.size > 100
    else:  # chains that pass over strangers
        hop = linked[start[linked] + pred[linked] < linked - 1]
        assert hop.size > 100 and (g[hop - 1] != g[hop]).any()
    # the optional arrays absent: the rest is the same, and nothing is written where they would have been
    got = _run(aligner, batch, groups, 4097, PARAMS, optional=False)
    _compare(got, want, skip=(5, 6, 7))
    assert all((got[k] == cases.CANARY).all() for k in (5, 6, 7))


def test_refused_and_empty_reads_other_parameters_and_an_empty_batch(aligner):
    batch = cases.mixed_batch(np.random.default_rng(5))
    n, total = len(batch[0]), len(batch[3])
    groups = np.random.default_rng(6).integers(-1, 3, total).tolist()
    want = _expected(batch, groups, 150, PARAMS)
    assert sorted(set(want[7][:n])) == [0, _lib.ERR_BAD_ARG, _lib.ERR_UNSUPPORTED] and want[7][0] == 0 and 0 < want[0][n] < total
    _compare(_run(aligner, batch, groups, 150, PARAMS), want)
    got = _run(aligner, batch, groups, 150, PARAMS, optional=False)
    _compare(got, want, skip=(5, 6, 7))
    assert all((got[k] == cases.CANARY).all() for k in (5, 6, 7))
    for max_cand, max_pred in ((129, 2), (1 << 30, 63), (0, 1)):
        params = (max_pred,) + cases.RING
        _compare(_run(aligner, batch, groups, max_cand, params), _expected(batch, groups, max_cand, params))
    empty = ([], [], [0], [], [], [])
    _compare(_run(aligner, empty, [], 10, PARAMS), _expected(empty, [], 10, PARAMS))
    no_cands = ([5, 7], [5, 7], [0, 0, 0], [], [], [])
    _compare(_run(aligner, no_cands, [], 10, PARAMS), _expected(no_cands, [], 10, PARAMS))


def test_pred_in_a_workspace_slot(aligner):
    """max_cand above 32 768: the pred bytes leave LDS.  The candidates behind the rows belong to no read."""
    rng = np.random.default_rng(9)
    reads = [cases.random_read(rng, 129), cases.random_read(rng, 0), cases.random_read(rng, 65)]
    t_lens, q_lens, start, ct, cq, cl = cases.csr(reads)
    filler = 40000 - len(ct)
    batch = (t_lens, q_lens, start, ct + [0] * filler, cq + [0] * filler, cl + [0] * filler)
    groups = [(i // 3) % 2 for i in range(len(ct))] + [0] * filler
    want = _expected(batch, groups, 1 << 20, PARAMS)
    got = _run(aligner, batch, groups, 1 << 20, PARAMS)
    _compare(got, want)
    assert (got[7][:3] == 0).all() and got[0][3] > 20
