"""mgl_sw_rank_chains_batch_device on the GPU against tests/rank_textbook.py, bit for bit: every output array of every read -- the chain
counts, the records, the anchor arrays, the statuses -- with canaries of 16 entries behind every array, behind each read's n_chains
records and from d_ranked_start_out[n] on.  Rows at the ballot, sort and LDS seams in both forms of the kernel, the hand cases of
tests/rank_cases.py at max_chains 1, 2 and 16, more kept chains than the list holds, chains of 1 and of N anchors, a mixed batch with
every refusal (again without the optional arrays, on one strand, and empty), and f / pred straight from the chain stage on one stream."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_dp_cases as dpc  # noqa: E402
import chain_dp_textbook as ctb  # noqa: E402
import rank_cases as rc  # noqa: E402
import rank_textbook as rtb  # noqa: E402

pytestmark = pytest.mark.gpu

PAD = 16
NAMES = ("n_chains", "records", "ranked_start", "ranked_t", "ranked_q", "ranked_len", "status")


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


def _canaries(b, max_chains):
    n, total = len(b[1]) // b[0], len(b[3])
    sizes = (n, n * max_chains * 12, n + 1, total, total, total, n)
    full = [torch.full((s + (PAD * 12 if k == 1 else PAD),), rc.CANARY, dtype=torch.int64 if k == 2 else torch.int32, device=torch.device("cuda", 0))
            for k, s in enumerate(sizes)]
    return sizes, full


def _inputs(b, row_status=True):
    strands, ql, start, ct, cq, cl, f, pred, st = b
    return (_g(ql, np.int32), _g(start, np.int64), _g(ct, np.int32), _g(cq, np.int32), _g(cl, np.int32), _g(f, np.int32), _g(pred, np.int32),
            _g(st, np.int32) if row_status else None)


def _check(aligner, b, params, anchors=True, status=True, row_status=True):
    """one call into arrays of canaries; everything against the textbook"""
    max_cand, max_chains = params[:2]
    n = len(b[1]) // b[0]
    sizes, full = _canaries(b, max_chains)
    out = [x[:s] for x, s in zip(full, sizes)]
    out[1] = out[1].view(n, max_chains, 12)
    if not anchors:
        out[2:6] = [None] * 4
    if not status:
        out[6] = None
    aligner.rank_chains_device(*_inputs(b, row_status), b[0], *params, out=tuple(out))
    torch.cuda.synchronize()
    want = list(rc.expected(b, params, PAD, row_status))
    for k in ([2, 3, 4, 5] if not anchors else []) + ([6] if not status else []):
        want[k][:] = rc.CANARY  # (nothing was handed in: nothing is written)
    for name, x, y in zip(NAMES, full, want):
        x = x.cpu().numpy()
        bad = np.flatnonzero(x != y)
        assert bad.size == 0, (name, params, bad[:8], x[bad[:8]], y[bad[:8]])
    return want


@pytest.fixture(scope="module")
def seam_rows():
    rng = np.random.default_rng(41)
    return [rc.forest_row(rng, n) for n in rc.SEAM_SIZES], rc.forest_row(rng, 8193)


@pytest.mark.parametrize("max_cand,max_chains", [(8192, 4), (4096, 16)])
def test_rows_at_the_ballot_sort_and_lds_seams(aligner, seam_rows, max_cand, max_chains):
    rows, above = seam_rows
    want = _check(aligner, rc.batch([[r] for r in rows] + [[above]], 1), (max_cand, max_chains, 20, 2, 128))
    refused = [n > max_cand for n in rc.SEAM_SIZES] + [True]
    assert (want[6][:17] == np.where(refused, rtb.UNSUPPORTED, 0)).all() and (want[0][3:17][~np.array(refused[3:])] >= 4).all()
    # two rows a read: a large row beside a small one, either way round
    pairs = [[rows[i], rows[len(rows) - 1 - i]] for i in range(len(rows))] + [[rows[5], above]]
    want = _check(aligner, rc.batch(pairs, 2), (max_cand, max_chains, 20, 2, 128))
    assert want[6][16] == rtb.UNSUPPORTED and (want[6][:16] == (rtb.UNSUPPORTED if max_cand == 4096 else 0)).sum() == (4 if max_cand == 4096 else 16)


@pytest.mark.parametrize("max_chains", [1, 2, 16])
def test_hand_cases(aligner, max_chains):
    for name, strands, rows, (min_score, min_cnt, mask_level), chains in rc.HAND:
        want = _check(aligner, rc.batch([rows], strands), (4096, max_chains, min_score, min_cnt, mask_level))
        assert want[0][0] == min(len(chains), max_chains), name
    for name, strands, rows, max_cand, status in rc.refusals():
        want = _check(aligner, rc.batch([rows], strands), (max_cand, max_chains, 40, 3, 128))
        assert want[6][0] == status, name
    # the reads of all hand cases of one strand in one batch, at one set of parameters
    _check(aligner, rc.batch([c[2] for c in rc.HAND if c[1] == 1], 1), (4096, max_chains, 10, 1, 128))
    _check(aligner, rc.batch([c[2] for c in rc.HAND if c[1] == 2], 2), (4096, max_chains, 40, 1, 128))


@pytest.mark.parametrize("max_chains", [1, 7, 16])
def test_more_kept_chains_than_the_list_holds(aligner, max_chains):
    """40 and 33 chains of one anchor, their scores in no order: insertion at every place of the list, and eviction"""
    reads = [[rc.singles_row(40), rc.singles_row(33)], [rc.singles_row(17), rc.singles_row(0)], [rc.singles_row(1), rc.singles_row(16)]]
    want = _check(aligner, rc.batch(reads, 2), (4096, max_chains, 40, 1, 256))
    assert want[0][:3].tolist() == [max_chains, min(17, max_chains), min(17, max_chains)]
    _check(aligner, rc.batch([[r[0]] for r in reads], 1), (64, max_chains, 45, 1, 1))


def test_chains_of_one_anchor_and_of_every_anchor(aligner):
    sizes = (1, 2, 64, 65, 257, 4096)
    want = _check(aligner, rc.batch([[rc.line_row(n)] for n in sizes] + [[rc.singles_row(5)]], 1), (4096, 4, 5, 1, 128))
    assert want[1].reshape(-1, 12)[::4, 2][:6].tolist() == list(sizes) and want[2][7] == sum(sizes) + 4  # K = N: the walk of N steps
    want = _check(aligner, rc.batch([[rc.line_row(8192), rc.line_row(3)]], 2), (8192, 2, 5, 1, 128))
    assert want[1][2] == 8192 and want[0][0] == 2


@pytest.mark.parametrize("strands", [2, 1])
def test_a_mixed_batch_with_every_refusal(aligner, strands):
    b = rc.mixed_batch(np.random.default_rng(43), strands)
    params = (150, 4, 20, 2, 128)
    want = _check(aligner, b, params)
    assert len(want[0]) - PAD == (39 if strands == 2 else 40) and set(want[6][:-PAD].tolist()) == {0, rtb.BAD_ARG, rtb.UNSUPPORTED}
    if strands == 2:  # again without the optional arrays: the poisoned rows are read now and refuse their reads
        bare = _check(aligner, b, params, anchors=False, status=False, row_status=False)
        assert (bare[0] != want[0]).sum() == 2
        _check(aligner, b, (150, 16, 1, 1, 1))


@pytest.mark.parametrize("strands", [1, 2])
def test_an_empty_batch(aligner, strands):
    want = _check(aligner, rc.batch([], strands), (4096, 4, 40, 3, 128))
    assert want[2][0] == 0
    _check(aligner, rc.batch([], strands), (4096, 4, 40, 3, 128), anchors=False, status=False, row_status=False)


def test_f_and_pred_straight_from_the_chain_stage(aligner):
    """chain_anchors_device(dp=True) and rank_chains_device on one stream of their own, nothing in between"""
    rng = np.random.default_rng(44)
    reads = [dpc.random_read(rng, int(rng.integers(0, 300)), spread=int(rng.choice((3, 40, 300)))) for _ in range(40)]
    reads[4] = (0, reads[4][1], reads[4][2])  # a row the chain stage refuses: its f and pred stay as they were
    t_lens, q_lens, start, ct, cq, cl = dpc.csr(reads)
    chain_params = (64, 200, 200, 50, 38, 3)
    cs, xt, xq, xl, score, f, pred, status = ctb.chain_batch(t_lens, q_lens, start, ct, cq, cl, 250, *chain_params)
    assert status[4] == ctb.BAD_ARG and ctb.UNSUPPORTED in status
    f, pred = [rc.POISON if x is None else x for x in f], [rc.POISON if x is None else x for x in pred]
    b = (2, q_lens, start, ct, cq, cl, f, pred, status)
    params = (250, 4, 1, 1, 128)
    sizes, full = _canaries(b, 4)
    out = [x[:s] for x, s in zip(full, sizes)]
    out[1] = out[1].view(20, 4, 12)
    total = len(ct)
    dp_out = (torch.empty(41, dtype=torch.int64, device="cuda"), *(torch.empty(total, dtype=torch.int32, device="cuda") for _ in range(3)),
              torch.empty(40, dtype=torch.int32, device="cuda"), torch.full((total,), rc.POISON, dtype=torch.int32, device="cuda"),
              torch.full((total,), rc.POISON, dtype=torch.int32, device="cuda"), torch.empty(40, dtype=torch.int32, device="cuda"))
    ins = _inputs(b)
    tl = _g(t_lens, np.int32)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain = aligner.chain_anchors_device(tl, ins[0], *ins[1:5], 250, chain_params[0], chain_params[1:3], *chain_params[3:], out=dp_out)
        aligner.rank_chains_device(ins[0], *ins[1:5], chain[5], chain[6], chain[7], 2, *params, out=tuple(out))
    torch.cuda.synchronize()
    assert (chain[5].cpu().numpy() == np.asarray(f)).all() and (chain[6].cpu().numpy() == np.asarray(pred)).all()
    for name, x, y in zip(NAMES, full, rc.expected(b, params, PAD)):
        x = x.cpu().numpy()
        bad = np.flatnonzero(x != y)
        assert bad.size == 0, (name, bad[:8], x[bad[:8]], y[bad[:8]])
    # a row's first chain is the chain stage's own
    rec, nc = full[1].cpu().numpy().reshape(-1, 12), full[0].cpu().numpy()
    got_score = chain[4].cpu().numpy()
    for p in range(20):
        if nc[p]:
            first = rec[4 * p]
            assert first[0] == got_score[2 * p + first[1]] == max(got_score[2 * p:2 * p + 2])


def test_rank_chains_over_lists(aligner):
    rng = np.random.default_rng(45)
    reads = [[rc.forest_row(rng, int(rng.integers(0, 150))), rc.dp_row(rng, int(rng.integers(0, 150)))] for _ in range(10)]
    reads[3][1] = (0, *reads[3][1][1:])  # a refused read
    rows = [r for rd in reads for r in rd]
    max_cand = max(len(r[1]) for r in rows)
    nc, recs, rs, rt, rq, rl, status = rc.textbook(rc.batch(reads, 2), (max_cand, 5, 20, 2, 128))
    args = ([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows], [r[4] for r in rows])
    chains, anchors, st = aligner.rank_chains(*args, strands=2, max_chains=5, min_score=20, min_cnt=2, return_anchors=True)
    assert [[tuple(c) for c in cs] for cs in chains] == [[tuple(r) for r in cs] for cs in recs] and st.tolist() == status and status[3] == rtb.BAD_ARG
    flat = list(zip(rt, rq, rl))
    assert [[a for chain in per for a in chain] for per in anchors] == [flat[rs[p]:rs[p + 1]] for p in range(10)] and sum(nc) > 20
    again, st2 = aligner.rank_chains(*args, strands=2, max_chains=5, min_score=20, min_cnt=2)
    assert again == chains and st2.tolist() == status
