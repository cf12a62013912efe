"""mgl_sw_chain_anchors_batch_device on the GPU: every output -- d_chain_start_out, the three chain arrays up to d_chain_start_out[n], the
scores, f, pred, the status -- bit for bit the textbook's (tests/chain_dp_textbook.py), canaries behind every array and in the chain
arrays from d_chain_start_out[n] on; and candidates -> chain -> alignment on one stream against the textbook's chain uploaded from the
host."""
import functools
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_dp_cases as cases  # noqa: E402
import chain_dp_textbook as tb  # noqa: E402
import extend_adaptive_cases as xcases  # noqa: E402
import seed_extend_textbook as stb  # noqa: E402
from mgl_amd import _lib, synth  # noqa: E402

pytestmark = pytest.mark.gpu

PAD = 16
NAMES = ("chain_start", "chain_t", "chain_q", "chain_len", "score", "f", "pred", "status")
GATK = (200, -150, 260, 11)


@pytest.fixture(scope="module")
def aligner():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mgl_amd import smithwaterman as sw

    a = sw.MicrosoftSmithWaterman(0)
    assert a.load()
    yield a
    a.close()


def _upload(batch):
    dev = torch.device("cuda", 0)
    g = lambda x, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=dt))).to(dev)  # noqa: E731
    t_lens, q_lens, start, ct, cq, cl = batch
    return (g(t_lens, np.int32), g(q_lens, np.int32), g(start, np.int64), g(ct, np.int32), g(cq, np.int32), g(cl, np.int32))


def _run(al, batch, max_cand, params, optional=True):
    """one call into arrays that are CANARY everywhere and PAD entries longer than their capacity -> the whole arrays, as numpy"""
    dev = torch.device("cuda", 0)
    n, total = len(batch[0]), len(batch[3])
    full = [torch.full((size + PAD,), cases.CANARY, dtype=dt, device=dev)
            for size, dt in ((n + 1, torch.int64), (total, torch.int32), (total, torch.int32), (total, torch.int32), (n, torch.int32), (total, torch.int32),
                             (total, torch.int32), (n, torch.int32))]
    sizes = (n + 1, total, total, total, n, total, total, n)
    views = [None if not optional and k in (5, 6, 7) else x[:size] for k, (x, size) in enumerate(zip(full, sizes))]
    al.chain_anchors_device(*_upload(batch), max_cand, params[0], params[1:3], *params[3:], out=tuple(views))
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in full]


def _compare(got, want, skip=()):
    for k, name in enumerate(NAMES):
        if k not in skip:
            bad = np.flatnonzero(got[k] != want[k])
            assert bad.size == 0, (name, bad[:8], got[k][bad[:8]], want[k][bad[:8]])


@pytest.mark.parametrize("max_pred", cases.RING_PREDS)
def test_ring_edges(aligner, max_pred):
    batch = cases.csr(cases.ring_reads(np.random.default_rng(100 + max_pred), max_pred))
    params = (max_pred,) + cases.RING
    got = _run(aligner, batch, 256, params)
    _compare(got, cases.expected(batch, 256, params, PAD))
    assert (got[7][:len(batch[0])] == 0).all()
    n = len(cases.RING_SIZES)
    k = np.diff(got[0][:len(batch[0]) + 1])
    assert k[0] == 0 and k[1] == 1 and k[n] == (3 if max_pred == 64 else 1) and k[n + 1] == 3 and k[n + 2] == 1  # the three spaced reads


def test_rule_edges_ilog2_steps_ties_overlaps_and_the_guards_edge(aligner):
    by_params = {}
    for name, params, read, pred in cases.RULE_CASES + cases.LOG_CASES:
        by_params.setdefault(params, []).append((read, pred))
    assert len(by_params) >= 6
    for params, reads in by_params.items():
        batch = cases.csr([r for r, _ in reads])
        got = _run(aligner, batch, 8, params)
        _compare(got, cases.expected(batch, 8, params, PAD))
        assert got[6][:len(batch[3])].tolist() == [x for _, pred in reads for x in pred]  # the hand values


@functools.lru_cache(maxsize=None)
def _mixed(filler=0):
    t_lens, q_lens, start, ct, cq, cl = cases.mixed_batch(np.random.default_rng(5))
    return t_lens, q_lens, start, ct + [0] * filler, cq + [0] * filler, cl + [0] * filler  # (filler: candidates that belong to no read)


MIXED_PARAMS = (64,) + cases.RING


def test_mixed_batch_statuses_prefix_sum_canaries_and_optional_arrays(aligner):
    batch = _mixed()
    want = cases.expected(batch, 150, MIXED_PARAMS, PAD)
    n = len(batch[0])
    assert sorted(set(want[7][:n])) == [0, _lib.ERR_BAD_ARG, _lib.ERR_UNSUPPORTED] and 0 < want[0][n] < len(batch[3])
    _compare(_run(aligner, batch, 150, MIXED_PARAMS), want)
    # the optional arrays NULL: the rest is the same, and nothing is written where they would have been
    got = _run(aligner, batch, 150, MIXED_PARAMS, optional=False)
    _compare(got, want, skip=(5, 6, 7))
    assert all((got[k] == cases.CANARY).all() for k in (5, 6, 7))
    # max_pred and max_cand at other values on the same batch
    for max_cand, max_pred in ((129, 2), (1 << 30, 63), (0, 64)):
        params = (max_pred,) + cases.RING
        _compare(_run(aligner, batch, max_cand, params), cases.expected(batch, max_cand, params, PAD))


def test_ranges_that_leave_the_candidates(aligner):
    reads = [cases.random_read(np.random.default_rng(k), 30) for k in range(3)]
    t_lens, q_lens, start, ct, cq, cl = cases.csr(reads)
    batch = (t_lens + [9, 9], q_lens + [9, 9], [-1] + start[1:] + [91, 91], ct, cq, cl)  # [-1, 30), [30, 60), [60, 90), [90, 91), [91, 91)
    want = cases.expected(batch, 64, MIXED_PARAMS, PAD)
    assert want[7][:5].tolist() == [1, 0, 0, 1, 1]
    _compare(_run(aligner, batch, 64, MIXED_PARAMS), want)


def test_pred_in_a_workspace_slot_fewer_slots_than_reads_and_nomem(aligner):
    from mgl_amd import smithwaterman as sw

    small = sw.MicrosoftSmithWaterman(0)
    try:
        small.set_workspace(1 << 20)
        # 200 000 candidates: max_cand above what LDS holds, so pred goes to a slot of 200 192 bytes; behind 800 256 bytes of staging
        # one MiB holds one slot: one wave works all reads off
        batch = _mixed(200000 - len(_mixed()[3]))
        want = cases.expected(batch, 1 << 20, MIXED_PARAMS, PAD)
        _compare(_run(small, batch, 1 << 20, MIXED_PARAMS), want)
        _compare(_run(aligner, batch, 1 << 20, MIXED_PARAMS), want)  # the default workspace: a slot per wave
        # 230 000: 920 256 bytes of staging leave less than the slot's 230 144
        batch = _mixed(230000 - len(_mixed()[3]))
        with pytest.raises(_lib.MglSwError) as e:
            _run(small, batch, 1 << 20, MIXED_PARAMS)
        assert e.value.status == _lib.ERR_NOMEM
        n, total = len(batch[0]), len(batch[3])
        dev = torch.device("cuda", 0)
        out = (torch.full((n + 1,), 7, dtype=torch.int64, device=dev),) + tuple(torch.full((k,), 7, dtype=torch.int32, device=dev) for k in (total, total, total, n, total, total, n))
        with pytest.raises(_lib.MglSwError):
            small.chain_anchors_device(*_upload(batch), 1 << 20, out=out)
        torch.cuda.synchronize()
        assert all(bool((x == 7).all()) for x in out)  # nothing was written
        _compare(_run(small, batch, 150, MIXED_PARAMS), cases.expected(batch, 150, MIXED_PARAMS, PAD))  # (pred in LDS: no slot needed)
    finally:
        small.close()


# ---- candidates -> chain -> alignment

def _pack(Ts, Qs):
    from mgl_amd.smithwaterman import _pack_pairs

    return _pack_pairs(Ts, Qs, torch.device("cuda", 0), None, False)


def _end_to_end(al, Ts, Qs, cands, band):
    """align_candidates_device on a stream of its own, and align_chain_device on the textbook's chains uploaded from the host -> both
    tuples of arrays, the chain stage's arrays, the textbook's chains"""
    n, packed, stride = _pack(Ts, Qs)
    batch = cases.csr([(len(T), len(Q), c) for T, Q, c in zip(Ts, Qs, cands)])
    max_cand = max(len(c) for c in cands)
    up = _upload(batch)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain, got = al.align_candidates_device(*packed[:6], *up[2:], *packed[6:], max_cand, band, -1, GATK, *cases.MINIMAP[:1], cases.MINIMAP[1:3],
                                                *cases.MINIMAP[3:], to_query_end=True, cigar_stride=stride, sides=True, gap_scores=True)
    torch.cuda.synchronize()  # the one synchronisation: nothing above waited for the device
    want_chain = [tb.chain_dp(len(T), len(Q), c, *cases.MINIMAP) for T, Q, c in zip(Ts, Qs, cands)]
    flat = [a for r in want_chain for a in r.chain]
    start = np.concatenate([[0], np.cumsum([len(r.chain) for r in want_chain])])
    g = lambda x, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=dt))).to(torch.device("cuda", 0))  # noqa: E731
    pad = len(batch[3]) - len(flat)  # (the arrays as long as the stage's: d_gap_score_out has one entry per anchor index)
    host = [g(start, np.int64)] + [g([a[c] for a in flat] + [0] * pad, np.int32) for c in range(3)]
    want = al.align_chain_device(*packed[:6], *host, *packed[6:], cases.MINIMAP[1], cases.MINIMAP[2], band, -1, GATK, to_query_end=True, cigar_stride=stride,
                                 sides=True, gap_scores=True)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in got], [x.cpu().numpy() for x in want], [x.cpu().numpy() for x in chain if x is not None], want_chain, stride


def _same(got, want, n):
    """every output array of align_chain_device equal; a CIGAR row up to its length (the entry writes no byte at or beyond it)"""
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape
        if k == 4:
            a, b = a.reshape(n, -1), b.reshape(n, -1)
            assert all((a[p, :got[5][p]] == b[p, :got[5][p]]).all() for p in range(n))
        else:
            assert (a == b).all(), k


def test_candidates_to_alignment_on_one_stream_equals_the_textbooks_chain_uploaded(aligner):
    rng = np.random.default_rng(2043)
    pairs = synth.chain_pairs(43, 16, length=2000)
    Ts, Qs = [p[0] for p in pairs], [p[1] for p in pairs]
    noisy = [synth.noisy_candidates(rng, len(T), len(Q), true, off=(300, 900)) for T, Q, true in pairs]
    got, want, chain, want_chain, _ = _end_to_end(aligner, Ts, Qs, [c for c, _ in noisy], 64)
    assert len(got) == len(want) == 7
    _same(got, want, len(pairs))
    assert (got[6] == 0).all() and (chain[-1] == 0).all()
    assert chain[0].tolist() == np.concatenate([[0], np.cumsum([len(r.chain) for r in want_chain])]).tolist()
    assert chain[4].tolist() == [r.score for r in want_chain]
    for (c, kind), r in zip(noisy, want_chain):
        assert len(r.chain) >= 8 and {x for x, k in zip(c, kind) if k >= synth.CAND_DECOY} and not {x for x, k in zip(c, kind) if k >= synth.CAND_DECOY} & set(r.chain)


def test_the_drift_pair_with_decoys_reaches_both_ends_with_ten_gap_elements(aligner):
    T, Q = xcases.drift_pairs()["deletions"]
    seeds = []
    for t in range(40, len(T) - 20, 100):  # exact 20-mers of the window, looked up in the query
        q = Q.find(T[t:t + 20])
        if q >= 0 and Q.find(T[t:t + 20], q + 1) < 0:
            seeds.append((t, q, 20))
    assert len(seeds) >= 20
    cands, kind = synth.noisy_candidates(np.random.default_rng(3), len(T), len(Q), seeds, off=(300, 900))
    assert kind.count(synth.CAND_DECOY) > 20 and kind.count(synth.CAND_REPEAT) > 5
    got, want, chain, want_chain, stride = _end_to_end(aligner, [T], [Q], [cands], 64)
    _same(got, want, 1)
    aln, cg, ln, st = got[0][0], got[4], got[5], got[6]
    assert st[0] == 0 and chain[-1][0] == 0
    assert (aln[1], aln[2], aln[3], aln[4]) == (0, len(T), 0, len(Q))
    els = stb.elements(cg[:ln[0]].tobytes().decode())
    assert [op for _, op in els if op != "M"] == ["D"] * 10 and all(n == 20 for n, op in els if op == "D")
