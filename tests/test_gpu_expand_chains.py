"""mgl_sw_expand_chains_batch_device on the GPU against tests/lines_textbook.py, bit for bit: the job count, job_start, the job records,
the per-job arrays, the jobs' anchors, the oriented buffer and the statuses, with canaries of 16 entries behind every output array and
behind d_jobs_out[job_capacity], and canary bytes in every byte of the oriented buffer that is not to be written -- around every read
in both halves.  Reads of 0 .. 16 chains, keep_secondary 0 and 1, max_chains 1, 4 and 16, chains of 1 .. 4 096 anchors, read lengths
and offsets at every seam of the 16-byte copy, reads with jobs on one strand or both, non-ACGT bytes, every refusal at the front, in
the middle and at the end, the capacity rule, an empty batch, the optional arrays left out, the empty tail fed to the stages behind,
and the records straight from the rank stage on one stream."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lines_cases as lc  # noqa: E402
import lines_textbook as ltb  # noqa: E402
import rank_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu

PAD = lc.PAD
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
TORCH = {np.int64: torch.int64, np.int32: torch.int32, np.uint8: torch.uint8}


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
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=dt))).to(DEV)


def _inputs(b, rank_status=True):
    n, mc = len(b["q_len"]), b["max_chains"]
    rec = np.full((n, mc, 12), lc.CANARY, np.int32)  # (records at or beyond n_chains are not the rank stage's: they must not be read)
    for p, recs in enumerate(b["records"]):
        for c, r in enumerate(recs[:mc]):
            rec[p, c] = r
    return (_g(np.frombuffer(b["queries"], np.uint8), np.uint8), _g(b["q_start"], np.int64), _g(b["q_len"], np.int32),
            _g(b["rank_status"], np.int32) if rank_status else None, _g(b["n_chains"], np.int32), _g(rec, np.int32), _g(b["ranked_start"], np.int64),
            _g(b["ranked_t"], np.int32), _g(b["ranked_q"], np.int32), _g(b["ranked_len"], np.int32))


def _check(aligner, b, keep_secondary, job_capacity, status=True, rank_status=True):
    """one call into arrays of canaries; everything against the textbook"""
    e, want = lc.expand_expected(b, keep_secondary, job_capacity, rank_status)
    sizes = lc.expand_sizes(b, job_capacity)
    full = [torch.full((s + (8 * PAD if k == 2 else PAD),), lc.CANARY_BYTE if dt == np.uint8 else lc.CANARY, dtype=TORCH[dt], device=DEV)
            for k, (s, dt) in enumerate(zip(sizes, lc.expand_dtypes()))]
    out = [x[:s] for x, s in zip(full, sizes)]
    out[2] = out[2].view(job_capacity, 8)
    if not status:
        out[10] = None
        want[10][:] = lc.CANARY
    aligner.expand_chains_device(*_inputs(b, rank_status), b["max_chains"], keep_secondary, job_capacity, out=tuple(out))
    torch.cuda.synchronize()
    for name, x, y in zip(lc.EXPAND_NAMES, full, want):
        x = x.cpu().numpy()
        bad = np.flatnonzero(x != y)
        assert bad.size == 0, (name, keep_secondary, job_capacity, bad[:8], x[bad[:8]], y[bad[:8]])
    return e, out


def _reads(rng, counts, lengths, sizes=(1, 2, 3, 5), status=None):
    return [(lc.random_read(rng, lengths[p % len(lengths)]), 0 if status is None else status[p], lc.random_records(rng, m, sizes)) for p, m in enumerate(counts)]


@pytest.mark.parametrize("max_chains", [1, 4, 16])
@pytest.mark.parametrize("keep_secondary", [0, 1])
def test_reads_of_every_chain_count(aligner, max_chains, keep_secondary):
    rng = np.random.default_rng(10 * max_chains + keep_secondary)
    counts = [c for c in (0, 1, 2, 15, 16, 3, 0, 16, 1) if c <= max_chains]
    b = lc.expand_batch(_reads(rng, counts, [40, 17, 300, 1]), max_chains, gap=3, first=5)
    e, _ = _check(aligner, b, keep_secondary, len(counts) * max_chains)
    assert e.n_jobs > 0 and (keep_secondary == 0 or e.n_jobs == sum(counts))
    _check(aligner, b, keep_secondary, len(counts) * max_chains, status=False, rank_status=False)


def test_chains_at_the_wave_seams(aligner):
    rng = np.random.default_rng(3)
    reads = [(lc.random_read(rng, 50), 0, [lc.ranked(500 - c, c & 1, k, c if c != 2 else 0) for c, k in enumerate(ks)])
             for ks in ([1, 63, 64], [65, 4096, 1, 64], [4096], [64, 64, 65, 63])]
    b = lc.expand_batch(reads, 4)
    for keep in (0, 1):
        e, _ = _check(aligner, b, keep, 16)
        assert e.n_jobs == (12 if keep else 9)


@pytest.mark.parametrize("first", [0, 5, 11])
def test_read_lengths_and_offsets_at_the_seams_of_the_copy(aligner, first):
    """every length at every residue mod 16 of the read's place, a byte apart at least, with jobs on both strands, on strand 0 only and
    on strand 1 only; `first` shifts the two halves of the oriented buffer, which lie query_bytes apart, against each other"""
    rng = np.random.default_rng(first)
    lengths = [1, 15, 16, 17, 31, 32, 33, 255, 256, 257]
    reads, residues = [], []
    for r in range(16):
        for k, n in enumerate(lengths + ([10007] if r == first else [])):
            strands = ([0, 1], [0], [1])[(k + r) % 3]
            reads.append((lc.random_read(rng, n), 0, [lc.ranked(100 - c, s, 1 + c, c) for c, s in enumerate(strands)]))
            residues.append(r)
    b = lc.expand_batch(reads, 2, gap=1, first=first, residues=residues)
    assert {(s % 16, n) for s, n in zip(b["q_start"], b["q_len"])} >= {(r, n) for r in range(16) for n in lengths}
    e, _ = _check(aligner, b, 1, 2 * len(reads))
    assert e.n_jobs == sum(len(r[2]) for r in reads)


def test_every_refusal_at_the_front_in_the_middle_and_at_the_end(aligner):
    rng = np.random.default_rng(5)

    def batch():
        return lc.expand_batch(_reads(rng, [3, 2, 4, 1, 3, 2, 4], [33, 70]), 4, gap=2, first=1)

    def edits(b, p):
        yield "q_len 0", lambda: b["q_len"].__setitem__(p, 0)
        yield "q_start < 0", lambda: b["q_start"].__setitem__(p, -1)
        yield "leaves the buffer", lambda: b["q_start"].__setitem__(p, b["query_bytes"] - b["q_len"][p] + 1)
        yield "n_chains < 0", lambda: b["n_chains"].__setitem__(p, -1)
        yield "n_chains > max_chains", lambda: (b["n_chains"].__setitem__(p, 5), b["records"].__setitem__(p, b["records"][p] + [lc.ranked(1, 0, 1, 0)] * 5))
        yield "strand 2", lambda: b["records"].__setitem__(p, [b["records"][p][0]._replace(strand=2)] + b["records"][p][1:])
        yield "n_anchors 0", lambda: b["records"].__setitem__(p, b["records"][p][:-1] + [b["records"][p][-1]._replace(n_anchors=0)])
        yield "the range is not the sum", lambda: b["records"].__setitem__(p, b["records"][p][:-1] + [b["records"][p][-1]._replace(n_anchors=b["records"][p][-1].n_anchors + 1)])
        yield "the rank stage's status", lambda: b["rank_status"].__setitem__(p, 5)

    for p in (0, 3, 6):
        for k in range(9):
            b = batch()
            name, edit = list(edits(b, p))[k]
            edit()
            e, _ = _check(aligner, b, 1, 28)
            assert [s != 0 for s in e.status] == [q == p for q in range(7)], (name, p, e.status)
            assert e.status[p] == (5 if k == 8 else ltb.BAD_ARG)
    # ranges: one that descends (the read behind it then holds more than its records say), one that leaves the total
    b = batch()
    b["ranked_start"][3] = b["ranked_start"][2] - 1
    e, _ = _check(aligner, b, 1, 28)
    assert e.status[2] == ltb.BAD_ARG and e.status[3] == ltb.BAD_ARG and sum(e.status) == 2
    b = batch()
    b["ranked_start"][7] += 1
    e, _ = _check(aligner, b, 0, 28)
    assert e.status == [0] * 6 + [ltb.BAD_ARG]


def test_the_capacity_rule(aligner):
    rng = np.random.default_rng(6)
    b = lc.expand_batch(_reads(rng, [3, 4, 2, 1, 4, 1], [20]), 4)
    total = 15
    e, _ = _check(aligner, b, 1, total)  # exactly fitting
    assert e.status == [0] * 6 and e.n_jobs == total
    e, _ = _check(aligner, b, 1, total - 1)  # one short: the last read goes
    assert e.status == [0] * 5 + [ltb.NOMEM]
    e, _ = _check(aligner, b, 1, 10)  # 3 + 4 + 2 + 1 fit, the read of 4 does not, and the later read of 1 has no room either
    assert e.status == [0, 0, 0, 0, ltb.NOMEM, ltb.NOMEM]
    e, _ = _check(aligner, b, 1, 8)  # 3 + 4 fit, 2 does not, the later, smaller read of 1 still does, 4 does not, 1 does not
    assert e.status == [0, 0, ltb.NOMEM, 0, ltb.NOMEM, ltb.NOMEM] and e.n_jobs == 8
    e, _ = _check(aligner, b, 1, 0)
    assert e.status == [ltb.NOMEM] * 6 and e.n_jobs == 0
    # more than one step of the scan, the cut inside the second
    big = lc.expand_batch(_reads(rng, [1 + (p % 3) for p in range(1500)], [3]), 4)
    e, _ = _check(aligner, big, 1, 2500)
    assert e.n_jobs == 2500 and ltb.NOMEM in e.status[1024:] and ltb.NOMEM not in e.status[:1024] and e.status[-1] == ltb.NOMEM
    assert any(s == 0 for s in e.status[e.status.index(ltb.NOMEM):])  # a later, smaller read still fits


def test_empty_batch(aligner):
    b = lc.expand_batch([], 4)
    e, _ = _check(aligner, b, 1, 0)
    assert e.n_jobs == 0
    _check(aligner, b, 1, 5)


def test_the_empty_tail_is_refused_by_the_stages_behind(aligner):
    rng = np.random.default_rng(8)
    b = lc.expand_batch([(lc.random_read(rng, 60), 0, [lc.ranked(90, 0, 2, 0), lc.ranked(80, 1, 1, 1)])], 4)
    b["ranked_t"], b["ranked_q"], b["ranked_len"] = [100, 130, 400], [5, 35, 10], [20, 20, 20]
    cap = 4
    e, out = _check(aligner, b, 1, cap)
    assert e.n_jobs == 2
    ref = _g(np.frombuffer(lc.random_read(rng, 1000), np.uint8), np.uint8)
    can = lambda n, dt=torch.int32: torch.full((n,), lc.CANARY, dtype=dt, device=DEV)  # noqa: E731
    window = (can(cap, torch.int64), can(cap), can(3), can(cap))
    aligner.locate_window_device(1000, out[4], out[5], out[6], out[7], out[8], 50, 400, out=window)
    aln = aligner.align_chain_device(ref, window[0], window[1], out[9], out[3], out[4], out[5], window[2], out[7], out[8], 400, 100, 100, 100, 16, -1,
                                     cigar_stride=64)
    torch.cuda.synchronize()
    wst, ast, ln = window[3].cpu().numpy(), aln[6].cpu().numpy(), aln[5].cpu().numpy()
    assert list(wst) == [0, 0, ltb.BAD_ARG, ltb.BAD_ARG] and list(ast[2:]) == [ltb.BAD_ARG] * 2 and list(ln[2:]) == [0, 0]
    assert (aln[0].cpu().numpy()[2:] == 0).all()


def test_straight_from_the_rank_stage_on_one_stream(aligner):
    """the hand cases of the rank stage: its records, anchors and statuses go in as it wrote them, nothing in between"""
    cases = [c for c in rc.HAND if c[1] == 2]
    rb = rc.batch([c[2] for c in cases], 2)
    params = (4096, 4, 40, 1, 128)
    strands, ql, start, ct, cq, cl, f, pred, st = rb
    n = len(ql) // 2
    rng = np.random.default_rng(2)
    lens = [int(ql[2 * p]) for p in range(n)]
    seqs = [lc.random_read(rng, max(x, 1)) for x in lens]
    q_start = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])[:-1]
    stream = torch.cuda.Stream(DEV)
    with torch.cuda.stream(stream):
        ins = (_g(ql, np.int32), _g(start, np.int64), _g(ct, np.int32), _g(cq, np.int32), _g(cl, np.int32), _g(f, np.int32), _g(pred, np.int32), _g(st, np.int32))
        queries = _g(np.frombuffer(b"".join(seqs), np.uint8), np.uint8)
        qs, qlen = _g(q_start, np.int64), _g(lens, np.int32)
        stream.synchronize()
        ranked = aligner.rank_chains_device(*ins, 2, *params, anchors=True)
        got = aligner.expand_chains_device(queries, qs, qlen, ranked[6], ranked[0], ranked[1], *ranked[2:6], 4, True, None)
        stream.synchronize()
    import rank_textbook as rtb

    nc, recs, rs, rt, rq, rl, rst = rtb.rank_batch(2, ql, start, ct, cq, cl, f, pred, st, *params)
    total = len(ct)
    pad = [0] * (total - len(rt))
    e = ltb.expand_chains(q_start, lens, len(b"".join(seqs)), rst, nc, recs, 4, rs, rt + pad, rq + pad, rl + pad, total, 1, 4 * n)
    assert e.n_jobs > 0
    host = [x.cpu().numpy() for x in got]
    assert host[0][0] == e.n_jobs and list(host[1]) == e.job_start and list(host[10]) == e.status
    assert host[2].tolist() == [list(j) for j in e.jobs] and list(host[3]) == e.job_q_start and list(host[4]) == e.job_q_len
    assert list(host[5]) == e.job_anchor_start
    k = len(e.job_anchor_t)
    assert list(host[6][:k]) == e.job_anchor_t and list(host[7][:k]) == e.job_anchor_q and list(host[8][:k]) == e.job_anchor_len
    want = ltb.oriented(b"".join(seqs), q_start, lens, len(b"".join(seqs)), e, before=bytes(host[9]))
    assert bytes(host[9]) == want
