"""mgl_sw_classify_alignments_batch_device on the GPU against tests/lines_textbook.py, bit for bit: every line record, n_lines,
primary_job and status, with canaries of 16 entries behind every output array and in every line record that is not to be written.
The CPU hand cases and the MAPQ table, reads of 0 .. 16 jobs side by side in the quarter waves, batches of 1 .. 65 reads, reads whose
jobs are all dead, poisoned alignment records under non-zero statuses, every per-read refusal, and an empty batch."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lines_cases as lc  # noqa: E402
import lines_textbook as ltb  # noqa: E402

pytestmark = pytest.mark.gpu

PAD = lc.PAD


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


def _check(aligner, batch, params, status=True):
    """one call into arrays of canaries; everything against the textbook"""
    job_start, jobs, aln, st, cap = batch
    n = len(job_start) - 1
    c, want = lc.classify_expected(batch, params)
    dev = torch.device("cuda", 0)
    full = [torch.full((s + p,), lc.CANARY, dtype=torch.int32, device=dev) for s, p in ((8 * cap, 8 * PAD), (n, PAD), (n, PAD), (n, PAD))]
    out = [full[0][:8 * cap].view(cap, 8), full[1][:n], full[2][:n], full[3][:n] if status else None]
    rec = np.zeros((cap, 8), np.int32)
    rec[:, 0], rec[:, 3], rec[:, 4] = [a[0] for a in aln], [a[1] for a in aln], [a[2] for a in aln]
    rec[:, [1, 2, 5, 6, 7]] = lc.CANARY  # (the fields the stage does not read)
    aligner.classify_alignments_device(_g(job_start, np.int64), _g(np.asarray(jobs, np.int32).reshape(cap, 8), np.int32), _g(rec, np.int32),
                                       _g(st, np.int32), *params, out=tuple(out))
    torch.cuda.synchronize()
    if not status:
        want[3][:] = lc.CANARY
    for name, x, y in zip(lc.CLASSIFY_NAMES, full, want):
        x = x.cpu().numpy()
        bad = np.flatnonzero(x != y)
        assert bad.size == 0, (name, params, bad[:8], x[bad[:8]], y[bad[:8]])
    return c


def test_hand_cases(aligner):
    for case in lc.HAND:
        c = _check(aligner, lc.hand_batch(case), case[2])
        assert [(l.order, l.flag, l.parent) for l in c.lines[:len(case[1])]] == case[3] and c.n_lines[0] == case[4] and c.primary_job[0] == case[5], case[0]
    # all of them in one batch: the parents are job indices of the batch
    _check(aligner, lc.classify_batch([case[1] for case in lc.HAND]), (1, 40, 128))


def test_mapq_table(aligner):
    for (s, c, k, n_sub, subsc, csub, match, min_score), want in lc.MAPQ:
        # a primary of score s over [0, 100) with n_sub secondaries inside it, the best of them first
        mine = [(ltb.Job(None, 0, 0, k, c, 0, 1000, 0), (s, 0, 100), 0)]
        mine += [(ltb.Job(None, 1 + x, 0, 5, csub if x == 0 else 1, 0, 1000, 0), (subsc if x == 0 else 1, 10, 60), 0) for x in range(n_sub)]
        got = _check(aligner, lc.classify_batch([mine]), (match, min_score, 128))
        assert got.lines[0].mapq == want and got.lines[0].n_sub == n_sub and got.lines[0].subsc == subsc, (s, c, k, n_sub)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65])
def test_quarter_wave_neighbours_of_every_size(aligner, n):
    rng = np.random.default_rng(100 + n)
    sizes = [(p * 5 + n) % 17 for p in range(n)] if n > 5 else [16, 0, 7, 1, 16][:n]
    for mask_level in (1, 128, 256):
        c = _check(aligner, lc.classify_batch(lc.random_classify_reads(rng, sizes)), (int(rng.choice([1, 2, 200])), 40, mask_level))
    assert sum(c.n_lines) > 0 or n < 3


def test_all_sizes_in_one_batch_and_all_dead_reads(aligner):
    rng = np.random.default_rng(7)
    reads = lc.random_classify_reads(rng, list(range(17)) + list(range(16, -1, -1)))
    dead = [[(j, a, 5) for j, a, _ in mine] for mine in lc.random_classify_reads(rng, [16, 3, 1])]
    c = _check(aligner, lc.classify_batch(reads[:20] + dead + reads[20:]), (200, 40, 128))
    assert c.n_lines[20:23] == [0, 0, 0] and c.primary_job[20:23] == [-1, -1, -1] and max(c.n_lines) >= 8
    _check(aligner, lc.classify_batch(reads), (200, 40, 128), status=False)


def test_every_refusal(aligner):
    rng = np.random.default_rng(9)
    reads = lc.random_classify_reads(rng, [4, 16, 2, 5, 3, 1])
    job_start, jobs, aln, st, cap = lc.classify_batch(reads, tail=20)
    base = list(job_start)
    for name, edit in (("descends", lambda s: s.__setitem__(2, s[1] - 1)), ("leaves the capacity", lambda s: s.__setitem__(6, cap + 1)),
                       ("negative", lambda s: s.__setitem__(0, -1)), ("longer than 16", lambda s: s.__setitem__(6, s[5] + 17))):
        start = list(base)
        edit(start)
        c = _check(aligner, (start, jobs, aln, st, cap), (1, 40, 128))
        assert ltb.BAD_ARG in c.status and 0 in c.status, name
    # a job of another read, in the first, a middle and the last read
    for p, j in ((0, 0), (1, 10), (5, base[6] - 1)):
        other = list(jobs)
        other[j] = other[j]._replace(read=other[j].read + 1)
        c = _check(aligner, (base, other, aln, st, cap), (1, 40, 128))
        assert [s != 0 for s in c.status] == [q == p for q in range(6)]


def test_empty_batch(aligner):
    _check(aligner, ([0], [ltb.EMPTY_JOB] * 4, [(0, 0, 0)] * 4, [1] * 4, 4), (1, 40, 128))
    _check(aligner, ([0], [], [], [], 0), (1, 40, 128))
