"""Reads in, EVERY ranked chain aligned and classified (map_reads_all_device), on a stream of its own with one synchronisation at the
end, on the repeat reads of DESIGN.md section 9k -- four of the eight with a second copy of their window in the reference, exact or at
one per cent -- and one short read of unrelated sequence.  The rank stage's tuple and the jobs against the textbook composition
(tests/rank_cases.py: repeat_mapped, then lines_textbook.expand_chains); the lines against lines_textbook.classify_alignments over the
alignments the device made; the alignment, CIGAR and describe record of every read's rank-0 job against map_reads_described_device's
on the same inputs, bit for bit; the second copy as a 0x100 line with an alignment of its own; keep_secondary = 0 gives a job per
own-parent chain only.  And against an index of contigs: contig_cases' reads and two split reads, every stage's tuple against the
composition of the CPU textbooks (tests/lines_cases.py), a supplementary line in another contig, rid / rname over lists, the SAM."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import index_cases as ic  # noqa: E402
import lines_textbook as ltb  # noqa: E402
import rank_cases as rc  # noqa: E402
import seed_cases as cases  # noqa: E402
from mgl_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

GATK = (200, -150, 260, 11)
UNRELATED = cases.rand_seq(np.random.default_rng(2), 120)  # (it shares no minimizer with the reference: the textbook finds no candidate)


@pytest.fixture(scope="module")
def aligner():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mgl_amd import smithwaterman as sw

    a = sw.MicrosoftSmithWaterman(0)
    assert a.load()
    yield a
    a.close()


@pytest.mark.parametrize("divergence", [0.0, 0.01])
def test_every_ranked_chain_is_aligned_and_classified(aligner, divergence):
    from mgl_amd.smithwaterman import _pack_pairs

    dev = torch.device("cuda", 0)
    ref, reads, truth, copy, _, (nc, recs, rs, rt, rq, rl, rank_status) = rc.repeat_mapped(divergence, (UNRELATED,))
    n = len(reads)
    _, packed, _ = _pack_pairs(reads, reads, dev, None, False)
    max_ql = packed[7]
    stride = 2 * max(ic.MAX_TL, max_ql)
    args = (*packed[3:6], ic.MAX_TL, max_ql, 64, -1, GATK)
    stages = dict(ic.SEEDING, **ic.CHAINING, **rc.RANKING, slack=ic.SLACK, strands=2, to_query_end=True, cigar_stride=stride)
    index = aligner.build_index(ref, rc.K, rc.W)
    try:
        base = aligner.map_reads_described_device(index, *args, **stages)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            got = aligner.map_reads_all_device(index, *args, **stages)
            own = aligner.map_reads_all_device(index, *args, keep_secondary=False, **stages)
        torch.cuda.synchronize()  # the one synchronisation: nothing above waited for the device
        seeds, chain, ranked, jobs, window, aln, described, lines = [[None if x is None else x.cpu().numpy() for x in t] for t in got]
        cap = 4 * n

        # ---- the rank stage: the textbook composition's records
        assert ranked[0].tolist() == nc == [2] * 4 + [1] * 4 + [0] and ranked[6].tolist() == rank_status
        for p in range(n):
            assert [tuple(int(v) for v in ranked[1][p, c]) for c in range(nc[p])] == [tuple(r) for r in recs[p]], p

        # ---- the jobs: expand_chains over the textbook's rank output
        q_start, q_len, qbytes = packed[4].cpu().numpy(), packed[5].cpu().numpy(), int(packed[3].numel())
        total = int(got[2][3].numel())
        pad = [0] * (total - len(rt))
        for keep, g in ((1, jobs), (0, [None if x is None else x.cpu().numpy() for x in own[3]])):
            e = ltb.expand_chains(q_start, q_len, qbytes, rank_status, nc, recs, 4, rs, rt + pad, rq + pad, rl + pad, total, keep, cap)
            assert e.n_jobs == (12 if keep else 8) and g[0][0] == e.n_jobs and g[1].tolist() == e.job_start and g[10].tolist() == e.status == [0] * n
            assert g[2].tolist() == [list(j) for j in e.jobs] and g[3].tolist() == e.job_q_start and g[4].tolist() == e.job_q_len
            k = len(e.job_anchor_t)
            assert g[5].tolist() == e.job_anchor_start and g[6][:k].tolist() == e.job_anchor_t and g[7][:k].tolist() == e.job_anchor_q
            assert g[8][:k].tolist() == e.job_anchor_len
            ori = ltb.oriented(packed[3].cpu().numpy().tobytes(), q_start, q_len, qbytes, e, before=g[9].tobytes())
            assert g[9].tobytes() == ori
        e = ltb.expand_chains(q_start, q_len, qbytes, rank_status, nc, recs, 4, rs, rt + pad, rq + pad, rl + pad, total, 1, cap)

        # ---- the stages behind run over all job_capacity jobs and refuse the empty ones
        assert window[3][:12].tolist() == [0] * 12 and aln[6][:12].tolist() == [0] * 12 and described[3][:12].tolist() == [0] * 12
        assert (window[3][12:] == _lib.ERR_BAD_ARG).all() and (aln[6][12:] == _lib.ERR_BAD_ARG).all() and (aln[5][12:] == 0).all()
        assert (described[3][12:] == _lib.ERR_BAD_ARG).all() and (described[0][12:] == 0).all()

        # ---- the lines: classify_alignments over the device's alignments
        triples = [(int(r[0]), int(r[3]), int(r[4])) for r in aln[0]]
        c = ltb.classify_alignments(e.job_start, e.jobs, cap, triples, aln[6].tolist(), GATK[0], 40, 128)
        assert lines[1].tolist() == c.n_lines == [2] * 4 + [1] * 4 + [0] and lines[2].tolist() == c.primary_job and lines[3].tolist() == c.status
        for j in range(12):
            assert tuple(lines[0][j]) == tuple(c.lines[j]), j
        assert c.primary_job[8] == -1  # the unrelated read: unmapped

        # ---- every read's rank-0 job is the alignment map_reads_described_device makes: record, window, CIGAR, describe record
        b_window, b_aln, b_desc = ([x.cpu().numpy() for x in base[3]], [None if x is None else x.cpu().numpy() for x in base[4]], [x.cpu().numpy() for x in base[6]])
        cg, bcg = aln[4].reshape(cap, stride), b_aln[4].reshape(n, stride)
        md, bmd = described[1].reshape(cap, stride), b_desc[1].reshape(n, stride)
        for p in range(8):
            j = e.job_start[p]
            assert c.primary_job[p] == j and e.jobs[j].rank == 0
            assert window[0][j] == b_window[0][p] and window[1][j] == b_window[1][p]
            assert (aln[0][j] == b_aln[0][p]).all() and aln[5][j] == b_aln[5][p] and (cg[j, :aln[5][j]] == bcg[p, :aln[5][j]]).all()
            assert (described[0][j] == b_desc[0][p]).all() and (md[j, :described[0][j, 6]] == bmd[p, :described[0][j, 6]]).all()

        # ---- the second copy: a secondary line with an alignment, a CIGAR and an NM of its own
        t_start = window[0]
        for p in range(4):
            j = e.job_start[p]
            first, second = c.lines[j], c.lines[j + 1]
            assert first.flag & ~0x10 == 0 and second.flag & ~0x10 == 0x100 and second.parent == j and first.n_sub == 1
            beg = t_start[j + 1] + aln[0][j + 1, 1]
            assert copy[p][0] - ic.SLACK <= beg < copy[p][0] + copy[p][1] and aln[5][j + 1] > 0 and described[0][j + 1, 0] > 1500
            if divergence == 0.0:
                assert aln[0][j + 1, 0] == aln[0][j, 0] and first.mapq == 0 and first.subsc == aln[0][j, 0]
            else:
                assert aln[0][j + 1, 0] < aln[0][j, 0] and 0 < first.mapq < 60 and described[0][j + 1, 1] > described[0][j, 1]
        assert all(c.lines[e.job_start[p]].mapq == 60 for p in range(4, 8))
        own_lines = [x.cpu().numpy() for x in own[7]]
        assert own_lines[1].tolist() == [1] * 8 + [0] and (own_lines[0][:8, 2] == 60).all()  # without the secondaries nothing lowers a MAPQ

        # ---- over lists: the same lines, and the SAM written from them rebuilds the reference under EVERY line
        from mgl_amd import formats

        listed = dict(stages)
        listed.pop("cigar_stride")
        res = aligner.map_reads_all(index, reads, 64, -1, GATK, max_tl=ic.MAX_TL, **listed)
        assert res.n_lines.tolist() == c.n_lines and [len(x) for x in res.lines] == c.n_lines
        for p in range(n):
            for k, ln in enumerate(res.lines[p]):
                j = [j for j in range(e.job_start[p], e.job_start[p + 1]) if c.lines[j].order == k][0]
                assert (ln.ref_beg, ln.ref_end, ln.score, ln.q_beg, ln.q_end) == (t_start[j] + aln[0][j, 1], t_start[j] + aln[0][j, 2], aln[0][j, 0], aln[0][j, 3], aln[0][j, 4])
                assert (ln.strand, ln.flag, ln.mapq, ln.status, ln.rid, ln.rname, ln.xcigar) == (e.jobs[j].strand, c.lines[j].flag, c.lines[j].mapq, 0, None, None, None)
                assert ln.cigar == cg[j, :aln[5][j]].tobytes().decode() and ln.nm == described[0][j, 1:4].sum() and ln.n_match == described[0][j, 0]
                assert ln.block_len == ln.n_match + ln.nm and ln.md == md[j, :described[0][j, 6]].tobytes()
                assert res.lines[p][ln.parent] is (ln if c.lines[j].parent == j else res.lines[p][c.lines[c.lines[j].parent].order])
        import tempfile

        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "all.sam")
            formats.write_sam_all(path, "ref", len(ref), ["r%d" % p for p in range(n)], reads, None, res)
            _, _, recs = formats.read_sam(path)
            assert len(recs) == sum(c.n_lines) + 1
            flat = [ln for lines_ in res.lines for ln in lines_]
            for rec, ln in zip([r for r in recs if r.pos >= 0], flat):
                assert formats.reference_under_read(rec)[0] == ref[ln.ref_beg:ln.ref_end] and rec.pos == ln.ref_beg
    finally:
        index.close()


def test_contigs_and_split_reads(aligner):
    """contig_cases' eleven reads and two split reads (tests/lines_cases.py: contig_reads) against the index of contigs, extension to the
    query's end off: every stage's tuple equals the composition of the CPU textbooks (lines_cases.contig_composed), which
    tests/test_lines_pipeline.py proves adversarial."""
    import contig_cases as cc
    import lines_cases as lc
    from mgl_amd import formats
    from mgl_amd.smithwaterman import _pack_pairs

    dev = torch.device("cuda", 0)
    reads, _ = lc.contig_reads()
    _, packed, _ = _pack_pairs(reads, reads, dev, None, False)
    # (the packed buffer has spare bytes behind the last read: the second half of the oriented buffer begins behind them)
    buffer, start, length, names, reads, tb, d = lc.contig_composed(False, query_pad=int(packed[3].numel()) - sum(len(r) for r in reads))
    contigs, _, _ = cc.pipeline_set()
    e, c, located = d["expanded"], d["classified"], d["located"]
    n, cap = len(reads), 4 * len(reads)
    max_ql = packed[7]
    stride = 2 * max(ic.MAX_TL, max_ql)
    args = (*packed[3:6], ic.MAX_TL, max_ql, cc.BAND, cc.ZDROP, cc.GATK)
    stages = dict(ic.SEEDING, **ic.CHAINING, **cc.RANKING, slack=ic.SLACK, strands=2, to_query_end=False, cigar_stride=stride)
    index = aligner.build_index_contigs(contigs, cc.K, cc.W)
    try:
        base = aligner.map_reads_described_device(index, *args, **stages)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            got = aligner.map_reads_all_device(index, *args, **stages)
        torch.cuda.synchronize()  # the one synchronisation
        seeds, chain, ranked, jobs, window, aln, described, lines = [[None if x is None else x.cpu().numpy() for x in t] for t in got]

        # ---- rank, jobs, windows, alignments, lines: the textbook composition's
        nc, recs, rs, rt, rq, rl, rank_status = tb[6]
        assert ranked[0].tolist() == nc and ranked[6].tolist() == rank_status
        for p in range(n):
            assert [tuple(int(v) for v in ranked[1][p, k]) for k in range(nc[p])] == [tuple(r) for r in recs[p]], p
        assert jobs[0][0] == e.n_jobs == 16 and jobs[1].tolist() == e.job_start and jobs[10].tolist() == e.status
        assert jobs[2].tolist() == [list(j) for j in e.jobs] and jobs[3].tolist() == e.job_q_start and jobs[4].tolist() == e.job_q_len
        k = len(e.job_anchor_t)
        assert jobs[5].tolist() == e.job_anchor_start and jobs[6][:k].tolist() == e.job_anchor_t and jobs[7][:k].tolist() == e.job_anchor_q
        assert jobs[8][:k].tolist() == e.job_anchor_len
        q_start, q_len, qbytes = packed[4].cpu().numpy(), packed[5].cpu().numpy(), int(packed[3].numel())
        assert jobs[9].tobytes() == ltb.oriented(packed[3].cpu().numpy().tobytes(), q_start, q_len, qbytes, e, before=jobs[9].tobytes())
        m = e.n_jobs
        assert window[0][:m].tolist() == located[0][:m] and window[1][:m].tolist() == located[1][:m] and window[3].tolist() == located[3]
        assert window[4][:m].tolist() == located[4][:m] and window[2][:k].tolist() == located[2][:k]
        assert aln[6].tolist() == d["aln_status"] and (aln[6][m:] == _lib.ERR_BAD_ARG).all() and (aln[6][:m] == 0).all()
        cg = aln[4].reshape(cap, stride)
        for j in range(m):
            assert tuple(aln[0][j]) == tuple(d["full"][j]), j
            assert cg[j, :aln[5][j]].tobytes().decode() == d["cigars"][j], j
        assert lines[1].tolist() == c.n_lines and lines[2].tolist() == c.primary_job and lines[3].tolist() == c.status == [0] * n
        for j in range(m):
            assert tuple(lines[0][j]) == tuple(c.lines[j]), j

        # ---- what the CPU proves of these inputs, on the device's own tuples
        line = lambda p, k: [j for j in range(e.job_start[p], e.job_start[p + 1]) if lines[0][j, 0] == k][0]  # noqa: E731
        first, second = line(cc.CHIMERA, 0), line(cc.CHIMERA, 1)  # a supplementary line in the other contig
        assert lines[0][first, 1] == 0 and lines[0][second, 1] == 0x800 and {int(window[4][first]), int(window[4][second])} == {0, 1}
        first, second = line(0, 0), line(0, 1)  # the window two contigs hold: a secondary of equal score, mapq 0
        assert lines[0][second, 1] == 0x100 and lines[0][first, 2] == 0 and aln[0][first, 0] == aln[0][second, 0] and window[4][second] == 3
        assert sorted(int(jobs[2][line(n - 1, k), 2]) for k in (0, 1)) == [0, 1]  # the inverted split read: a job on each strand
        assert lines[1][cc.UNRELATED_AT] == 0 and lines[2][cc.UNRELATED_AT] == -1

        # ---- the primary line of every non-split read is map_reads_described_device's alignment on the same inputs
        b_window, b_aln, b_desc = [x.cpu().numpy() for x in base[3]], [None if x is None else x.cpu().numpy() for x in base[4]], [x.cpu().numpy() for x in base[6]]
        bcg = b_aln[4].reshape(n, stride)
        for p in range(n - 2):
            if p == cc.UNRELATED_AT:
                continue
            j = int(lines[2][p])
            assert jobs[2][j, 1] == 0 and window[0][j] == b_window[0][p] and window[4][j] == b_window[4][p]
            assert (aln[0][j] == b_aln[0][p]).all() and aln[5][j] == b_aln[5][p] and (cg[j, :aln[5][j]] == bcg[p, :aln[5][j]]).all()
            assert (described[0][j] == b_desc[0][p]).all()

        # ---- over lists: rid, rname and positions from the contig's start; the SAM rebuilds each contig under every line
        listed = dict(stages)
        listed.pop("cigar_stride")
        res = aligner.map_reads_all(index, reads, cc.BAND, cc.ZDROP, cc.GATK, max_tl=ic.MAX_TL, **listed)
        assert res.n_lines.tolist() == c.n_lines
        for p in range(n):
            for k, ln in enumerate(res.lines[p]):
                j = line(p, k)
                r = located[4][j]
                assert (ln.rid, ln.rname, ln.flag, ln.mapq, ln.score) == (r, names[r], c.lines[j].flag, c.lines[j].mapq, d["full"][j].score)
                assert (ln.ref_beg, ln.ref_end) == (located[0][j] + d["full"][j].t_beg - start[r], located[0][j] + d["full"][j].t_end - start[r])
                assert ln.cigar == d["cigars"][j] and (ln.q_beg, ln.q_end) == (d["full"][j].q_beg, d["full"][j].q_end)
        import tempfile

        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "all.sam")
            formats.write_sam_all(path, names, length, ["r%d" % p for p in range(n)], reads, None, res)
            _, refs, recs_ = formats.read_sam(path)
            assert refs == list(zip(names, length)) and len(recs_) == sum(c.n_lines) + 1
            flat = [ln for ls in res.lines for ln in ls]
            mapped = [r for r in recs_ if r.pos >= 0]
            assert len(mapped) == len(flat)
            for rec, ln in zip(mapped, flat):
                assert formats.reference_under_read(rec)[0] == contigs[ln.rid][1][ln.ref_beg:ln.ref_end] and rec.pos == ln.ref_beg
            text = open(path).read()
            assert text.count("SA:Z:") == 2 and text.count("tp:A:S") == 3  # the chimera's two lines; READ 0's copy and the split reads' second lines
    finally:
        index.close()
