"""Reads against a reference of contigs, on the GPU (map_reads_described_device and the list forms on an index of
build_index_contigs): synth.contig_mapping_set(11, 8, length=2000, spacer=3000, contigs=4) with the three adversarial reads and the
unrelated one of tests/contig_cases.py, both strands, on a stream of its own with one synchronisation.  Every stage's tuple is the
textbook composition's (tests/contig_textbook.py), the SAM rebuilds each contig under every read, and the same reads through an index
WITHOUT contigs over the same buffer still give what tests/index_textbook.py's map_reads gives."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contig_cases as cc  # noqa: E402
import index_cases as ic  # noqa: E402
from mgl_amd import _lib, formats, synth  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def aligner():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mgl_amd import smithwaterman as sw

    a = sw.MicrosoftSmithWaterman(0)
    assert a.load()
    yield a
    a.close()


def _eq(name, got, want, upto=None):
    got = got.cpu().numpy()[:upto].tolist()
    want = list(want)[:upto]
    assert len(got) == len(want), name
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if b is not None and a != b]
    assert not bad, (name, bad[:8], [got[i] for i in bad[:8]], [want[i] for i in bad[:8]])


def _stages_equal(got, seeded, chained, chosen, located, q_start, q_len):
    """the first four tuples of a mapper against the textbook's (None in the textbook: not written, not compared)"""
    total, chain_total, anchors = seeded[0][-1], chained[0][-1], chosen[2][-1]
    for i, name in enumerate(("cand_start", "cand_t", "cand_q", "cand_len")):
        _eq(name, got[0][i], seeded[i], total if i else None)
    _eq("seed status", got[0][6], seeded[4])
    _eq("row_t_len", got[0][4], seeded[5])
    _eq("row_q_len", got[0][5], seeded[6])
    for i, name in enumerate(("chain_start", "chain_t", "chain_q", "chain_len", "chain score", "f", "pred", "chain status")):
        _eq(name, got[1][i], chained[i], chain_total if i in (1, 2, 3) else total if i in (5, 6) else None)
    oriented = got[2][1].cpu().numpy()
    assert all(oriented[s:s + m].tobytes() == bytes(chosen[1][s:s + m]) for s, m in zip(q_start, q_len))
    for i, name in ((0, "strand"), (2, "anchor_start"), (3, "anchor_t"), (4, "anchor_q"), (5, "anchor_len"), (6, "chosen score"), (7, "choice status")):
        _eq(name, got[2][i], chosen[i], anchors if i in (3, 4, 5) else None)
    for i, name in enumerate(("t_start", "t_len", "rebased anchor_t", "window status", "rid")[:len(located)]):
        _eq(name, got[3][i], located[i], anchors if i == 2 else None)


def test_the_pipeline_over_contigs(aligner, tmp_path):
    from mgl_amd.smithwaterman import ContigDescribedMapResult, _pack_pairs

    dev = torch.device("cuda", 0)
    buffer, start, length, names, reads, _, textbook = cc.pipeline_textbook()
    seeded, groups, chained, chosen, located, fed, ranked = textbook
    want = cc.pipeline_described(True)
    contigs, _, truth = cc.pipeline_set()
    n = len(reads)
    _, packed, _ = _pack_pairs(reads, reads, dev, None, False)
    max_ql = packed[7]
    stride = 2 * max(ic.MAX_TL, max_ql)
    stages = dict(ic.SEEDING, **ic.CHAINING)
    align = dict(to_query_end=True, cigar_stride=stride)
    q_start, q_len = packed[4].cpu().numpy(), packed[5].cpu().numpy()
    index = aligner.build_index_contigs(contigs, cc.K, cc.W)
    plain = aligner.build_index(buffer, cc.K, cc.W)
    try:
        assert bytes(index.ref.cpu().numpy()) == buffer and index.contigs.names == names
        assert index.contigs.starts.tolist() == start and index.contigs.lens.tolist() == length
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            got = aligner.map_reads_described_device(index, *packed[3:6], ic.MAX_TL, max_ql, cc.BAND, cc.ZDROP, cc.GATK, slack=ic.SLACK, strands=2, **stages,
                                                     **align, **cc.RANKING)
            group = index.contig_of_device(got[0][1], got[0][3])
        torch.cuda.synchronize()  # the one synchronisation: nothing above waited for the device
        assert len(got) == 7 and len(got[3]) == 5

        # ---- the stages: the textbook composition's
        _eq("group", group, groups, seeded[0][-1])
        _stages_equal(got, seeded, chained, chosen, located, q_start, q_len)
        nc, rec = got[5][0].cpu().numpy(), got[5][1].cpu().numpy()
        assert nc.tolist() == ranked[0] and got[5][6].cpu().numpy().tolist() == ranked[6]
        for p in range(n):
            assert [tuple(int(v) for v in rec[p, c]) for c in range(nc[p])] == [tuple(r) for r in ranked[1][p]], p
        rid = got[3][4].cpu().numpy()
        assert rid.tolist() == [t[0] for t in truth] + [rid[cc.CHIMERA], 1, -1] and rid[cc.CHIMERA] in (0, 1)
        ast = got[4][6].cpu().numpy()
        assert ast.tolist() == want["status"] == [0] * 10 + [_lib.ERR_BAD_ARG]

        # ---- over lists: positions from the contig's start, rid and rname, the secondary chains' contigs
        res = aligner.map_reads_described(index, reads, cc.BAND, cc.ZDROP, cc.GATK, slack=ic.SLACK, strands=2, max_tl=ic.MAX_TL, extended=True, **stages,
                                          to_query_end=True, **cc.RANKING)
        assert isinstance(res, ContigDescribedMapResult)
        for f in ("ref_beg", "ref_end", "strand", "score", "status", "mapq", "n_chains", "q_beg", "q_end", "nm", "n_match", "block_len", "rid"):
            assert np.asarray(getattr(res, f)).tolist() == want[f], f
        assert list(res.cigars) == want["cigars"] and list(res.xcigars) == want["xcigars"] and res.md == want["md"]
        assert res.secondary == want["secondary"] and res.rname == want["rname"]
        assert res.mapq[0] == 0 and res.secondary[0][0][5] == 3 and res.rid[0] == 0  # the window that two contigs hold
        assert res.secondary[cc.CHIMERA][0][4] == 1 and {res.rid[cc.CHIMERA], res.secondary[cc.CHIMERA][0][5]} == {0, 1}  # the other half: primary
        assert res.ref_beg[cc.EDGE] >= 0 and abs(int(res.ref_beg[cc.EDGE]) - cc.EDGE_OFF) <= 2 and res.strand[cc.EDGE] == 1
        for p, (c, pos, m, strand) in enumerate(truth):
            assert res.rid[p] == c and res.strand[p] == strand and abs(int(res.ref_beg[p]) - pos) <= 40 and abs(int(res.ref_end[p]) - pos - m) <= 40
        ranked_res = aligner.map_reads_ranked(index, reads, cc.BAND, cc.ZDROP, cc.GATK, slack=ic.SLACK, strands=2, max_tl=ic.MAX_TL, **stages,
                                              to_query_end=True, **cc.RANKING)
        base = aligner.map_reads(index, reads, cc.BAND, cc.ZDROP, cc.GATK, slack=ic.SLACK, strands=2, max_tl=ic.MAX_TL, **stages, to_query_end=True)
        for f in ("ref_beg", "ref_end", "strand", "score", "status", "rid"):
            assert np.asarray(getattr(ranked_res, f)).tolist() == np.asarray(getattr(base, f)).tolist() == want[f], f
        assert ranked_res.rname == base.rname == want["rname"] and ranked_res.secondary == want["secondary"]

        # ---- the SAM: one @SQ per contig, and every read's record rebuilds ITS contig
        lens = [len(s) for _, s in contigs]
        read_names = ["read%d" % p for p in range(n)]
        for extended in (False, True):
            path = tmp_path / ("out%d.sam" % extended)
            formats.write_sam(path, names, lens, read_names, reads, None, res, extended=extended)
            _, refs, records = formats.read_sam(path)
            assert refs == list(zip(names, lens)) and len(records) == n
            for p, r in enumerate(records):
                if want["status"][p]:
                    assert (r.flag, r.ref_id, r.pos, r.cigar) == (4, -1, -1, [])
                    continue
                assert r.ref_id == res.rid[p] and r.pos == res.ref_beg[p] and r.seq == (synth.revcomp(reads[p]) if res.strand[p] else reads[p])
                under, edits = formats.reference_under_read(r)
                span = sum(k for k, op in r.cigar if op in "M=XD")
                assert under == contigs[r.ref_id][1][r.pos:r.pos + span] and edits == r.tags["NM"] == res.nm[p] and r.mapq == res.mapq[p]
        paf = tmp_path / "out.paf"
        formats.write_paf(paf, names, lens, read_names, reads, res)
        lines = [x.split("\t") for x in open(paf).read().splitlines()]
        assert len(lines) == 10
        for line, p in zip(lines, range(10)):
            assert line[5:9] == [names[res.rid[p]], str(lens[res.rid[p]]), str(int(res.ref_beg[p])), str(int(res.ref_end[p]))]

        # ---- nothing changed for an index without contigs: the same buffer as ONE sequence is index_textbook.map_reads
        old = cc.pipeline_ungrouped()
        got = aligner.map_reads_device(plain, *packed[3:6], ic.MAX_TL, max_ql, cc.BAND, cc.ZDROP, cc.GATK, slack=ic.SLACK, strands=2, **stages, **align)
        torch.cuda.synchronize()
        assert len(got[3]) == 4 and got[1][5] is None
        chained_plain = list(old[1])
        chained_plain[5] = chained_plain[6] = None
        seeded_o, chosen_o, located_o = old[0], old[2], old[3]
        total, chain_total, anchors = seeded_o[0][-1], chained_plain[0][-1], chosen_o[2][-1]
        for i, name in enumerate(("cand_start", "cand_t", "cand_q", "cand_len")):
            _eq(name, got[0][i], seeded_o[i], total if i else None)
        for i, name in ((0, "chain_start"), (1, "chain_t"), (2, "chain_q"), (3, "chain_len"), (4, "chain score"), (7, "chain status")):
            _eq(name, got[1][i], chained_plain[i], chain_total if i in (1, 2, 3) else None)
        for i, name in ((0, "strand"), (2, "anchor_start"), (3, "anchor_t"), (4, "anchor_q"), (5, "anchor_len")):
            _eq(name, got[2][i], chosen_o[i], anchors if i in (3, 4, 5) else None)
        for i, name in enumerate(("t_start", "t_len", "rebased anchor_t", "window status")):
            _eq(name, got[3][i], located_o[i], anchors if i == 2 else None)
        # and there the chimeric read's window does hold the gap: what the contig stages are for
        t_start, t_len = got[3][0].cpu().numpy(), got[3][1].cpu().numpy()
        assert t_start[cc.CHIMERA] < start[1] - 1 < t_start[cc.CHIMERA] + t_len[cc.CHIMERA]
        plain_res = aligner.map_reads(plain, reads, cc.BAND, cc.ZDROP, cc.GATK, slack=ic.SLACK, strands=2, max_tl=ic.MAX_TL, **stages, to_query_end=True)
        assert type(plain_res).__name__ == "MapResult" and len(plain_res) == 6
    finally:
        index.close()
        plain.close()
