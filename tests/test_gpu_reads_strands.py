"""Reads of either strand -> seeds of both orientations -> chains of the 2n rows -> the strand -> the alignment, on a stream of its own
with one synchronisation at the end (align_reads_strands_device), against align_reads_device fed the correctly oriented reads from the
host: 16 pairs with known chains of which every odd read is given reverse-complemented, and one pair of unrelated sequences."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seed_cases as cases  # noqa: E402
from mgl_amd import _lib, synth  # noqa: E402

pytestmark = pytest.mark.gpu

GATK = (200, -150, 260, 11)
CHAINING = dict(max_pred=64, max_dist=1000, bw=500, pen_gap=38, pen_skip=0)


@pytest.fixture(scope="module")
def aligner():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mgl_amd import smithwaterman as sw

    a = sw.MicrosoftSmithWaterman(0)
    assert a.load()
    yield a
    a.close()


@pytest.mark.parametrize("k,w", [(15, 10), (11, 5)])
def test_reads_of_either_strand_equal_the_oriented_reads_through_the_one_strand_pipeline(aligner, k, w):
    from mgl_amd.smithwaterman import _pack_pairs

    dev = torch.device("cuda", 0)
    pairs = synth.chain_pairs(11, 16, length=2000)
    rng = np.random.default_rng(62)  # (a seed at which the unrelated pair shares no minimizer on either row: seed 61 shares one 11-mer)
    Ts = [p[0] for p in pairs] + [cases.rand_seq(rng, 1500)]
    oriented = [p[1] for p in pairs] + [cases.rand_seq(rng, 1400)]
    truth = [i % 2 for i in range(16)] + [0]  # (a pair with chains on neither row is strand 0)
    given = [synth.revcomp(Q) if s else Q for Q, s in zip(oriented, truth)]
    n, packed, stride = _pack_pairs(Ts, given, dev, None, False)
    _, packed_oriented, _ = _pack_pairs(Ts, oriented, dev, None, False)
    align = dict(to_query_end=True, cigar_stride=stride, sides=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        seeds, chain, chosen, got = aligner.align_reads_strands_device(*packed, 64, -1, GATK, k, w, 8, True, 2048, **CHAINING, **align)
    torch.cuda.synchronize()  # the one synchronisation: nothing above waited for the device
    _, want_chain, want = aligner.align_reads_device(*packed_oriented, 64, -1, GATK, k, w, 8, True, 2048, **CHAINING, **align)
    torch.cuda.synchronize()
    strand, reads, anchor_start, at, aq, al, score, status = (x.cpu().numpy() for x in chosen)
    assert strand.tolist() == truth and (status == 0).all()
    assert (seeds[6].cpu().numpy() == 0).all() and (chain[7].cpu().numpy() == 0).all()
    q_start, q_len = packed[4].cpu().numpy(), packed[5].cpu().numpy()
    want_reads = packed_oriented[3].cpu().numpy()
    assert all((reads[a:a + m] == want_reads[a:a + m]).all() for a, m in zip(q_start, q_len))
    # the chosen chains are the oriented reads' chains
    wcs, wct, wcq, wcl, wscore = (x.cpu().numpy() for x in want_chain[:5])
    assert (anchor_start == wcs).all() and (score == wscore).all() and anchor_start[16] == anchor_start[17] and anchor_start[16] > 16 * 5
    tot = int(wcs[-1])
    assert (at[:tot] == wct[:tot]).all() and (aq[:tot] == wcq[:tot]).all() and (al[:tot] == wcl[:tot]).all()
    # every array of the alignment; a CIGAR row up to its length (the entry writes no byte at or beyond it)
    got, want = [None if x is None else x.cpu().numpy() for x in got], [None if x is None else x.cpu().numpy() for x in want]
    assert len(got) == len(want) == 7
    for i, (a, b) in enumerate(zip(got, want)):
        assert (a is None) == (b is None)
        if a is None:
            continue
        if i == 4:
            a, b = a.reshape(n, -1), b.reshape(n, -1)
            assert all((a[p, :got[5][p]] == b[p, :got[5][p]]).all() for p in range(16))
        elif i in (0, 1, 2, 5):
            assert (a[:16] == b[:16]).all(), i  # (what a refused pair's record holds is not defined)
        else:
            assert (a == b).all(), i
    assert got[6].tolist() == [0] * 16 + [_lib.ERR_BAD_ARG]
    aln = got[0][:16]
    assert (aln[:, 1] <= 200).all() and (aln[:, 2] >= np.array([len(T) for T in Ts[:16]]) - 200).all()
