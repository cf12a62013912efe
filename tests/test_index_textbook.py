"""tests/index_textbook.py against restatements of its own definitions and against seed_textbook.py where the two must agree, and the
conditions on the inputs of tests/test_gpu_map_reads.py: the textbook composition finds the true strand and a window that holds the
true span for every one of the 16 reads.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import index_cases as ic  # noqa: E402
import index_textbook as itb  # noqa: E402
import seed_cases as cases  # noqa: E402
import seed_textbook as stb  # noqa: E402
import strand_textbook as rtb  # noqa: E402


def _brute_index(R, k, w):
    """every window's minimum, restated: per window the valid k-mer with the smallest (hash, position)"""
    code = {65: 0, 67: 1, 71: 2, 84: 3}
    nk = len(R) - k + 1
    if nk < 1:
        return []
    keys = []
    for i in range(nk):
        cs = [code.get(b) for b in R[i:i + k]]
        keys.append(None if None in cs else int("".join(str(c) for c in cs), 4))
    picked = set()
    for a in range(max(nk - w, 0) + 1):
        valid = [(stb.kmer_hash(keys[i]), i) for i in range(a, min(a + w, nk)) if keys[i] is not None]
        if valid:
            picked.add(min(valid)[1])
    out = [(keys[i], i) for i in picked]
    out.sort(key=lambda e: e[0] * (1 << 32) + e[1])
    return out


@pytest.mark.parametrize("k", [4, 11, 15, 16])
def test_build_index_is_ascending_and_equals_a_brute_force_restatement(k):
    rng = np.random.default_rng(k)
    for w in (1, 10, 32):
        for alphabet in (b"AC", b"ACGT"):
            R = bytearray(cases.rand_seq(rng, int(rng.integers(40, 400)), alphabet))
            R[int(rng.integers(len(R)))] = ord("N")
            index = itb.build_index(bytes(R), k, w)
            assert index == _brute_index(bytes(R), k, w) and len(index) > 0
            assert all(a < b for a, b in zip(index, index[1:]))
    assert itb.build_index(b"ACG", 4, 1) == [] and itb.build_index(b"N" * 50, 4, 3) == []


@pytest.mark.parametrize("k", [4, 11, 15, 16])
def test_a_row_equals_seed_pair_against_the_reference_while_no_key_exceeds_max_occ_ref(k):
    rng = np.random.default_rng(100 + k)
    seen = 0
    for w in (1, 10, 32):
        for alphabet in (b"AC", b"ACGT"):
            R = bytearray(cases.rand_seq(rng, int(rng.integers(150, 500)), alphabet))
            R[int(rng.integers(len(R)))] = ord("N")
            R = bytes(R)
            a = int(rng.integers(0, len(R) - 120))
            Q = cases.mutate(rng, R[a:a + 120])
            index = itb.build_index(R, k, w)
            top = max((len(v) for v in itb.by_key(index).values()), default=0)
            for max_occ, merge in ((8, 1), (2, 0), (64, 1)):
                for max_occ_ref in {max(top, 1), 8192}:
                    got = itb.seed_index_row(index, len(R), Q, k, w, max_occ, max_occ_ref, merge, 8192)
                    want = stb.seed_pair(R, Q, k, w, max_occ, merge, 8192)
                    assert got == want
                    seen += len(got.cands)
    assert seen > 0


def test_a_key_at_max_occ_ref_is_kept_and_one_above_is_dropped():
    rng = np.random.default_rng(3)
    kmer = b"ACGTTGCAAGC"
    pad = lambda: cases.rand_seq(rng, 9, b"CT")  # noqa: E731  (C and T only: the k-mer, with its A and G, occurs nowhere else)
    R = b"".join(pad() + kmer for _ in range(5)) + pad()
    Q = pad() + kmer + pad()
    k = len(kmer)
    index = itb.build_index(R, k, 1)
    key = stb.kmers(kmer, k)[0]
    assert len(itb.by_key(index)[key]) == 5
    kept = itb.seed_index_row(index, len(R), Q, k, 1, 8, 5, 0, 4096)
    dropped = itb.seed_index_row(index, len(R), Q, k, 1, 8, 4, 0, 4096)
    assert [c for c in kept.cands if c[1] == 9] == [(9 + 20 * i, 9, k) for i in range(5)]
    assert [c for c in dropped.cands if c[1] == 9] == [] and dropped.status == 0
    assert len(kept.cands) == len(dropped.cands) + 5
    # and the read's side: the k-mer twice in the read, max_occ 2 and 1
    Q2 = pad() + kmer + pad() + kmer
    assert len(itb.seed_index_row(index, len(R), Q2, k, 1, 2, 5, 0, 4096).cands) >= 10
    assert not [c for c in itb.seed_index_row(index, len(R), Q2, k, 1, 1, 5, 0, 4096).cands if c[1] in (9, 29)]
    # the bounds: raw hits above max_cand, an empty read
    assert itb.seed_index_row(index, len(R), Q2, k, 1, 2, 5, 0, 9).status == itb.UNSUPPORTED
    assert itb.seed_index_row(index, len(R), b"", k, 1, 2, 5, 0, 9).status == itb.BAD_ARG


def test_rows_of_two_strands_are_the_strand_textbooks_rows_and_the_capacity_rule_is_per_row():
    rng = np.random.default_rng(4)
    R = cases.rand_seq(rng, 600)
    Qs = [R[50:150], rtb.revcomp(R[300:420]), b"", R[200:260] + rtb.revcomp(R[400:470])]
    index = itb.build_index(R, 11, 3)
    one = itb.seed_index_batch(index, len(R), Qs, 11, 3, 1, 8, 64, 1, 512, 1 << 20)
    two = itb.seed_index_batch(index, len(R), Qs, 11, 3, 2, 8, 64, 1, 512, 1 << 20)
    oriented = rtb.rows(Qs, Qs)[1]
    assert itb.rows(Qs, 2) == oriented and itb.rows(Qs, 1) == Qs
    want = [itb.seed_index_row(index, len(R), Q, 11, 3, 8, 64, 1, 512) for Q in oriented]
    for r, row in enumerate(want):
        a, b = two[0][r], two[0][r + 1]
        assert list(zip(two[1][a:b], two[2][a:b], two[3][a:b])) == row.cands and two[4][r] == row.status
        if r % 2 == 0:
            c, d = one[0][r // 2], one[0][r // 2 + 1]
            assert list(zip(one[1][c:d], one[2][c:d], one[3][c:d])) == row.cands
    assert two[5] == [600] * 8 and two[6] == [len(Q) for Q in oriented]
    counts = np.diff(two[0])
    assert counts[0] > 0 and counts[1] == 0 and counts[2] == 0 and counts[3] > 0 and counts[6] > 0 and counts[7] > 0
    assert two[4] == [0, 0, 0, 0, itb.BAD_ARG, itb.BAD_ARG, 0, 0]
    cut = itb.seed_index_batch(index, len(R), Qs, 11, 3, 2, 8, 64, 1, 512, int(two[0][7]) - 1)
    assert cut[4] == [0, 0, 0, 0, itb.BAD_ARG, itb.BAD_ARG, itb.NOMEM, itb.NOMEM] and cut[0][-1] == two[0][6]


def test_locate_window_on_hand_made_chains():
    ref_len, slack, max_tl, chains = ic.locate_cases()
    start, at, aq, al = ic.csr([c[2] for c in chains])
    q_len = [c[1] for c in chains]
    t_start, t_len, out, status = itb.locate_window(ref_len, q_len, start, at, aq, al, slack, max_tl)
    assert status == [c[3] for c in chains]
    by_name = {c[0]: p for p, c in enumerate(chains)}
    got = lambda name: (t_start[by_name[name]], t_len[by_name[name]])  # noqa: E731
    assert got("plain") == (2890, 1180) and got("clipped-at-0") == (0, 960) and got("clipped-at-ref_len") == (9000, 1000)
    assert got("K=0") == (0, 0) and got("K=1") == (4800, 500) and got("K=1-at-the-ends") == (9885, 115)
    assert got("max_tl-exact") == (1900, 1500) and got("max_tl+1") == (0, 0) and got("t+l=ref_len,q+l=ql") == (9390, 610)
    for p, (name, _, anchors, st) in enumerate(chains):
        a, b = int(start[p]), int(start[p + 1])
        if st:
            assert (t_start[p], t_len[p]) == (0, 0) and out[a:b] == [None] * (b - a), name
        else:
            assert out[a:b] == [t - t_start[p] for t, _, _ in anchors] and all(x >= 0 for x in out[a:b]), name
    # slack = 0: the window is the chain's span and what the read's ends need
    assert itb.locate_window(ref_len, [1000], [0, 2], [3000, 3400], [10, 420], [20, 30], 0, max_tl)[:2] == ([2990], [3430 + 550 - 2990])
    # a range of anchor_start that descends or leaves [0, total_anchors]
    for bad in ([2, 1], [-1, 1], [0, 3]):
        assert itb.locate_window(ref_len, [1000], bad, [3000, 3400], [10, 420], [20, 30], 0, max_tl)[3] == [itb.BAD_ARG]
    assert itb.locate_window(ref_len, [1000], [0, 2], [3000, 3400], [10, 420], [20, 30], 0, max_tl, total_anchors=1)[3] == [itb.BAD_ARG]


@pytest.mark.parametrize("k,w", [(15, 10), (11, 5)])
def test_the_inputs_of_the_pipeline_test_the_textbook_maps_16_of_16(k, w):
    ref, reads, truth, (seeded, chained, chosen, located, fed) = ic.mapped(k, w)
    assert len(reads) == 16 and all(len(r) > 1500 for r in reads) and len(ref) > 16 * 4500
    from mgl_amd import synth

    pairs = synth.chain_pairs(11, 16, length=2000)
    assert all(ref[pos:pos + n] == pairs[p][0] and s == p % 2 for p, (pos, n, s) in enumerate(truth))
    assert all(reads[p] == (synth.revcomp(pairs[p][1]) if p % 2 else pairs[p][1]) for p in range(16))
    assert chosen[0] == [s for _, _, s in truth]                                   # the true strand, 16 of 16
    t_start, t_len, _, status = located
    assert status == [0] * 16 and seeded[4] == [0] * 32 and chained[7] == [0] * 32
    assert all(a <= pos and pos + n <= a + m for (pos, n, _), a, m in zip(truth, t_start, t_len))  # the window holds the true span, 16 of 16
    assert max(t_len) <= ic.MAX_TL
    for (Q, a, m, anchors), (pos, n, s) in zip(fed, truth):
        assert len(anchors) >= 5 and all(ref[a + t:a + t + l] == Q[q:q + l] for t, q, l in anchors)  # every anchor is an exact match in place
