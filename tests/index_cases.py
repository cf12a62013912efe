"""What tests/test_index_textbook.py (the textbook against restatements and against its own conditions) and the GPU tests of the index
family share: the hand-made chains of locate_window, and the reads of the pipeline test with the parameters they are mapped at."""
import functools

import numpy as np

import index_textbook as itb
import seed_cases as cases

CANARY = cases.CANARY
CHAINING = dict(max_pred=64, max_dist=1000, bw=500, pen_gap=38, pen_skip=0)  # section 9i's
SEEDING = dict(max_occ=8, max_occ_ref=64, merge=1, max_cand=2048)
# the flanks of synth.chain_pairs carry 30-base insertions in front of the first anchor and a per cent of small indels: at 200 the
# textbook's windows hold every read's true span (test_index_textbook.py asserts it)
SLACK = 200
MAX_TL = 2600


@functools.lru_cache(maxsize=None)
def mapping():
    from mgl_amd import synth

    return synth.mapping_set(11, 16, length=2000, spacer=3000)


@functools.lru_cache(maxsize=None)
def mapped(k, w, extra=()):
    """the textbook composition over the 16 reads (and `extra` ones behind them) at (k, w) -> (ref, reads, truth, map_reads' tuple)"""
    ref, reads, truth = mapping()
    reads = list(reads) + list(extra)
    c, s = CHAINING, SEEDING
    got = itb.map_reads(itb.build_index(ref, k, w), len(ref), reads, k, w, 2, s["max_occ"], s["max_occ_ref"], s["merge"], s["max_cand"],
                        2 * len(reads) * s["max_cand"], c["max_pred"], c["max_dist"], c["max_dist"], c["bw"], c["pen_gap"], c["pen_skip"], SLACK, MAX_TL)
    return ref, reads, truth, got


def locate_cases():
    """-> (ref_len, slack, max_tl, [(name, ql, [(t, q, l)], expected status)]): chains clipped at either end of the reference, K = 0 and
    K = 1, every refusal, max_tl exact and one above"""
    ref_len, slack, max_tl = 10000, 100, 1500
    out = [
        ("plain", 1000, [(3000, 10, 20), (3400, 420, 30), (3900, 930, 40)], 0),
        ("clipped-at-0", 1000, [(50, 200, 20), (500, 640, 25)], 0),
        ("clipped-at-ref_len", 1000, [(9200, 100, 20), (9900, 800, 100)], 0),
        ("clipped-at-both", 1400, [(20, 100, 20), (9980, 1370, 20)], itb.UNSUPPORTED),
        ("K=0", 500, [], 0),
        ("K=1", 300, [(5000, 100, 15)], 0),
        ("K=1-at-the-ends", 15, [(9985, 0, 15)], 0),
        ("ql<1", 0, [(100, 0, 10)], itb.BAD_ARG),
        ("l<1", 500, [(100, 10, 10), (200, 110, 0)], itb.BAD_ARG),
        ("t<0", 500, [(-1, 10, 10), (200, 110, 10)], itb.BAD_ARG),
        ("q<0", 500, [(100, -1, 10), (200, 110, 10)], itb.BAD_ARG),
        ("t+l>ref_len", 500, [(100, 10, 10), (9995, 110, 6)], itb.BAD_ARG),
        ("q+l>ql", 500, [(100, 10, 10), (200, 491, 10)], itb.BAD_ARG),
        ("t+l=ref_len,q+l=ql", 500, [(9500, 10, 10), (9990, 490, 10)], 0),
        # lo = 2000 - 0 - 100, hi = 3300 + (1300 - 1300) + 100 with q along the diagonal: hi - lo = 1500 = max_tl, and one above
        ("max_tl-exact", 1300, [(2000, 0, 10), (3290, 1290, 10)], 0),
        ("max_tl+1", 1300, [(2000, 0, 10), (3291, 1290, 10)], itb.UNSUPPORTED),
        ("many", 1200, [(4000 + 11 * i, 5 + 11 * i, 10) for i in range(100)], 0),
    ]
    return ref_len, slack, max_tl, out


def csr(chains):
    """lists of anchors -> (anchor_start, anchor_t, anchor_q, anchor_len)"""
    start = np.zeros(len(chains) + 1, np.int64)
    if chains:
        np.cumsum([len(c) for c in chains], out=start[1:])
    flat = np.asarray([a for c in chains for a in c], dtype=np.int32).reshape(-1, 3)
    return start, flat[:, 0].copy(), flat[:, 1].copy(), flat[:, 2].copy()
