"""What tests/test_contig_textbook.py, tests/test_sam_contigs.py (CPU) and the GPU tests of the contig stages share: hand-made tables and
anchors, and the reads of the pipeline test with their textbook composition.

The pipeline's reference is synth.contig_mapping_set(11, 8, length=2000, spacer=3000, contigs=4) with the window of read 0 copied once
more, behind 500 random bases, onto the end of the last contig.  Behind the eight reads of the set come
  CHIMERA   the last 600 bases of contig 0 followed by the first 600 of contig 1, every 61st base substituted
  EDGE      600 bases of contig 1 from its base 20 on, substituted likewise and given reverse-complemented
  UNRELATED a read that shares no minimizer with the reference
and read 0 is the one whose window two contigs hold."""
import functools

import numpy as np

import contig_textbook as gtb
import index_cases as ic
import index_textbook as itb
import rank_cases as rc
import seed_cases

CANARY = ic.CANARY
GATK = (200, -150, 260, 11)
BAND, ZDROP = 64, -1
K, W = rc.K, rc.W
RANKING = rc.RANKING
CHIMERA, EDGE, UNRELATED_AT = 8, 9, 10
HALF, EDGE_OFF = 600, 20


def _substituted(seq, every=61):
    """every 61st base replaced by the next of A, C, G, T: an exact copy would merge into ONE anchor, and the rank stage wants three"""
    out = bytearray(seq)
    for i in range(every // 2, len(out), every):
        out[i] = b"CGTA"[b"ACGT".index(out[i])]
    return bytes(out)


@functools.lru_cache(maxsize=None)
def pipeline_set():
    """-> (contigs [(name, bytes)], reads, truth [(rid, pos, len, strand)] of the first eight reads)"""
    from mgl_amd import synth

    contigs, reads, truth = synth.contig_mapping_set(11, 8, length=2000, spacer=3000, contigs=4)
    rid, pos, n, _ = truth[0]
    rng = np.random.default_rng(97)
    filler = lambda m: seed_cases.rand_seq(rng, m)  # noqa: E731
    name, last = contigs[3]
    contigs = contigs[:3] + [(name, last + filler(500) + contigs[rid][1][pos:pos + n] + filler(500))]
    chimera = _substituted(contigs[0][1][-HALF:] + contigs[1][1][:HALF])
    edge = synth.revcomp(_substituted(contigs[1][1][EDGE_OFF:EDGE_OFF + HALF]))
    unrelated = seed_cases.rand_seq(np.random.default_rng(2), 120)
    return contigs, [bytes(r) for r in reads] + [chimera, edge, unrelated], truth


def stage_args():
    c, s = ic.CHAINING, ic.SEEDING
    return (s["max_occ"], s["max_occ_ref"], s["merge"], s["max_cand"]), (c["max_pred"], c["max_dist"], c["max_dist"], c["bw"], c["pen_gap"], c["pen_skip"])


@functools.lru_cache(maxsize=None)
def pipeline_textbook():
    """-> (buffer, start, length, names, reads, index, map_reads_contigs' tuple)"""
    contigs, reads, _ = pipeline_set()
    buffer, start, length = gtb.layout([s for _, s in contigs])
    index = itb.by_key(itb.build_index(buffer, K, W))
    seeding, chaining = stage_args()
    got = gtb.map_reads_contigs(index, len(buffer), start, length, reads, K, W, 2, *seeding, 2 * len(reads) * seeding[3], *chaining, ic.SLACK, ic.MAX_TL,
                                ranking=tuple(RANKING[f] for f in ("max_chains", "min_score", "min_cnt", "mask_level")))
    return buffer, start, length, [n for n, _ in contigs], reads, index, got


@functools.lru_cache(maxsize=None)
def pipeline_ungrouped():
    """index_textbook.map_reads on the same buffer as ONE sequence: what the contig stages are there to prevent"""
    buffer, _, _, _, reads, index, _ = pipeline_textbook()
    seeding, chaining = stage_args()
    return itb.map_reads(index, len(buffer), reads, K, W, 2, *seeding, 2 * len(reads) * seeding[3], *chaining, ic.SLACK, ic.MAX_TL)


@functools.lru_cache(maxsize=None)
def pipeline_described(to_query_end=True):
    """-> contig_textbook.describe_mapped's columns for the pipeline's reads"""
    buffer, start, _, names, _, _, got = pipeline_textbook()
    _, _, _, chosen, located, fed, ranked = got
    return gtb.describe_mapped(buffer, start, names, fed, chosen, located, ranked, GATK, BAND, ZDROP, to_query_end)


# ---- hand-made tables: contigs of 100, 1, 50 and 3 bases with gaps of 1, 2 and 1
TABLE = ([0, 101, 104, 155], [100, 1, 50, 3])
TABLE_LEN = 158


def contig_of_edges(start, length):
    """anchors (t, l) at every edge of every contig: at start, at end - 1, at end, crossing the end by one, one in front of the start,
    and the anchors contig_of refuses whatever the table"""
    out = [(-1, 5), (0, 0), (0, -3), (5, 0)]
    for s, n in zip(start, length):
        e = s + n
        out += [(s, 1), (s, n), (s, n + 1), (e - 1, 1), (e - 1, 2), (e, 1), (s - 1, 1), (s - 1, 2), (e - n // 2 - 1, n // 2 + 1), (e - n // 2 - 1, n // 2 + 2)]
    return out + [(start[-1] + length[-1], 1), (start[-1] + length[-1] + 7, 1), (2 ** 31 - 2, 1), (2 ** 31 - 1, 2 ** 31 - 1)]


def locate_cases():
    """-> (start, length, slack, max_tl, [(name, ql, anchors, status, t_start, t_len, rid)]) over contigs [0, 1000), [1001, 3001), [3002, 3502)"""
    start, length = [0, 1001, 3002], [1000, 2000, 500]
    cases = [
        ("inside", 300, [(1500, 10, 20), (1700, 210, 20)], 0, 1440, 400, 1),
        ("clipped at the contig's start", 300, [(1021, 10, 20), (1200, 190, 20)], 0, 1001, 359, 1),
        ("clipped at the contig's end", 300, [(2700, 10, 20), (2950, 260, 20)], 0, 2640, 361, 1),
        ("clipped on either side", 700, [(3012, 100, 20), (3400, 488, 20)], 0, 3002, 500, 2),
        ("the first contig, clipped at 0", 200, [(30, 60, 20)], 0, 0, 220, 0),
        ("a chain over two contigs", 400, [(900, 10, 20), (1100, 210, 20)], gtb.BAD_ARG, 0, 0, -1),
        ("an anchor over a contig's end", 400, [(900, 10, 20), (990, 100, 11)], gtb.BAD_ARG, 0, 0, -1),
        ("the first anchor in a gap", 400, [(1000, 10, 1), (1100, 210, 20)], gtb.BAD_ARG, 0, 0, -1),
        ("unmapped", 400, [], 0, 0, 0, -1),
        ("above max_tl", 900, [(1500, 0, 20), (2301, 800, 20)], gtb.UNSUPPORTED, 0, 0, -1),
        ("at max_tl", 900, [(1500, 0, 20), (2300, 800, 20)], 0, 1450, 1000, 1),
        ("q + l above ql", 100, [(1500, 90, 20)], gtb.BAD_ARG, 0, 0, -1),
    ]
    return start, length, 50, 1000, cases


def csr(chains):
    return ic.csr(chains)
