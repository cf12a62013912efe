"""What tests/test_sam_paf.py (CPU) and tests/test_gpu_map_reads_described.py (GPU) share: the textbook composition of the described read
mapper over tests/rank_cases.py's reads -- index_textbook.map_reads, rank_textbook.rank_batch, chain_textbook.chain_align on every
read's window and describe_textbook.describe on the alignment -- as a DescribedMapResult."""
import functools

import numpy as np

import chain_textbook as ctb
import describe_textbook as dtb
import index_cases as ic
import rank_cases as rc
import seed_cases

GATK = (200, -150, 260, 11)
BAND, ZDROP = 64, -1
BAD_ARG = 1
UNRELATED = seed_cases.rand_seq(np.random.default_rng(2), 120)  # (it shares no minimizer with the reference: the textbook finds no candidate)
TAIL = b"N" * 30  # unrelated sequence behind a read: what a clip is made of.  (Random bases would not do: with a match at 200 and a gap
# base at 11 the extension threads long gaps through them and reaches the read's end)


def reads_of(divergence):
    """what goes behind the eight reads of DESIGN.md section 9k: a read of unrelated sequence (unmapped: the nine reads of
    tests/test_gpu_map_reads_ranked.py), and -- those nine have no clip, the extension reaches every read's end -- the first two
    reads once more with 30 bases of unrelated sequence cut onto their ends: without to_query_end the alignment stops in front of
    them, a clip behind the read of strand 0 and in front of the oriented read of strand 1"""
    _, reads, _, _ = rc.repeat_set(divergence)
    return (UNRELATED, bytes(reads[0]) + TAIL, bytes(reads[1]) + TAIL)


@functools.lru_cache(maxsize=None)
def mapped(divergence, to_query_end):
    """-> (ref, reads, names, DescribedMapResult with lists of text for cigars and xcigars, [Description or None])"""
    from mgl_amd.smithwaterman import DescribedMapResult
    from mgl_amd import formats

    ref, reads, truth, copy, got, ranked = rc.repeat_mapped(divergence, reads_of(divergence))
    chosen, fed = got[2], got[4]
    nc, recs = ranked[0], ranked[1]
    n = len(reads)
    cols = {f: [] for f in DescribedMapResult._fields}
    descs = []
    for p, (oriented, t_start, t_len, anchors) in enumerate(fed):
        if not anchors:
            for f in ("ref_beg", "ref_end", "strand", "score", "q_beg", "q_end", "nm", "n_match", "block_len"):
                cols[f].append(0)
            cols["cigars"].append(""), cols["xcigars"].append(""), cols["md"].append(b""), cols["status"].append(BAD_ARG)
            descs.append(None)
        else:
            T = ref[t_start:t_start + t_len]
            aln, cigar, *_ = ctb.chain_align(T, oriented, anchors, *GATK, BAND, ZDROP, to_query_end)
            d = dtb.describe(T[aln.t_beg:aln.t_end], oriented[aln.q_beg:aln.q_end], formats.cigar_text_to_elements(cigar))
            for f, v in (("ref_beg", t_start + aln.t_beg), ("ref_end", t_start + aln.t_end), ("strand", chosen[0][p]), ("score", aln.score), ("q_beg", aln.q_beg),
                         ("q_end", aln.q_end), ("nm", dtb.nm(d)), ("n_match", d.n_match), ("block_len", dtb.block_len(d)), ("cigars", cigar),
                         ("xcigars", dtb.xcigar_text(d.xcigar)), ("md", d.md), ("status", 0)):
                cols[f].append(v)
            descs.append(d)
        cols["mapq"].append(recs[p][0].mapq if recs[p] else 0)
        cols["n_chains"].append(nc[p])
        cols["secondary"].append([(r.t_beg, r.t_end, r.strand, r.score, r.parent) for r in recs[p][1:]])
    arr = lambda f: np.asarray(cols[f], np.int64 if f in ("ref_beg", "ref_end") else np.int32)  # noqa: E731
    res = DescribedMapResult(*[cols[f] if f in ("cigars", "secondary", "md", "xcigars") else arr(f) for f in DescribedMapResult._fields])
    names = ["read%d" % p for p in range(n)]
    return ref, [bytes(r) for r in reads], names, res, descs
