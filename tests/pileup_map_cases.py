"""The pipeline's inputs for the pileup (tests/test_pileup_pipeline.py on the CPU, tests/test_gpu_map_reads_pileup.py on the GPU):
lines_cases.compose's composition of the CPU textbooks, extended by the pileup and sites textbooks, over lines_cases' contig reads and
over synth.variant_mapping_set -- a donor with planted substitutions, a deletion and an insertion, tiled by exact reads --, and the
planted truth as both tests assert it."""
import functools

import lines_cases as lc
import pileup_textbook as ptb

GATK = (200, -150, 260, 11)
BAND, ZDROP = 64, -1
SITES = (4, 2, 64)  # pileup_sites_device's defaults
CONTIG_SITES = (1, 1, 64)  # the contig reads lie one deep
VARIANT_SEED = 5
# the variant set's reads are exact copies of the donor: between two variants their minimizers merge into ONE anchor, and a read with
# fewer than two variants has fewer than the three anchors the rank stage asks for by default -- so this set is mapped with min_cnt = 1
VARIANT_RANKING = dict(max_chains=4, min_score=40, min_cnt=1, mask_level=128)


def selected(line, status, min_mapq=0):
    """map_reads_pileup_device's select and the alignment's status: which job is counted"""
    return status == 0 and line is not None and line.order >= 0 and not line.flag & 0x100 and line.mapq >= min_mapq


def alignments(d, reads, min_mapq=0):
    """compose's dict -> the textbook's alignments of the counted jobs: the position is the window's start and the record's t_beg"""
    from mgl_amd import formats

    e, c, out = d["expanded"], d["classified"], []
    for j, job in enumerate(e.jobs):
        if job.read < 0 or not selected(c.lines[j], d["aln_status"][j], min_mapq):
            continue
        r = d["full"][j]
        q = bytes(reads[job.read])
        q = lc.ltb.revcomp(q) if job.strand else q
        out.append((d["located"][0][j] + r.t_beg, q[r.q_beg:r.q_end], formats.cigar_text_to_elements(d["cigars"][j])))
    return out


def piled(d, reads, buffer, min_mapq=0, params=SITES):
    """-> (counts [8][len(buffer)], the sites textbook's (call, flags, sites))"""
    counts = ptb.pileup(alignments(d, reads, min_mapq), 0, len(buffer))
    return counts, ptb.sites(counts, buffer, 0, *params)


@functools.lru_cache(maxsize=None)
def contig_piled():
    """over lines_cases.contig_composed(False) -> (buffer, start, length, names, reads, compose's dict, counts, sites' tuple)"""
    buffer, start, length, names, reads, _, d = lc.contig_composed(False)
    return (buffer, start, length, names, reads, d) + piled(d, reads, buffer, params=CONTIG_SITES)


@functools.lru_cache(maxsize=None)
def variant_set():
    from mgl_amd import synth

    return synth.variant_mapping_set(VARIANT_SEED)


def variant_stages():
    """the arguments of the mappers on the variant set, as the GPU test passes them"""
    import index_cases as ic

    return dict(ic.SEEDING, **ic.CHAINING, **VARIANT_RANKING, slack=ic.SLACK, strands=2, to_query_end=False)


@functools.lru_cache(maxsize=None)
def variant_piled():
    """the textbook composition over variant_mapping_set() against a plain index -> (ref, reads, planted, compose's dict, counts,
    sites' tuple)"""
    import index_cases as ic
    import index_textbook as itb
    import rank_cases as rc
    import rank_textbook as rtb

    ref, reads, planted = variant_set()
    c, s = ic.CHAINING, ic.SEEDING
    got = itb.map_reads(itb.build_index(ref, rc.K, rc.W), len(ref), reads, rc.K, rc.W, 2, s["max_occ"], s["max_occ_ref"], s["merge"], s["max_cand"],
                        2 * len(reads) * s["max_cand"], c["max_pred"], c["max_dist"], c["max_dist"], c["bw"], c["pen_gap"], c["pen_skip"], ic.SLACK, ic.MAX_TL)
    seeded, chained = got[0], got[1]
    ranked = rtb.rank_batch(2, seeded[6], seeded[0], seeded[1], seeded[2], seeded[3], chained[5], chained[6], chained[7], s["max_cand"],
                            *(VARIANT_RANKING[f] for f in ("max_chains", "min_score", "min_cnt", "mask_level")))
    window = lambda *a: itb.locate_window(len(ref), *a, ic.SLACK, ic.MAX_TL)  # noqa: E731
    d = lc.compose(ranked, reads, window, ref, GATK, BAND, ZDROP, False, VARIANT_RANKING["max_chains"])
    return (ref, reads, planted, d) + piled(d, reads, ref)


def assert_planted_truth(ref, planted, sites, read_len=1000):
    """What the sites of the variant set must be, whoever made them (rows of mgl_sw_site's eight fields or textbook Sites): every
    planted SNV a bit-2 site whose alt is the donor's base and whose alt_count is the depth; the deleted positions carry bit 4; the
    position in front of the insertion carries bit 8; and no other site further than one read length from the reference's ends."""
    by_pos = {int(s[0]): tuple(int(v) for v in s) for s in sites}
    expected = set()
    for kind, pos, what in planted:
        if kind == "X":
            s = by_pos.get(pos)
            assert s is not None and s[1] & ptb.SNV, (kind, pos, s)
            assert s[6] == ptb.channel(what[0]) and s[7] == s[2] and s[3] == ptb.channel(ref[pos]), (kind, pos, s)
            expected.add(pos)
        elif kind == "D":
            for p in range(pos, pos + len(what)):
                assert p in by_pos and by_pos[p][1] & ptb.DELETION, (kind, p, by_pos.get(p))
                expected.add(p)
        else:
            assert pos in by_pos and by_pos[pos][1] & ptb.INSERTION, (kind, pos, by_pos.get(pos))
            expected.add(pos)
    others = [p for p in by_pos if p not in expected and read_len <= p < len(ref) - read_len]
    assert not others, others


def result_alignments(res, reads, starts=None, min_mapq=0):
    """an AllMapResult (map_reads_all, map_reads_pileup) -> the textbook's alignments of its counted lines: every line that is not
    secondary and has at least ``min_mapq``; ``starts``: the contigs' first positions where the index has contigs"""
    from mgl_amd import formats

    out = []
    for read, lines in zip(reads, res.lines):
        for ln in lines:
            if ln.flag & 0x100 or ln.mapq < min_mapq or ln.status != 0:
                continue
            q = lc.ltb.revcomp(bytes(read)) if ln.strand else bytes(read)
            out.append((ln.ref_beg + (int(starts[ln.rid]) if starts is not None else 0), q[ln.q_beg:ln.q_end], formats.cigar_text_to_elements(ln.cigar)))
    return out
