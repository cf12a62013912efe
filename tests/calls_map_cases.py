"""The pipeline's inputs for the calls (tests/test_calls_pipeline.py on the CPU, tests/test_gpu_map_reads_calls.py on the GPU):
pileup_map_cases' composition of the CPU textbooks, extended by the insertions and genotype textbooks, over
synth.diploid_variant_set -- two haplotypes with planted substitutions, a deletion and an insertion, heterozygous at every other
index, tiled by exact reads -- and over the haploid synth.variant_mapping_set; the planted truth as both tests assert it; and the VCF
round trip that rebuilds the haplotypes."""
import functools

import calls_textbook as ctb
import lines_cases as lc
import pileup_map_cases as pm

MAX_INS, MAX_DEL, ERROR_PHRED = 16, 64, 20
SETS = ("even", "odd", "haploid")


@functools.lru_cache(maxsize=None)
def variant_set(which):
    """-> (ref, reads, planted, zygosity): the diploid set with its heterozygous variants at the even or odd indices, or the haploid
    set, where everything is homozygous"""
    from mgl_amd import synth

    if which == "haploid":
        return pm.variant_set() + ([2] * len(pm.variant_set()[2]),)
    return synth.diploid_variant_set(pm.VARIANT_SEED, which)


def depth_of(which):
    return 8 if which == "haploid" else 16                    # a read every 125 bases, 1 000 long, of each haplotype


@functools.lru_cache(maxsize=None)
def composed(which):
    """pileup_map_cases.variant_piled's composition over variant_set(which) -> (ref, reads, compose's dict, counts, the sites
    textbook's tuple)"""
    import index_cases as ic
    import index_textbook as itb
    import rank_cases as rc
    import rank_textbook as rtb

    if which == "haploid":
        ref, reads, _, d, counts, found = pm.variant_piled()
        return ref, reads, d, counts, found
    ref, reads, _, _ = variant_set(which)
    c, s = ic.CHAINING, ic.SEEDING
    got = itb.map_reads(itb.build_index(ref, rc.K, rc.W), len(ref), reads, rc.K, rc.W, 2, s["max_occ"], s["max_occ_ref"], s["merge"], s["max_cand"],
                        2 * len(reads) * s["max_cand"], c["max_pred"], c["max_dist"], c["max_dist"], c["bw"], c["pen_gap"], c["pen_skip"], ic.SLACK, ic.MAX_TL)
    seeded, chained = got[0], got[1]
    ranked = rtb.rank_batch(2, seeded[6], seeded[0], seeded[1], seeded[2], seeded[3], chained[5], chained[6], chained[7], s["max_cand"],
                            *(pm.VARIANT_RANKING[f] for f in ("max_chains", "min_score", "min_cnt", "mask_level")))
    window = lambda *a: itb.locate_window(len(ref), *a, ic.SLACK, ic.MAX_TL)  # noqa: E731
    d = lc.compose(ranked, reads, window, ref, pm.GATK, pm.BAND, pm.ZDROP, False, pm.VARIANT_RANKING["max_chains"])
    return (ref, reads, d) + pm.piled(d, reads, ref)


def called(alignments, counts, sites, ref):
    """the insertions and genotype textbooks behind a table and its sites -> (ins, calls, rows)"""
    ins = ctb.insertions(alignments, 0, sites, MAX_INS)
    calls, rows = ctb.calls(counts, ref, 0, sites, ins, MAX_INS, MAX_DEL, ctb.genotype_costs(ERROR_PHRED))
    return ins, calls, rows


@functools.lru_cache(maxsize=None)
def composed_calls(which):
    """-> (ref, reads, planted, zygosity, compose's dict, counts, sites, ins, calls, rows)"""
    ref, reads, d, counts, (_, _, sites) = composed(which)
    _, _, planted, zygosity = variant_set(which)
    return (ref, reads, planted, zygosity, d, counts, sites) + called(pm.alignments(d, reads), counts, sites, ref)


def assert_planted_calls(ref, planted, zygosity, calls, depth, read_len=1000):
    """What the calls of a variant set must be, whoever made them (``calls``: smithwaterman.Call, REF / ALT as bytes): every planted
    variant exactly one call with its kind, position, length, alleles, the full depth, and gt 1 where it is heterozygous and 2 where
    it is homozygous; and no other call further than one read length from the reference's ends."""
    expected = set()
    for (kind, pos, what), z in zip(planted, zygosity):
        want = {"X": (ctb.SNV, 1, bytes(ref[pos:pos + 1]), what), "D": (ctb.DELETION, len(what), what, b""), "I": (ctb.INSERTION, len(what), b"", what)}[kind]
        hits = [c for c in calls if c.pos == pos and c.kind == want[0]]
        assert len(hits) == 1, (kind, pos, hits)
        c = hits[0]
        assert (c.kind, c.len, c.ref, c.alt) == want and c.depth == depth and c.gt == z and c.flags == 0, (kind, pos, z, c)
        assert c.ref_count + c.alt_count == depth and c.alt_count == (depth if z == 2 else depth // 2), c
        expected.add((pos, want[0]))
    others = [c for c in calls if (c.pos, c.kind) not in expected and read_len <= c.pos < len(ref) - read_len]
    assert not others, others


def host_calls(calls, rows, ref):
    """the textbook's calls and rows -> smithwaterman.Call, as map_reads_calls builds them"""
    from mgl_amd import smithwaterman as sw

    return [sw.make_call(c, r, ref) for c, r in zip(calls, rows)]


def apply_records(ref, records, keep):
    """the reference with the VCF records ``keep`` picks applied, from the last to the first -> a haplotype"""
    hap = bytearray(ref)
    for r in sorted((r for r in records if keep(r)), key=lambda r: -r.pos):
        assert bytes(hap[r.pos:r.pos + len(r.ref)]) == r.ref, r
        hap[r.pos:r.pos + len(r.ref)] = r.alt
    return bytes(hap)


def assert_vcf_rebuilds_the_haplotypes(path, ref, planted, zygosity, calls):
    """write_vcf then read_vcf: the records are the calls with a genotype, applying the gt >= 1 records rebuilds haplotype A, applying
    the 1/1 records haplotype B"""
    from mgl_amd import formats, synth

    written = formats.write_vcf(path, "chr", len(ref), ref, calls)
    header, records = formats.read_vcf(path)
    assert header[0] == "##fileformat=VCFv4.2" and "##contig=<ID=chr,length=%d>" % len(ref) in header
    assert header[-1].split("\t") == ["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT", "sample"]
    kept = [c for c in calls if c.gt >= 1]
    assert written == len(records) == len(kept) and [r.pos for r in records] == sorted(r.pos for r in records)
    for r in records:
        c = [c for c in kept if c.pos - (c.kind == ctb.DELETION) == r.pos][0]
        assert r.chrom == "chr" and r.filter == "PASS" and r.gt == ("0/1" if c.gt == 1 else "1/1"), (r, c)
        assert (r.qual, r.gq, r.dp, r.ad, r.pl) == (c.qual, c.gq, c.depth, (c.ref_count, c.alt_count), c.pl), (r, c)
        assert len(r.ref) >= 1 and len(r.alt) >= 1 and (c.kind == ctb.SNV or r.ref[0] == r.alt[0] == ref[r.pos]), r   # anchored in front
    hap_a = synth.apply_variants(ref, planted)
    hap_b = synth.apply_variants(ref, [v for v, z in zip(planted, zygosity) if z == 2])
    assert apply_records(ref, records, lambda r: True) == hap_a
    assert apply_records(ref, records, lambda r: r.gt == "1/1") == hap_b
    return records
