"""The textbook of mgl_sw_pileup_insertions_batch_device and mgl_sw_genotype_sites_device: what the insertions
behind the candidate sites are, and what the pileup's planes and those rows say per site -- events, genotypes, qualities.  Plain
Python in integers, written for clarity, over pileup_textbook's tables; the kernels are bit for bit these functions.

An alignment is pileup_textbook's (pos, query_span, cigar).  ``sites`` are the ACTIVE sites: the first min(max(n_sites, 0), capacity)
records, pileup_textbook.Site or rows of mgl_sw_site's eight fields.  The insertion table is one row per site of W = 6 * max_ins + 1
counts, added into modulo 2^32: word 0 the insertions longer than max_ins, word L those of exactly L bases, word
max_ins + 1 + 5 * j + ch channel ch in column j of the insertions of at most max_ins bases."""
import math
from collections import namedtuple

import pileup_textbook as ptb

SNV, DELETION, INSERTION = 1, 2, 3          # a call's kind
LONG_DEL = 1                                # a call's flag: the deletion run was cut at max_del
MASK, CLIP = ptb.MASK, ptb.CLIP
BASES = b"ACGTN"

Call = namedtuple("Call", "pos kind len ref alt depth ref_count alt_count gt gq qual pl0 pl1 pl2 flags reserved")


def genotype_costs(error_phred=20):
    """the wrappers' function, shared: -> ``costs`` as every function here takes them, in the entry's order (cost_match, cost_het,
    cost_error)"""
    from mgl_amd import smithwaterman

    c = smithwaterman.genotype_costs(error_phred)
    return c.cost_match, c.cost_het, c.cost_error


def width(max_ins):
    return 6 * max_ins + 1


def empty(n_rows, max_ins):
    return [[0] * width(max_ins) for _ in range(n_rows)]


def insertions(alignments, region_beg, sites, max_ins, table=None):
    """-> the table, ``table`` itself where it is given (the batch is added to what stands there; it has at least len(sites) rows)"""
    if not 1 <= max_ins <= 64:
        raise ValueError("max_ins outside 1 .. 64")
    table = empty(len(sites), max_ins) if table is None else table
    row_of = {}
    for s, site in enumerate(sites):
        row_of.setdefault(int(site[0]), s)                     # (strictly ascending as the sites entry writes them: no position twice)

    def add(row, word):
        row[word] = (row[word] + 1) & MASK

    for pos, query, cigar in alignments:
        q, j = bytes(query), 0
        for n, op in cigar:
            if op == "M":
                pos, j = pos + n, j + n
            elif op == "D":
                pos += n
            else:                                              # behind the position in front of the target cursor: the pileup's rule
                s = row_of.get(pos - 1 - region_beg)
                if s is not None and n > max_ins:
                    add(table[s], 0)
                elif s is not None:
                    add(table[s], n)
                    for col in range(n):
                        add(table[s], max_ins + 1 + 5 * col + ptb.channel(q[j + col]))
                j += n
    return table


def genotype(r, a, costs):
    """-> (gt, gq, qual, (pl0, pl1, pl2)) of r reads for the reference and a for the other allele"""
    cost_match, cost_het, cost_error = costs
    lik = (r * cost_match + a * cost_error, (r + a) * cost_het, a * cost_match + r * cost_error)
    m = min(lik)
    pl = tuple(min((x - m + 128) >> 8, CLIP) for x in lik)
    gt = lik.index(m)                                          # the lowest g with Lg == m
    return gt, min(99, min(pl[g] for g in range(3) if g != gt)), pl[0], pl


def check(max_ins, max_del, costs):
    if not 1 <= max_ins <= 64 or not 1 <= max_del <= 4096:
        raise ValueError("max_ins outside 1 .. 64 or max_del outside 1 .. 4096")
    if not all(1 <= c <= 1 << 20 for c in costs) or not costs[0] < costs[1] < costs[2]:
        raise ValueError("a cost outside 1 .. 2^20, or not cost_match < cost_het < cost_error")


def calls(counts, ref, region_beg, sites, ins, max_ins, max_del, costs):
    """``counts``: the pileup's planes; ``ref``: the targets' buffer the positions are offsets of; ``ins``: insertions' table or None
    -> (the calls in site order, inside a site SNV, deletion, insertion; their sequence rows: max_ins bytes each)"""
    check(max_ins, max_del, costs)
    region_len = len(counts[0])
    out, rows = [], []
    pos_of = [int(s[0]) for s in sites]
    flags_of = [int(s[1]) for s in sites]

    def deleted(k, at):
        return 0 <= k < len(sites) and flags_of[k] & ptb.DELETION and pos_of[k] == at

    def emit(pos, kind, n, ref_ch, alt, depth, r, a, flags=0, row=b""):
        gt, gq, qual, pl = genotype(r, a, costs)
        out.append(Call(pos, kind, n, ref_ch, alt, min(depth, CLIP), min(r, CLIP), min(a, CLIP), gt, gq, qual, pl[0], pl[1], pl[2], flags, 0))
        rows.append(row + bytes(max_ins - len(row)))

    for s, site in enumerate(sites):
        pos, flags, alt = pos_of[s], flags_of[s], int(site[6])
        if not 0 <= pos < region_len:                          # a site outside the table has no event
            continue
        c = [counts[p][pos] for p in range(ptb.PLANES)]
        depth = sum(c[:6])
        ref_ch = ptb.channel(ref[region_beg + pos])
        if flags & ptb.SNV and ref_ch <= 3 and 0 <= alt <= 3:
            emit(pos, SNV, 1, ref_ch, alt, depth, c[ref_ch], c[alt])
        if flags & ptb.DELETION and not deleted(s - 1, pos - 1):
            n = 1
            while n < max_del and deleted(s + n, pos + n):
                n += 1
            emit(pos, DELETION, n, ref_ch, -1, depth, c[ref_ch], c[ptb.DEL], LONG_DEL if deleted(s + n, pos + n) else 0)
        if flags & ptb.INSERTION and ins is not None and any(ins[s][1:max_ins + 1]):
            n = max(range(1, max_ins + 1), key=lambda k: (ins[s][k], -k))      # the largest word, the smallest length of a tie
            cols = ins[s][max_ins + 1:]
            row = bytes(BASES[max(range(5), key=lambda ch: (cols[5 * j + ch], -ch))] for j in range(n))
            emit(pos, INSERTION, n, ref_ch, -1, depth, max(depth - c[ptb.INS], 0), ins[s][n], 0, row)
    return out, rows


def alleles(call, row, ref, region_beg=0):
    """-> (REF, ALT) of a call as the bases it changes: one base each for an SNV, the deleted bases and nothing, nothing and the
    inserted bases (which stand BEHIND position pos)"""
    at = region_beg + call.pos
    if call.kind == SNV:
        return bytes(ref[at:at + 1]), BASES[call.alt:call.alt + 1]
    if call.kind == DELETION:
        return bytes(ref[at:at + call.len]), b""
    return b"", bytes(row[:call.len])


def phred_costs(error_phred):
    """genotype_costs stated a second way, for the tests: natural logarithms, one expression per genotype's per-read probability"""
    e = math.exp(-error_phred * math.log(10) / 10)
    cost = lambda p: -2560 * math.log(p) / math.log(10)  # noqa: E731
    return max(1, round(cost(1 - e))), round(cost(0.5 * (1 - e) + 0.5 * e / 3)), round(cost(e / 3))
