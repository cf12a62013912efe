"""Constructed inputs that tests/test_calls_textbook.py (CPU), tests/test_gpu_insertions.py and tests/test_gpu_genotype.py (GPU) share.
The alignments are tests/describe_cases.py's Cases, packed as that module packs them, with hand-made site lists; the tables for the
genotype entry are made by hand here, with no alignment behind them."""
from collections import namedtuple

import numpy as np

import calls_textbook as ctb
import describe_cases as dc
import pileup_cases as pc
import pileup_textbook as ptb

CANARY, PAD = pc.CANARY, pc.PAD
Q20 = (11, 778, 6341)        # genotype_costs(20) in the entry's order: cost_match, cost_het, cost_error


def site(pos, flags=ptb.COVERED | ptb.INSERTION, alt=-1):
    """a site record as the entries read it: pos, flags and alt; the other fields are not read and say so"""
    return ptb.Site(pos, flags, 777, 4, 5, 666, alt, 555)


def site_rows(sites, capacity=None):
    """-> int32 [capacity, 8]; the rows behind the sites are poison: positions that would match everything"""
    rows = np.full((len(sites) if capacity is None else capacity, 8), 0x7f7f7f7f, np.int32)
    if sites:
        rows[:len(sites)] = np.asarray(sites, np.int64).astype(np.int32)
    return rows


# ---- the insertions entry

SITE_LIST_SIZES = (0, 1, 2, 63, 64, 65, 1000)
FIRST, MIDDLE, LAST, NO_SITE = 9, 999, 1999, 1499      # the positions the four insertions of site_list_case stand behind


def site_list_case(rng, k):
    """one alignment with four insertions -- behind the first, a middle and the last site of a list of k sites, and behind a position
    that is no site -- -> (cases, [site])"""
    parts = [(10, "M"), (3, "I"), (990, "M"), (2, "I"), (500, "M"), (1, "I"), (500, "M"), (4, "I"), (30, "M")]
    t = dc.seq(rng, sum(n for n, op in parts if op == "M"))
    q, at = b"", 0
    for n, op in parts:
        if op == "M":
            q, at = q + dc.mutate(rng, t[at:at + n], 0.1), at + n
        else:
            q += dc.seq(rng, n)
    pos = {FIRST, LAST, MIDDLE}
    pos = set(sorted(pos)[:k]) if k < 3 else pos
    if k == 2:
        pos = {FIRST, LAST}
    free = [p for p in range(FIRST + 1, LAST) if p not in (MIDDLE, NO_SITE)]
    pos |= set(int(p) for p in rng.choice(free, max(k - len(pos), 0), replace=False))
    assert len(pos) == k and NO_SITE not in pos
    return [dc.case(t, q, parts)], [site(p, int(rng.integers(0, 16))) for p in sorted(pos)]


def length_cases(rng, max_ins):
    """insertions of 1, max_ins and max_ins + 1 bases (and, for the columns, of every length between where max_ins is small), each
    behind a site of its own, and two of different lengths behind one"""
    lens = sorted({1, max_ins, max_ins + 1, min(2, max_ins), max(max_ins - 1, 1)})
    parts = [(20, "M")]
    for n in lens + [1, max_ins]:
        parts += [(n, "I"), (20, "M")]
    cases = []
    for _ in range(3):
        t = dc.seq(rng, sum(n for n, op in parts if op == "M"))
        q, at = b"", 0
        for n, op in parts:
            q, at = (q + t[at:at + n], at + n) if op == "M" else (q + dc.seq(rng, n, b"ACGTN"), at)
        cases.append(dc.case(t, q, parts))
    # the three alignments lie end to end; the sites are the positions of the first one's insertions, and of the third one's first
    first = [19 + 20 * k for k in range(len(lens) + 2)]
    return cases, [site(p) for p in first] + [site(2 * len(cases[0].t) + 19)]


def seam_case(rng, binary):
    """a CIGAR of 1 100 elements, M and D in turn, whose elements 62 .. 66 and 510 .. 514 are insertions: the lanes' seam of a parse
    step and DESCRIBE_CHUNK's seam -> (cases, sites: every position)"""
    parts = [(2, "M") if k % 2 == 0 else (1, "D") for k in range(1100)]
    for k, n in zip(list(range(62, 67)) + list(range(510, 515)), (1, 2, 3, 1, 2, 3, 2, 1, 3, 2)):
        parts[k] = (n, "I")
    t = dc.seq(rng, sum(n for n, op in parts if op != "I"))
    q, at = b"", 0
    for n, op in parts:
        if op == "M":
            q += t[at:at + n]
        elif op == "I":
            q += dc.seq(rng, n)
        at += n if op != "I" else 0
    return [dc.case(t, q, parts)], [site(p) for p in range(len(t))]


def odd_bytes_case():
    """lower case, N and bytes that are no base at all inside an insertion"""
    ins = b"acgtNn\x00\xffRY-*ACGT"
    t = b"ACGTACGTACGTACGTACGT"
    return [dc.case(t, t[:10] + ins + t[10:], [(10, "M"), (len(ins), "I"), (10, "M")])], [site(9)]


def insertions_expected(cases, t_start, region_beg, sites, n_sites, capacity, max_ins, select=None, before=None, times=1):
    """What the entry must leave in a table of ``capacity`` rows that was ``before`` (zeros) between PAD canary words after ``times``
    calls: (uint32 [PAD + capacity * W + PAD], status int32 [n + PAD])"""
    active = sites[:min(max(n_sites, 0), capacity)]
    once = np.zeros((capacity, ctb.width(max_ins)), np.uint64)
    if active:
        once[:len(active)] = np.asarray(ctb.insertions(pc.alignments(cases, t_start, select), region_beg, active, max_ins), np.uint64)
    table = (once * times + (0 if before is None else np.asarray(before, np.uint64).reshape(once.shape))) & ptb.MASK
    pad = np.full(PAD, CANARY, np.uint32)
    return (np.concatenate([pad, table.astype(np.uint32).reshape(-1), pad]),
            np.concatenate([np.asarray(pc.statuses(cases, select), np.int32).reshape(-1), np.full(PAD, CANARY, np.int32)]))


# ---- tables for the genotype entry

Table = namedtuple("Table", "counts ref sites n_sites ins max_ins max_del costs")


def table(entries, length=None, max_ins=4, max_del=8, costs=Q20, n_sites=None, with_ins=True, ref_fill=b"A"):
    """entries: dicts in position order -- pos, c (up to eight counts), ref (a byte), flags, alt, ins ({word: count}) -> Table with one
    site per entry.  Positions without an entry hold depth 10 of the reference base."""
    length = max(e["pos"] for e in entries) + 2 if length is None else length
    ref = bytearray(ref_fill * length)
    counts = np.zeros((8, length), np.uint64)
    counts[0] = 10
    sites, rows = [], []
    for e in entries:
        c = list(e.get("c", [10])) + [0] * 8
        if e["pos"] < length:                                  # (a site outside the table has nothing in it)
            counts[:, e["pos"]] = c[:8]
            ref[e["pos"]] = e.get("ref", ord("A"))
        sites.append(site(e["pos"], e.get("flags", ptb.COVERED), e.get("alt", -1)))
        row = [0] * ctb.width(max_ins)
        for word, n in e.get("ins", {}).items():
            row[word] = n
        rows.append(row)
    return Table([[int(v) for v in plane] for plane in counts], bytes(ref), sites, len(sites) if n_sites is None else n_sites, rows if with_ins else None,
                 max_ins, max_del, costs)


def col(max_ins, j, ch):
    return max_ins + 1 + 5 * j + ch


SNV_F, DEL_F, INS_F = ptb.COVERED | ptb.SNV, ptb.COVERED | ptb.DELETION, ptb.COVERED | ptb.INSERTION


def kinds_table():
    """each kind alone, a position with all three, a site alt of 4, an N reference (no SNV call, but a deletion call), a site with no
    bit set, an SNV bit without an alt, and a site outside the table"""
    m = 4
    two = {2: 9, col(m, 0, 1): 9, col(m, 1, 3): 9}
    return table([
        dict(pos=3, c=[8, 8], flags=SNV_F, alt=1),
        dict(pos=7, c=[8, 0, 0, 0, 0, 8], flags=DEL_F),
        dict(pos=11, c=[16, 0, 0, 0, 0, 0, 9, 18], flags=INS_F, ins=two),
        dict(pos=15, c=[2, 0, 6, 0, 0, 8, 7, 14], ref=ord("a"), flags=SNV_F | 12, alt=2, ins={2: 7, col(m, 0, 0): 7, col(m, 1, 4): 7}),
        dict(pos=19, c=[8, 0, 0, 0, 8], flags=SNV_F, alt=4),
        dict(pos=23, c=[1, 1, 8, 1, 5, 7], ref=ord("N"), flags=SNV_F | 4, alt=2),
        dict(pos=27, c=[8, 8], flags=ptb.COVERED, alt=1),
        dict(pos=31, c=[8, 8], flags=SNV_F, alt=-1),
        dict(pos=35, c=[8, 0, 0, 8], ref=ord("t"), flags=SNV_F, alt=0),
        dict(pos=1 << 20, flags=SNV_F | 12, alt=1, ins=two),
    ], length=40, max_ins=m)


def runs_table(max_del=5):
    """deletion runs of 1, 2, max_del and max_del + 1 (flag 1, one call), of 2 * max_del + 1, a run broken by a gap in the positions, one
    broken by a site without the bit, and one cut by n_sites: the records behind the active sites go on with it"""
    entries, at = [], 2
    for n in (1, 2, max_del, max_del + 1, 2 * max_del + 1):
        entries += [dict(pos=at + k, c=[4 + k, 0, 0, 0, 0, 12 - k], flags=DEL_F) for k in range(n)]
        at += n + 2
    entries += [dict(pos=at + k, c=[4, 0, 0, 0, 0, 12], flags=DEL_F) for k in (0, 1, 3, 4)]                       # a gap at at + 2
    at += 7
    entries += [dict(pos=at + k, c=[4, 4, 0, 0, 0, 8], flags=DEL_F if k != 2 else SNV_F, alt=1) for k in range(5)]  # site at + 2 has no bit 4
    at += 7
    entries += [dict(pos=at + k, c=[4, 0, 0, 0, 0, 12], flags=DEL_F) for k in range(4)]
    t = table(entries, max_del=max_del)
    return t._replace(n_sites=len(entries) - 2)                                                                   # the last run is cut at 2


def block_seam_table():
    """600 sites, a deletion run over sites 250 .. 260 (the kernels' blocks meet at 255 | 256), all three kinds at site 255 and at 256"""
    m = 4
    entries = []
    for s in range(600):
        e = dict(pos=2 * s if s < 250 else 500 + (s - 250) if s <= 260 else 2 * s, c=[6, 5, 0, 0, 0, 0], flags=SNV_F, alt=1)
        if 250 <= s <= 260:
            e.update(c=[6, 5, 0, 0, 0, 5], flags=SNV_F | 4)
        if s in (255, 256, 599):
            e.update(c=[6, 5, 0, 0, 0, 5, 3, 3], flags=e["flags"] | 8, ins={1: 3, col(m, 0, 2): 3})
        entries.append(e)
    return table(entries, max_ins=m, max_del=64)


def insertion_ties_table():
    """the modal length on a tie (the smallest wins), the largest word not the first, only word 0 set (no call), a column's plurality
    on a tie (the lowest channel wins) and on every channel, a word above 2^31, and max_ins columns"""
    m = 4
    return table([
        dict(pos=2, c=[16, 0, 0, 0, 0, 0, 10, 30], flags=INS_F, ins={2: 5, 3: 5, col(m, 0, 1): 5, col(m, 0, 2): 5, col(m, 1, 3): 10, col(m, 2, 0): 5}),
        dict(pos=4, c=[16, 0, 0, 0, 0, 0, 10, 30], flags=INS_F, ins={1: 2, 3: 7, 4: 1, col(m, 0, 4): 4, col(m, 0, 3): 4, col(m, 1, 2): 9, col(m, 2, 1): 8}),
        dict(pos=6, c=[16, 0, 0, 0, 0, 0, 10, 990], flags=INS_F, ins={0: 10}),
        dict(pos=8, c=[16, 0, 0, 0, 0, 0, 10, 40], flags=INS_F, ins={4: 10, **{col(m, j, ch): 3 for j in range(4) for ch in range(5)}}),
        dict(pos=10, c=[3, 0, 0, 0, 0, 0, 1 << 31, 0], flags=INS_F, ins={1: (1 << 32) - 1, col(m, 0, 0): 1}),
        dict(pos=12, c=[16, 0, 0, 0, 0, 0, 20, 40], flags=INS_F, ins={0: 11, 2: 9, col(m, 0, 0): 1, col(m, 0, 4): 2, col(m, 1, 3): 2, col(m, 1, 4): 2}),
        dict(pos=14, c=[16, 0, 0, 0, 0, 0, 20, 40], flags=ptb.COVERED, ins={2: 9}),                              # rows and no bit 8: no call
    ], max_ins=m)


# r, a, costs -> (gt, (PL0, PL1, PL2), gq), worked by hand (tests/test_calls_textbook.py says how)
GENOTYPES = [
    (8, 8, Q20, 1, (150, 0, 150), 99),
    (0, 16, Q20, 2, (396, 48, 0), 48),
    (16, 0, Q20, 0, (0, 48, 396), 48),
    (1, 1, (1, 2, 3), 0, (0, 0, 0), 0),                       # L0 == L1 == L2: the lowest genotype
    (3, 1, (1, 2, 3), 0, (0, 0, 0), 0),                       # L0 = 6, L1 = 8, L2 = 10: differences below half a phred
    ((1 << 32) - 1, 0, (1, (1 << 20) - 1, 1 << 20), 0, (0, (1 << 31) - 1, (1 << 31) - 1), 99),
    (0, (1 << 32) - 1, (1, 2, 1 << 20), 2, ((1 << 31) - 1, 1 << 24, 0), 99),
    ((1 << 32) - 1, (1 << 32) - 1, (1 << 18, 1 << 19, 1 << 20), 1, ((1 << 31) - 1, 0, (1 << 31) - 1), 99),
    (98, 0, (1, 257, 1000), 0, (0, 98, 382), 98),
    (99, 0, (1, 257, 1000), 0, (0, 99, 386), 99),
    (100, 0, (1, 257, 1000), 0, (0, 100, 390), 99),
]


def genotype_tables():
    """GENOTYPES as SNV sites, one table per set of costs -> [(Table, [the rows of GENOTYPES in it])]"""
    out = []
    for costs in sorted({g[2] for g in GENOTYPES}):
        rows = [g for g in GENOTYPES if g[2] == costs]
        out.append((table([dict(pos=2 * k + 1, c=[g[0], 0, 0, g[1]], flags=SNV_F, alt=3) for k, g in enumerate(rows)], costs=costs), rows))
    return out


def calls_textbook(t, n_sites=None):
    n = t.n_sites if n_sites is None else n_sites
    active = t.sites[:min(max(n, 0), len(t.sites))]
    return ctb.calls(t.counts, t.ref, 0, active, t.ins, t.max_ins, t.max_del, t.costs)


def calls_expected(textbook, capacity, max_ins, seq=True):
    """``textbook``: calls_textbook's answer -> (calls int32 [(capacity + PAD) * 16], n_calls int64 [1 + PAD], seq uint8 [(capacity + PAD)
    * max_ins]) with canaries behind the capacity"""
    calls, rows = textbook
    out = np.full((capacity + PAD, 16), CANARY, np.int32)
    kept = calls[:capacity]
    if kept:
        out[:len(kept)] = np.asarray(kept, np.int64).astype(np.int32)
    sq = np.full((capacity + PAD, max_ins), CANARY & 0xff, np.uint8)
    for k, r in enumerate(rows[:capacity]):
        sq[k] = np.frombuffer(r, np.uint8)
    total = np.concatenate([np.asarray([len(calls)], np.int64), np.full(PAD, CANARY, np.int64)])
    return out.reshape(-1), total, sq.reshape(-1) if seq else None
