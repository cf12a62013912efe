"""Constructed inputs that tests/test_pileup_textbook.py (CPU) and tests/test_gpu_pileup.py (GPU) share.  The alignments are
tests/describe_cases.py's Cases, packed as that module packs them: a case's target lies at byte t_start of the targets' buffer, and
that byte offset is its position.  The tables for the sites entry are made by hand here."""
import numpy as np

import describe_cases as dc
import pileup_textbook as ptb

CANARY = 0x5A5A5A5A
PAD = 16
BAD_ARG = dc.BAD_ARG


def counted(cases, select=None):
    """which cases are counted: no status going in, selected, and passing describe's check"""
    return [not c.status_in and (select is None or select[k] != 0) and not c.want for k, c in enumerate(cases)]


def alignments(cases, t_start, select=None):
    """the textbook's alignments of the counted cases"""
    out = []
    for c, s, on in zip(cases, t_start, counted(cases, select)):
        if on:
            tb, _, qb, qe = c.rec
            out.append((int(s) + tb, c.q[qb:qe], c.cigar))
    return out


def statuses(cases, select=None):
    return [c.status_in or (0 if select is not None and select[k] == 0 else c.want) for k, c in enumerate(cases)]


def expected(cases, t_start, region, select=None, before=None, times=1):
    """What the entry must leave in a table that was ``before`` (zeros) with PAD canary words in front of plane 0 and behind plane 7,
    after ``times`` calls: (uint32 [PAD + 8 * region_len + PAD], status int32 [n + PAD])"""
    beg, length = region
    once = np.asarray(ptb.pileup(alignments(cases, t_start, select), beg, length), np.uint64)
    counts = (once * times + (0 if before is None else np.asarray(before, np.uint64).reshape(8, length))) & ptb.MASK  # (the adds commute)
    pad = np.full(PAD, CANARY, np.uint32)
    table = np.concatenate([pad, counts.astype(np.uint32).reshape(-1), pad])
    return table, np.concatenate([np.asarray(statuses(cases, select), np.int32).reshape(-1), np.full(PAD, CANARY, np.int32)])


# ---- the cases of the pileup entry beyond describe_cases'

def leading_insertions(rng):
    """the first alignment begins with an I at absolute position 0, which is dropped; the second begins with an I whose position lies
    in front of its own target -- the last byte of the first one's --, which is counted; then a trailing I, adjacent I I and D D,
    an I-only and a D-only alignment, an empty one, and bytes 0 and 255 and lower case and N in the query"""
    i, m = dc.seq(rng, 5), dc.seq(rng, 30)
    out = [dc.case(m, i + m + i, [(5, "I"), (30, "M"), (5, "I")]), dc.case(m, i + m + i, [(5, "I"), (30, "M"), (5, "I")])]
    a, b = dc.seq(rng, 10), dc.seq(rng, 10)
    out.append(dc.case(a + b, a + i + b, [(10, "M"), (2, "I"), (3, "I"), (10, "M")]))
    out.append(dc.case(a + i + b, a + b, [(10, "M"), (2, "D"), (3, "D"), (10, "M")]))
    out.append(dc.case(b"", dc.seq(rng, 77), [(77, "I")]))
    out.append(dc.case(dc.seq(rng, 77), b"", [(77, "D")]))
    out.append(dc.case(dc.seq(rng, 9), dc.seq(rng, 9), [], rec=(4, 4, 9, 9)))
    out.append(dc.case(dc.seq(rng, 20), b"ACGTacgtNn\x00\xff-*RYacgT", [(20, "M")]))
    out.append(dc.case(b"", dc.seq(rng, 3), [(3, "I")]))  # the last one: P - 1 is the last byte of the buffer in front of it
    return out


def edge_alignment(rng):
    """one alignment inside longer sequences, 70M 10D 70M 5I 100M, and the target columns at which a region is to begin and to end:
    0, 1, 63, 64, 65 of it, inside the D run, and around the position the I is counted at -> (case, [columns])"""
    a, d, b, i, c = dc.seq(rng, 70), dc.seq(rng, 10), dc.seq(rng, 70), dc.seq(rng, 5), dc.seq(rng, 100)
    case = dc.embedded(rng, a + d + b + c, dc.mutate(rng, a, 0.1) + b + i + c, [(70, "M"), (10, "D"), (70, "M"), (5, "I"), (100, "M")], 33, 21, 7, 3)
    return case, [0, 1, 63, 64, 65, 70, 75, 79, 80, 148, 149, 150, 151, 249, 250]


def stacked(rng, n=300, columns=200):
    """n identical alignments over the same positions (every t_start the same): where a lost add shows -> (cases, t_start)"""
    t = dc.seq(rng, columns)
    q = dc.mutate(rng, t, 0.2)
    q = q[:90] + dc.seq(rng, 4) + q[90:150] + q[160:]
    c = dc.case(t, q, [(90, "M"), (4, "I"), (60, "M"), (10, "D"), (40, "M")])
    return [c] * n, [0] * n


def poisoned(rng):
    """a slot that must not be read between two good alignments: the record and the CIGAR length point far outside"""
    good = lambda: dc.case(*dc.random_alignment(rng, 5, p_mismatch=0.2))  # noqa: E731
    t = dc.seq(rng, 20)
    return [good(), dc.case(t, t, None, slot=b"\xff" * 24, rec=(-9, 1 << 30, 77, -3), cigar_len=1 << 30, want=BAD_ARG), good()]


# ---- tables for the sites entry

SITE_BLOCK = 256
REGION_LENGTHS = (1, 255, 256, 257, 1023, 1024, 1025, 4097, 70001)


def tie_tables():
    """-> (counts [8, L] uint32, ref bytes): every pair of channels 0-5 tied at the top, under every reference channel"""
    cols, ref = [], bytearray()
    for r in b"ACGTN":
        for x in range(6):
            for y in range(x + 1, 6):
                c = [1, 1, 1, 1, 1, 1, 0, 0]
                c[x] = c[y] = 5
                cols.append(c)
                ref.append(r)
        cols.append([3] * 8)   # all tied
        ref.append(r)
    return np.asarray(cols, np.uint32).T.copy(), bytes(ref)


def threshold_tables(min_depth=8, min_alt=3, min_frac=64):
    """each threshold one below and exactly at its edge, for the SNV, the deletion and the insertion bit; a reference byte outside
    ACGT; counts of 2^31 and above -> (counts, ref, (min_depth, min_alt, min_frac))"""
    cols, ref = [], bytearray()

    def put(c, r=ord("A")):
        cols.append(c + [0] * (8 - len(c)))
        ref.append(r)

    for plane in (1, 5, 6):                      # C against a reference A; the deletion; the insertion
        for depth in (min_depth - 1, min_depth):
            for x in (min_alt - 1, min_alt):
                c = [0] * 8
                c[plane] = x
                c[0] = depth - (x if plane != 6 else 0)
                put(c)
        # x * 256 == min_frac * depth exactly, and one less: depth 16, x = 4 (of 64 / 256); depth 17 with the same x misses
        for depth in (16, 17):
            c = [0] * 8
            c[plane] = 4
            c[0] = depth - (4 if plane != 6 else 0)
            put(c)
    for r in (ord("N"), ord("a"), 0, 255, ord("t")):
        put([9, 8, 7, 6, 5, 4, 3, 2], r)
    big = 1 << 31
    put([big, big + 5, 0, 0, 0, 0, 0, 0])
    put([(1 << 32) - 1] * 8, ord("G"))
    put([0, 0, 0, 0, 0, big + 1, big, 7])
    return np.asarray(cols, np.uint64).astype(np.uint32).T.copy(), bytes(ref), (min_depth, min_alt, min_frac)


def region_table(rng, length, kind):
    """a table of ``length`` positions over a random reference.  kind "edges": sites at the first and last position of the region and of
    every block of SITE_BLOCK, and a few between; "none": covered and no site; "all": every position a site -> (counts, ref)"""
    ref = dc.seq(rng, length)
    counts = np.zeros((8, length), np.uint32)
    code = np.searchsorted(np.frombuffer(b"ACGT", np.uint8), np.frombuffer(ref, np.uint8))
    counts[code, np.arange(length)] = 10
    if kind == "none":
        return counts, ref
    at = np.arange(length) if kind == "all" else np.unique(np.concatenate([
        [0, length - 1], np.arange(0, length, SITE_BLOCK), np.arange(SITE_BLOCK - 1, length, SITE_BLOCK), rng.integers(0, length, 1 + length // 97)]))
    what = rng.integers(0, 3, len(at))
    counts[(code[at] + 1) % 4, at] += np.where(what == 0, 6, 0).astype(np.uint32)
    counts[5, at] += np.where(what == 1, 5, 0).astype(np.uint32)
    counts[6, at] += np.where(what == 2, 4, 0).astype(np.uint32)
    counts[7, at] += np.where(what == 2, 9, 0).astype(np.uint32)
    return counts, ref


def sites_textbook(counts, ref, region_beg, params):
    return ptb.sites([list(map(int, row)) for row in counts], ref, region_beg, *params)


def sites_expected(textbook, capacity):
    """``textbook``: sites_textbook's answer -> (call uint8 [L + PAD], flags uint8 [L + PAD], sites int32 [(capacity + PAD) * 8],
    n_sites int64 [1 + PAD]) with canaries behind each and behind the capacity"""
    call, flags, out = textbook
    length = len(call)
    pad = np.full(PAD, CANARY & 0xff, np.uint8)
    rows = np.full((capacity + PAD, 8), CANARY, np.int32)
    kept = out[:capacity]
    if kept:
        rows[:len(kept)] = np.asarray(kept, np.int64).astype(np.int32)
    assert len(call) == len(flags) == length
    total = np.concatenate([np.asarray([len(out)], np.int64), np.full(PAD, CANARY, np.int64)])
    return np.concatenate([np.frombuffer(call, np.uint8), pad]), np.concatenate([np.asarray(flags, np.uint8), pad]), rows.reshape(-1), total
