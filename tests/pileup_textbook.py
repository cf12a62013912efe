"""The textbook of mgl_sw_pileup_alignments_batch_device and mgl_sw_pileup_sites_device: what a batch of
alignments adds up to per position of the reference, and what those counts say per position.  Plain Python, written for clarity; the
kernels are bit for bit these functions.

An alignment is (pos, query_span, cigar): the absolute position of its first target column (t_start + t_beg, a byte offset in the
targets' buffer), the query bytes it spends, and a list of (len, op), op in M / I / D, len >= 1, that spends exactly them.  The target's
bytes are not part of it: the planes take the QUERY's base.  The table is eight planes (lists) of region_len counts, added into modulo
2^32: planes 0-4 the query byte over an M column (A / a, C / c, G / g, T / t, anything else), plane 5 the columns of a D element,
planes 6 and 7 the I elements and their bases, at the position in front of the target cursor."""
from collections import namedtuple

PLANES = 8
DEL, INS, INS_BASES = 5, 6, 7
CALLS = b"ACGTN*"
COVERED, SNV, DELETION, INSERTION = 1, 2, 4, 8
MASK = (1 << 32) - 1
CLIP = (1 << 31) - 1

Site = namedtuple("Site", "pos flags depth ref call call_count alt alt_count")


def channel(byte):
    return {65: 0, 97: 0, 67: 1, 99: 1, 71: 2, 103: 2, 84: 3, 116: 3}.get(byte, 4)


def empty(region_len):
    return [[0] * region_len for _ in range(PLANES)]


def pileup(alignments, region_beg, region_len, counts=None):
    """-> counts, ``counts`` itself where it is given (the batch is added to what stands there)"""
    counts = empty(region_len) if counts is None else counts

    def add(plane, pos, v=1):
        if region_beg <= pos < region_beg + region_len:       # a position outside the region, -1 included, is not counted
            counts[plane][pos - region_beg] = (counts[plane][pos - region_beg] + v) & MASK

    for pos, query, cigar in alignments:
        q, j = bytes(query), 0
        for n, op in cigar:
            if n < 1 or op not in ("M", "I", "D"):
                raise ValueError("not an M / I / D element of at least one base: %r" % ((n, op),))
            if op == "M":
                for c in range(n):
                    add(channel(q[j + c]), pos + c)
                pos, j = pos + n, j + n
            elif op == "D":
                for c in range(n):
                    add(DEL, pos + c)
                pos += n
            else:                                              # behind the position in front of the target cursor
                add(INS, pos - 1)
                add(INS_BASES, pos - 1, n)
                j += n
        if j != len(q):
            raise ValueError("the CIGAR spends %d query bytes of %d" % (j, len(q)))
    return counts


def pileup_by_columns(alignments, region_beg, region_len, counts=None):
    """The same function stated another way, for the tests: every alignment is expanded to columns (element, target position or None,
    query byte or None) first; then the columns are counted -- an M or D column where it stands, the inserted columns of one element
    together at the last target position in front of them (the position in front of the alignment where there is none)."""
    counts = empty(region_len) if counts is None else counts
    for pos, query, cigar in alignments:
        cols, t, j = [], pos, 0
        for e, (n, op) in enumerate(cigar):
            for _ in range(n):
                cols.append((e, t if op != "I" else None, query[j] if op != "D" else None))
                t, j = t + (op != "I"), j + (op != "D")
        assert j == len(query)
        events, last, inserted = [], pos - 1, {}
        for e, t, b in cols:
            if t is None:
                inserted.setdefault(e, [last, 0])[1] += 1
            else:
                events.append((DEL if b is None else channel(b), t, 1))
                last = t
        for at, n in inserted.values():
            events += [(INS, at, 1), (INS_BASES, at, n)]
        for plane, at, v in events:
            if region_beg <= at < region_beg + region_len:
                counts[plane][at - region_beg] = (counts[plane][at - region_beg] + v) & MASK
    return counts


def site(counts, i, ref_byte, min_depth, min_alt, min_frac):
    """position i of the table -> Site with pos = i and nothing clipped"""
    c = [counts[p][i] for p in range(PLANES)]
    depth = sum(c[:6])
    ref = channel(ref_byte)
    call = max(range(6), key=lambda k: (c[k], -k))             # the largest count, the lowest channel of a tie
    others = [k for k in range(5) if k != ref]
    alt = max(others, key=lambda k: (c[k], -k))
    alt, alt_count = (alt, c[alt]) if c[alt] > 0 else (-1, 0)
    ok = lambda x: x >= min_alt and x * 256 >= min_frac * depth  # noqa: E731
    flags = 0
    if depth >= min_depth:
        flags = COVERED | (SNV if ok(alt_count) else 0) | (DELETION if ok(c[DEL]) else 0) | (INSERTION if ok(c[INS]) else 0)
    return Site(i, flags, depth, ref, call, c[call], alt, alt_count)


def sites(counts, ref, region_beg, min_depth, min_alt, min_frac):
    """``ref``: the targets' buffer the positions are offsets of.  -> (call: bytes, one per position; flags: a list; the sites: the
    positions with flags & 14 in position order, depth and the two counts clipped to 2^31 - 1)"""
    if min_depth < 1 or min_alt < 1 or not 1 <= min_frac <= 256:
        raise ValueError("min_depth or min_alt < 1, or min_frac outside 1 .. 256")
    call, flags, out = bytearray(), [], []
    for i in range(len(counts[0])):
        s = site(counts, i, ref[region_beg + i], min_depth, min_alt, min_frac)
        call.append(CALLS[s.call] if s.flags & COVERED else ord("N"))
        flags.append(s.flags)
        if s.flags & (SNV | DELETION | INSERTION):
            out.append(s._replace(depth=min(s.depth, CLIP), call_count=min(s.call_count, CLIP), alt_count=min(s.alt_count, CLIP)))
    return bytes(call), flags, out
