"""Seeded synthetic read batches (the bench / fixture workloads of SURVEY.md section 8d).

Everything is numpy-vectorised so a 10 M-pair batch can be produced in seconds;
the generators are deterministic in (seed, arguments).
"""
import numpy as np

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


def rng_for(seed):
    return np.random.Generator(np.random.MT19937(seed))


def random_genome(rng, n):
    """n uniform-random ACGT bases as a uint8 array."""
    return BASES[rng.integers(0, 4, size=n, dtype=np.uint8)]


def illumina_reads(rng, genome, starts, read_len=150, sub=0.01, ins=0.001, dele=0.001):
    """Fixed-length reads copied from ``genome`` at ``starts`` with per-base errors.

    For output base k of a read: with probability ``ins`` it is a random inserted
    base (consumes no genome base); otherwise it copies the next genome base,
    after skipping one genome base with probability ``dele``, and is substituted
    by a different base with probability ``sub``.  Returns uint8 [n, read_len].
    """
    n = len(starts)
    is_ins = rng.random((n, read_len)) < ins
    is_del = rng.random((n, read_len)) < dele
    is_sub = rng.random((n, read_len)) < sub
    copied = ~is_ins
    # genome index for each copied base: start + #copied-before + #deleted-up-to-here
    src = np.cumsum(copied, axis=1) - copied + np.cumsum(is_del & copied, axis=1)
    src = src + np.asarray(starts, dtype=np.int64)[:, None]
    np.clip(src, 0, len(genome) - 1, out=src)
    reads = genome[src]
    code = np.searchsorted(BASES, reads).astype(np.uint8)  # A,C,G,T -> 0..3 (BASES is sorted)
    shift = rng.integers(1, 4, size=(n, read_len), dtype=np.uint8)
    code = np.where(is_sub, (code + shift) & 3, code)
    rnd = rng.integers(0, 4, size=(n, read_len), dtype=np.uint8)
    code = np.where(is_ins, rnd, code)
    return BASES[code]


def config1(seed=42, n_reads=1000, ref_len=1000, read_len=150):
    """BASELINE.json configs[0]: n_reads 150 bp reads, each against the full 1 kb reference."""
    rng = rng_for(seed)
    ref = random_genome(rng, ref_len)
    starts = rng.integers(0, ref_len - read_len + 1, size=n_reads)
    # keep room for a few deletions at the right edge
    starts = np.minimum(starts, ref_len - read_len - 8)
    reads = illumina_reads(rng, ref, starts, read_len)
    return ref, reads


def window_batch(seed, n_pairs, window=256, read_len=150, genome_len=1 << 24):
    """BASELINE.json configs[1]: per-pair target window of ``window`` bases cut from a random
    genome, read = read_len-bp copy starting U[0, window-read_len-8] into the window, Illumina errors.

    Returns (genome uint8[genome_len], win_start int64[n], reads uint8[n, read_len]).
    """
    rng = rng_for(seed)
    genome = random_genome(rng, genome_len)
    win_start = rng.integers(0, genome_len - window, size=n_pairs, dtype=np.int64)
    inner = rng.integers(0, window - read_len - 8 + 1, size=n_pairs, dtype=np.int64)
    reads = illumina_reads(rng, genome, win_start + inner, read_len)
    return genome, win_start, reads


def ont_pair(rng, length, sub=0.05, ins=0.05, dele=0.05):
    """One ONT-style pair: random target of ``length`` and a noisy copy (variable length)."""
    t = random_genome(rng, length)
    out = []
    code_t = np.searchsorted(BASES, t)
    r = rng.random((length, 3))
    extra = rng.integers(0, 4, size=length)
    shift = rng.integers(1, 4, size=length)
    for k in range(length):
        if r[k, 0] < ins:
            out.append(extra[k])
        if r[k, 1] < dele:
            continue
        c = code_t[k]
        if r[k, 2] < sub:
            c = (c + shift[k]) & 3
        out.append(c)
    q = BASES[np.asarray(out, dtype=np.int64)]
    return t, q


def chain_flank(rng, length, every=200, anchor=20, jumps=5, jump=30):
    """One flank of a long-read pair with known anchors (DESIGN.md section 9f's pairs): a random target of ``length`` and a noisy copy
    -- 5 % substitutions, 1 % + 1 % indels of 1 .. 3 bases, ``jumps`` insertions of ``jump`` bases -- in which about every ``every``
    target bases ``anchor`` bases are copied exactly.  -> (t, q, [(start in t, start in q)] of the exact stretches), t and q bytes."""
    t = BASES[rng.integers(4, size=length)]
    at = {(length // (jumps + 1)) * (x + 1) + 11 * x for x in range(jumps)}
    q, skip, exact, marks, pending = [], 0, 0, [], False
    for pos, ch in enumerate(t):
        pending = pending or pos in at
        if pending and not exact:  # (a jump that falls into an exact stretch comes behind it)
            q.extend(BASES[rng.integers(4, size=jump)])
            pending = False
        if pos % every == every // 2 and pos + anchor <= length and not skip:
            exact = anchor
            marks.append((pos, len(q)))
        if exact:
            exact -= 1
            q.append(ch)
            continue
        if skip:
            skip -= 1
            continue
        r = rng.random()
        if r < 0.01:
            skip = int(rng.integers(0, 3))
            continue
        if r < 0.02:
            q.extend(BASES[rng.integers(4, size=int(rng.integers(1, 4)))])
        q.append(BASES[rng.integers(4)] if rng.random() < 0.05 else ch)
    return t.tobytes(), np.array(q, np.uint8).tobytes(), marks


def chain_pairs(seed, count, length=10000, seed_len=50, every=200, anchor=20, jumps=5, jump=30):
    """``count`` pairs of about ``length`` bases with their true chains: two flanks of ``chain_flank`` laid outwards from an exact seed
    of ``seed_len`` bases near the middle.  -> [(T, Q, chain)], chain = [(t, q, l)] ascending, every anchor exact."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        left_len = (length - seed_len) // 2 + int(rng.integers(-(length // 50), length // 50 + 1))
        (lt, lq, lm), (rt, rq, rm) = (chain_flank(rng, n, every, anchor, jumps, jump) for n in (left_len, length - seed_len - left_len))
        mid = BASES[rng.integers(4, size=seed_len)].tobytes()
        # the left flank was made outwards from the seed and is laid down reversed: a stretch at (u, v) lies at (len - u - anchor, ...)
        chain = sorted((len(lt) - u - anchor, len(lq) - v - anchor, anchor) for u, v in lm)
        chain.append((len(lt), len(lq), seed_len))
        chain += [(len(lt) + seed_len + u, len(lq) + seed_len + v, anchor) for u, v in rm]
        T, Q = lt[::-1] + mid + rt, lq[::-1] + mid + rq
        assert all(T[a:a + n] == Q[b:b + n] for a, b, n in chain)
        out.append((T, Q, chain))
    return out


_COMP = np.arange(256, dtype=np.uint8)
_COMP[[65, 67, 71, 84]] = [84, 71, 67, 65]


def revcomp(b):
    """The reverse complement of a byte string as the strand stages define it (tests/strand_textbook.py): upper-case A <-> T and
    C <-> G, every other byte kept, the order reversed."""
    return _COMP[np.frombuffer(bytes(b), np.uint8)][::-1].tobytes()


CAND_TRUE, CAND_OVERLAP, CAND_DECOY, CAND_REPEAT = range(4)


def noisy_candidates(rng, tl, ql, chain, decoys=2.0, repeats=0.5, overlaps=0.5, off=(300, 3000)):
    """What a seeding stage hands a chainer for one pair, given the pair's true ``chain``: the true anchors; per true anchor about
    ``overlaps`` shorter hits inside it, shifted along the true diagonal (they overlap it); about ``repeats`` copies of it at the same
    query position and another target position; and about ``decoys`` hits of its length on a wrong diagonal next to it.  A decoy or a
    repeat copy is ``off[0]`` .. ``off[1]`` bases off the diagonal of the true anchor it was made from, to either side (at minimap2's
    pen_gap = 38 / 256 a detour over a hit 300 off costs 48 each way and gains the hit's 20).  Sorted by
    target position (then query position).  -> (candidates [(t, q, l)], kind per candidate: CAND_*)."""
    out = [(t, q, l, CAND_TRUE) for t, q, l in chain]
    for t, q, l in chain:
        for _ in range(rng.poisson(overlaps)):
            if l >= 4:
                d = int(rng.integers(1, l // 2 + 1))
                out.append((t + d, q + d, l - d, CAND_OVERLAP))
        for kind, rate in ((CAND_REPEAT, repeats), (CAND_DECOY, decoys)):
            for _ in range(rng.poisson(rate)):
                shift = int(rng.integers(off[0], off[1] + 1)) * (1 if rng.random() < 0.5 else -1)
                along = 0 if kind == CAND_REPEAT else int(rng.integers(-100, 101))  # a decoy lies anywhere around the anchor
                nt, nq = t + along + shift, q + along
                if 0 <= nt and nt + l <= tl and 0 <= nq and nq + l <= ql:
                    out.append((nt, nq, l, kind))
    out.sort()
    return [c[:3] for c in out], [c[3] for c in out]


def mapping_set(seed, count, length=10000, spacer=3000):
    """Reads with a known place on one reference: the windows of ``chain_pairs(seed, count, length)`` laid into one random reference
    with ``spacer`` random bases in front of, between and behind them; every odd read is given reverse-complemented.
    -> (ref, reads, truth), truth[p] = (the position of T_p in ref, len(T_p), the strand of read p)."""
    pairs = chain_pairs(seed, count, length)
    rng = np.random.default_rng([seed, count, length, spacer])
    parts, truth, at = [], [], 0
    for p, (T, _, _) in enumerate(pairs):
        parts.append(BASES[rng.integers(4, size=spacer)].tobytes())
        at += spacer
        truth.append((at, len(T), p % 2))
        parts.append(T)
        at += len(T)
    parts.append(BASES[rng.integers(4, size=spacer)].tobytes())
    reads = [revcomp(Q) if p % 2 else Q for p, (_, Q, _) in enumerate(pairs)]
    return b"".join(parts), reads, truth


def split_mapping_set(seed, count, length=10000, spacer=3000):
    """Split reads on ``mapping_set(seed, count, length, spacer)``'s reference: read p is a chimera of two windows, the first half of
    the read of T_p followed by the second half of the read of T_(p + 1) (T_0 behind the last), both as ``chain_pairs`` made them
    (forward).  Every third read (p % 3 == 2) has its second part reverse-complemented: an inversion, ONE read with a part on each
    strand.  -> (ref, reads, truth), truth[p] = the read's two parts, each (the position of the part's window in ref, the window's
    length, the part's strand, q_beg, q_end): the part is read[q_beg:q_end] and lies inside that window, in its first half (part 0)
    or its second (part 1)."""
    ref, _, placed = mapping_set(seed, count, length, spacer)
    pairs = chain_pairs(seed, count, length)
    reads, truth = [], []
    for p in range(count):
        a, b = pairs[p][1], pairs[(p + 1) % count][1]
        first, second = a[:len(a) // 2], b[len(b) // 2:]
        inverted = p % 3 == 2
        reads.append(first + (revcomp(second) if inverted else second))
        truth.append([(placed[p][0], placed[p][1], 0, 0, len(first)),
                      (placed[(p + 1) % count][0], placed[(p + 1) % count][1], 1 if inverted else 0, len(first), len(first) + len(second))])
    return ref, reads, truth


def contig_cuts(count, truth, spacer, contigs):
    """The ``contigs`` - 1 positions at which ``mapping_set``'s reference is cut into contigs, ascending: every one inside a spacer
    between two reads (the outer spacers where there is one read), spread over them in order, evenly spaced inside a spacer.  The
    byte AT a cut belongs to neither side: it is the gap."""
    if contigs == 1:
        return []
    begins = [pos - spacer for pos, _, _ in truth] + [truth[-1][0] + truth[-1][1]]  # where the count + 1 spacers begin
    usable = begins[1:count] if count > 1 else begins
    per = [0] * len(usable)
    for k in range(contigs - 1):
        per[k * len(usable) // (contigs - 1)] += 1
    assert 2 * max(per) < spacer, "the spacers do not hold that many cuts"
    return [b + spacer * (j + 1) // (m + 1) for b, m in zip(usable, per) for j in range(m)]


def contig_mapping_set(seed, count, length=10000, spacer=3000, contigs=2):
    """``mapping_set(seed, count, length, spacer)``'s reference cut into ``contigs`` pieces inside its spacers (``contig_cuts``; the
    byte at a cut is dropped: laid out again with one gap byte between two contigs, every base is where ``mapping_set`` has it).
    -> (contigs as [(name, bytes)], reads, truth), truth[p] = (the contig of T_p, its position in that contig, len(T_p), the strand)."""
    ref, reads, truth = mapping_set(seed, count, length, spacer)
    assert spacer >= 3 and 1 <= contigs
    edges = [-1] + contig_cuts(count, truth, spacer, contigs) + [len(ref)]
    pieces = [("contig%d" % c, ref[a + 1:b]) for c, (a, b) in enumerate(zip(edges, edges[1:]))]
    rid = [max(c for c in range(contigs) if edges[c] < pos) for pos, _, _ in truth]
    return pieces, reads, [(c, pos - edges[c] - 1, n, s) for c, (pos, n, s) in zip(rid, truth)]


def repeat_mapping_set(seed, count, length=10000, spacer=3000, copies=0, divergence=0.0):
    """``mapping_set(seed, count, length, spacer)`` on a reference with repeats: the windows of the first ``copies`` reads appended
    once more to the reference, each with its bases substituted (by another base) at rate ``divergence`` and followed by ``spacer``
    random bases.  The reads and the truth are ``mapping_set``'s: the true place of a read is its first copy.
    -> (ref, reads, truth, copy), copy[p] = (the position of the second copy of T_p in ref, len(T_p)) for p < copies."""
    ref, reads, truth = mapping_set(seed, count, length, spacer)
    assert 0 <= copies <= count and 0.0 <= divergence <= 1.0
    rng = np.random.default_rng([seed, count, length, spacer, copies, int(round(divergence * 1e6))])
    parts, copy, at = [ref], [], len(ref)
    for pos, n, _ in truth[:copies]:
        w = np.frombuffer(ref[pos:pos + n], np.uint8).copy()
        hit = np.flatnonzero(rng.random(n) < divergence)
        code = np.searchsorted(BASES, w[hit])
        w[hit] = BASES[(code + rng.integers(1, 4, size=len(hit))) % 4]
        copy.append((at, n))
        parts.append(w.tobytes())
        parts.append(BASES[rng.integers(4, size=spacer)].tobytes())
        at += n + spacer
    return b"".join(parts), reads, truth, copy


def variant_mapping_set(seed, ref_len=8000, read_len=1000, step=125, snvs=10, dele=3, ins=2):
    """A random reference, a DONOR copy of it with ``snvs`` substitutions, one deletion of ``dele`` bases and one insertion of ``ins``
    bases, and reads that tile the donor exactly: one of ``read_len`` every ``step`` bases, every odd one reverse-complemented.  The
    variants lie at least 300 bases apart and 1 000 from either end; the bases of an indel differ from both bases next to it (the
    reference is changed there to make it so), so the indel has one placement.
    -> (ref, reads, planted), planted a list in position order of ("X", pos, the donor's base), ("D", pos of the first deleted base,
    the deleted bases) and ("I", the position the insertion stands behind, the inserted bases), positions those of the reference."""
    rng = np.random.default_rng([seed, ref_len, read_len, step, snvs, dele, ins])
    count, apart, edge = snvs + 2, 300, 1000
    free = ref_len - 2 * edge - (count - 1) * apart - dele - 2
    assert free >= 0, "the reference does not hold the variants 300 apart and 1 000 from its ends"
    at = edge + np.sort(rng.integers(0, free + 1, count)) + apart * np.arange(count)
    kinds = ["X"] * count
    d, i = (int(x) for x in rng.choice(count, 2, replace=False))
    kinds[d], kinds[i] = "D", "I"
    ref = bytearray(random_genome(rng, ref_len).tobytes())
    pick = lambda avoid: int(rng.choice([b for b in b"ACGT" if b not in avoid]))  # noqa: E731
    planted = []
    for kind, pos in zip(kinds, (int(x) for x in at)):
        if kind == "X":
            planted.append(("X", pos, bytes([pick((ref[pos],))])))
        elif kind == "D":
            for k in range(pos, pos + dele):
                ref[k] = pick((ref[pos - 1], ref[pos + dele]))
            planted.append(("D", pos, bytes(ref[pos:pos + dele])))
        else:
            planted.append(("I", pos, bytes(pick((ref[pos], ref[pos + 1])) for _ in range(ins))))
    return bytes(ref), _tile(apply_variants(ref, planted), read_len, step), planted


def apply_variants(ref, planted):
    """the reference with ``planted`` (variant_mapping_set's, in position order) applied: a haplotype"""
    donor, shift = bytearray(ref), 0
    for kind, pos, what in planted:
        if kind == "X":
            donor[pos + shift] = what[0]
        elif kind == "D":
            del donor[pos + shift:pos + shift + len(what)]
            shift -= len(what)
        else:
            donor[pos + shift + 1:pos + shift + 1] = what
            shift += len(what)
    return bytes(donor)


def _tile(donor, read_len, step):
    reads = [donor[s:s + read_len] for s in range(0, len(donor) - read_len + 1, step)]
    return [revcomp(r) if k % 2 else r for k, r in enumerate(reads)]


def diploid_variant_set(seed, het="even", **kw):
    """``variant_mapping_set(seed, **kw)``'s reference and donor as haplotype A, which carries every planted variant, and a haplotype
    B that carries only the planted variants of the OTHER parity of index than ``het`` ("even" or "odd"): the variants whose index has
    parity ``het`` are heterozygous, the others homozygous.  Reads tile both haplotypes as that function tiles its donor, A's first.
    -> (ref, reads, planted, zygosity), zygosity[k] 1 where planted[k] is heterozygous and 2 where it is homozygous."""
    if het not in ("even", "odd"):
        raise ValueError('het is "even" or "odd"')
    ref, reads, planted = variant_mapping_set(seed, **kw)
    read_len, step = kw.get("read_len", 1000), kw.get("step", 125)
    parity = 0 if het == "even" else 1
    zygosity = [1 if k % 2 == parity else 2 for k in range(len(planted))]
    hap_b = apply_variants(ref, [v for v, z in zip(planted, zygosity) if z == 2])
    return ref, reads + _tile(hap_b, read_len, step), planted, zygosity
