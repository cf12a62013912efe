"""Constructed inputs that tests/test_describe_textbook.py (CPU), tests/test_gpu_describe.py (GPU) and scripts/describe_fuzz.py share.
A case is Case(t, q, rec, cigar, slot, cigar_len, status_in, want): the pair's whole sequences, (t_beg, t_end, q_beg, q_end), the CIGAR
as [(len, op)] (None where the slot is made by hand), the bytes of the slot (None: made from the CIGAR), its length (None: the slot's),
a status going in, and the status expected where it is not 0 / an overflow.  Seeded by the caller."""
from collections import namedtuple

import numpy as np

import describe_textbook as dtb

BAD_ARG, OVERFLOW = 1, 2
CANARY = 0x5A5A5A5A
CANARY_BYTE = 0x5A
PAD = 16

Case = namedtuple("Case", "t q rec cigar slot cigar_len status_in want")


def case(t, q, cigar, rec=None, slot=None, cigar_len=None, status_in=0, want=0):
    t, q = bytes(t), bytes(q)
    return Case(t, q, tuple(rec) if rec is not None else (0, len(t), 0, len(q)), cigar, slot, cigar_len, status_in, want)


def seq(rng, n, alphabet=b"ACGT"):
    return np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), n)].tobytes()


def mutate(rng, s, p, alphabet=b"ACGT"):
    """every byte replaced by ANOTHER one of the alphabet with probability p"""
    out = bytearray(s)
    for k in np.flatnonzero(rng.random(len(s)) < p):
        out[k] = rng.choice([c for c in alphabet if c != out[k]])
    return bytes(out)


def random_alignment(rng, n_elements, alphabet=b"ACGT", p_mismatch=0.1, max_len=40):
    """-> (target, query, [(len, op)]): n_elements elements, now and then two equal operations next to each other"""
    t, q, cigar, last = b"", b"", [], None
    for _ in range(n_elements):
        op = "MID"[int(rng.integers(0, 3))] if last is None or rng.random() < 0.1 else rng.choice([o for o in "MID" if o != last])
        n = int(rng.integers(1, max_len + 1))
        s = seq(rng, n, alphabet)
        if op == "M":
            t, q = t + s, q + mutate(rng, s, p_mismatch, alphabet)
        elif op == "I":
            q += s
        else:
            t += s
        cigar.append((n, str(op)))
        last = op
    return t, q, cigar


def with_mismatches(rng, s, columns):
    out = bytearray(s)
    for c in columns:
        out[c] = rng.choice([x for x in b"ACGT" if x != out[c]])
    return bytes(out)


def embedded(rng, t, q, cigar, t_pre, t_post, q_pre, q_post, **kw):
    """the alignment inside longer sequences: the spans start at t_pre / q_pre"""
    T, Q = seq(rng, t_pre) + t + seq(rng, t_post), seq(rng, q_pre) + q + seq(rng, q_post)
    return case(T, Q, cigar, (t_pre, t_pre + len(t), q_pre, q_pre + len(q)), **kw)


def slot_of(c, binary):
    return dtb.cigar_bytes(c.cigar, binary) if c.slot is None else bytes(c.slot)


def pack(cases, binary, cigar_stride=None, gaps=None):
    """-> dict of numpy arrays as the entry reads them.  The first case's sequences start at byte 0 of their buffers and the last
    case's end at the last byte; ``gaps[k]`` = (bytes in front of case k's target, of its query), so that a span starts at any
    residue of 16."""
    n = len(cases)
    gaps = gaps or [(0, 0)] * n
    tb, qb, ts, qs = bytearray(), bytearray(), [], []
    for c, (gt, gq) in zip(cases, gaps):
        tb += b"#" * gt
        qb += b"%" * gq
        ts.append(len(tb)), qs.append(len(qb))
        tb += c.t
        qb += c.q
    slots = [slot_of(c, binary) for c in cases]
    if cigar_stride is None:
        cigar_stride = (max([len(s) for s in slots] + [4]) + 3) // 4 * 4
    cg = np.full((n, cigar_stride), ord("?"), np.uint8)
    for k, s in enumerate(slots):
        s = s[:cigar_stride]
        cg[k, :len(s)] = np.frombuffer(s, np.uint8)
    rec = np.zeros((n, 8), np.int32)
    rec[:, 0], rec[:, 5:] = 12345, -7  # the fields that are not read
    rec[:, 1:5] = np.asarray([c.rec for c in cases], np.int64).reshape(n, 4).astype(np.int32)
    u8 = lambda b: np.frombuffer(bytes(b) or b"\0", np.uint8).copy()  # noqa: E731
    return dict(targets=u8(tb), t_start=np.asarray(ts, np.int64), t_len=np.asarray([len(c.t) for c in cases], np.int32), queries=u8(qb),
                q_start=np.asarray(qs, np.int64), q_len=np.asarray([len(c.q) for c in cases], np.int32), aln=rec, cigar=cg.reshape(-1),
                cigar_stride=cigar_stride, cigar_len=np.asarray([len(s) if c.cigar_len is None else c.cigar_len for c, s in zip(cases, slots)], np.int32),
                status_in=np.asarray([c.status_in for c in cases], np.int32))


def described(c):
    tb, te, qb, qe = c.rec
    return dtb.describe(c.t[tb:te], c.q[qb:qe], c.cigar)


def expected(cases, binary, md_stride, xcigar_stride, md=True, xcigar=True):
    """What the entry must leave in output arrays that were CANARY everywhere and PAD entries longer than their size:
    (stats [n * 8 + PAD] int32, md [n * md_stride + PAD] uint8 or None, xcigar likewise, status [n + PAD] int32)"""
    n = len(cases)
    stats, status = np.full(n * 8 + PAD, CANARY, np.int32), np.full(n + PAD, CANARY, np.int32)
    mdo = np.full(n * md_stride + PAD, CANARY_BYTE, np.uint8) if md else None
    xco = np.full(n * xcigar_stride + PAD, CANARY_BYTE, np.uint8) if xcigar else None
    for k, c in enumerate(cases):
        if c.status_in or c.want:
            stats[8 * k:8 * k + 8], status[k] = 0, c.status_in or c.want
            continue
        d = described(c)
        stats[8 * k:8 * k + 8] = dtb.stats(d, binary)
        xb = dtb.xcigar_bytes(d.xcigar, binary)
        over = False
        if md:
            keep = d.md[:md_stride]
            mdo[k * md_stride:k * md_stride + len(keep)] = np.frombuffer(keep, np.uint8)
            over |= len(d.md) > md_stride
        if xcigar:
            keep = xb[:xcigar_stride // 4 * 4 if binary else xcigar_stride]
            xco[k * xcigar_stride:k * xcigar_stride + len(keep)] = np.frombuffer(keep, np.uint8)
            over |= len(xb) > xcigar_stride
        status[k] = OVERFLOW if over else 0
    return stats, mdo, xco, status


# ---- the cases of the GPU test
STEP_COLUMNS = (1, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097)
RUNS = (9, 10, 99, 100, 999, 1000, 9999, 10000)
DELETIONS = (1, 63, 64, 65, 1000)


def seam_cases(rng):
    """one-M alignments at the seams of a 64-column step, one mismatch moved over the first, last and seam columns; 200 columns all
    mismatched; match runs at the digit borders"""
    out = []
    for cols in STEP_COLUMNS:
        t = seq(rng, cols)
        out.append(case(t, t, [(cols, "M")]))
        for at in sorted({0, 62, 63, 64, 65, cols - 2, cols - 1, cols // 64 * 64 - 1, cols // 64 * 64}):
            if 0 <= at < cols:
                out.append(case(t, with_mismatches(rng, t, [at]), [(cols, "M")]))
    t = seq(rng, 200)
    out.append(case(t, with_mismatches(rng, t, range(200)), [(200, "M")]))
    for run in RUNS:
        t = seq(rng, 2 * run + 1)
        out.append(case(t, with_mismatches(rng, t, [run]), [(2 * run + 1, "M")]))
    return out


def indel_cases(rng):
    """deletions with a mismatch directly before and directly behind; an insertion inside a run across a step seam; CIGARs that begin
    and end with I or D, only I, only D, empty; 3 000 elements of 1M1I / 1M1D (more than one LDS chunk); lower case and N"""
    out = []
    for n in DELETIONS:
        a, d, b = seq(rng, 70), seq(rng, n), seq(rng, 70)
        out.append(case(a + d + b, with_mismatches(rng, a, [69]) + with_mismatches(rng, b, [0]), [(70, "M"), (n, "D"), (70, "M")]))
    a, i, b = seq(rng, 60), seq(rng, 5), seq(rng, 100)
    out.append(case(a + b, a + i + b, [(60, "M"), (5, "I"), (100, "M")]))
    out.append(case(a + b, with_mismatches(rng, a, [3]) + i + with_mismatches(rng, b, [7]), [(60, "M"), (5, "I"), (100, "M")]))
    m = seq(rng, 30)
    out.append(case(m, i + m + i, [(5, "I"), (30, "M"), (5, "I")]))
    out.append(case(i + m + i, m, [(5, "D"), (30, "M"), (5, "D")]))
    out.append(case(i + m, m + i, [(5, "D"), (30, "M"), (5, "I")]))
    out.append(case(b"", seq(rng, 77), [(77, "I")]))
    out.append(case(seq(rng, 77), b"", [(77, "D")]))
    out.append(case(seq(rng, 9), seq(rng, 9), [], rec=(4, 4, 9, 9)))
    out.append(case(b"", b"", []))
    for op in "ID":
        m, x = seq(rng, 3000), seq(rng, 3000)
        both = bytes(v for pair in zip(m, x) for v in pair)
        q = mutate(rng, m, 0.2)
        qq = bytes(v for pair in zip(q, x) for v in pair)
        out.append(case(m, qq, [(1, "M"), (1, "I")] * 3000) if op == "I" else case(both, q, [(1, "M"), (1, "D")] * 3000))
    t = seq(rng, 150, b"ACGTNacgtn")
    out.append(case(t, mutate(rng, t, 0.3, b"ACGTNacgtn"), [(150, "M")]))
    out.append(case(b"ACGTNNacgt" * 7, b"acgtNNACGT" * 7, [(70, "M")]))
    return out


def offset_cases(rng):
    """-> (cases, gaps): every residue 0 .. 15 of t_start + t_beg and of q_start + q_beg, in two orders; the first case's spans start at
    byte 0 of their buffers, the last one's end at their last byte"""
    cases, gaps = [], []
    t, q, cg = random_alignment(rng, 5, p_mismatch=0.2)
    cases.append(case(t, q, cg))
    gaps.append((0, 0))
    tb, qb = len(t), len(q)
    for r in range(16):
        t, q, cg = random_alignment(rng, 6, p_mismatch=0.2)
        t_pre, q_pre = int(rng.integers(0, 5)), int(rng.integers(0, 5))
        c = embedded(rng, t, q, cg, t_pre, int(rng.integers(0, 5)), q_pre, int(rng.integers(0, 5)))
        g = ((r - tb - t_pre) % 16, ((5 * r + 3) - qb - q_pre) % 16)
        assert (tb + g[0] + t_pre) % 16 == r and (qb + g[1] + q_pre) % 16 == (5 * r + 3) % 16
        tb, qb = tb + g[0] + len(c.t), qb + g[1] + len(c.q)
        cases.append(c)
        gaps.append(g)
    t, q, cg = random_alignment(rng, 5, p_mismatch=0.2)
    cases.append(embedded(rng, t, q, cg, 7, 0, 11, 0))
    gaps.append((1, 2))
    return cases, gaps


def refusals(rng):
    """every per-alignment refusal, each between two good alignments -> cases (the slots in TEXT; see binary_refusals)"""
    good = lambda: case(*random_alignment(rng, 5, p_mismatch=0.2))  # noqa: E731
    t = seq(rng, 20)
    bad = [
        case(t, t, [(20, "M")], rec=(0, 21, 0, 20), want=BAD_ARG),                       # spans outside the lengths
        case(t, t, [(20, "M")], rec=(0, 20, -1, 19), want=BAD_ARG),
        case(t, t, [(10, "M")], rec=(12, 2, 0, 10), want=BAD_ARG),
        case(t, t, [(20, "M")], rec=(0, 20, 5, 4), want=BAD_ARG),
        case(t, t, [(19, "M")], want=BAD_ARG),                                            # sums one off, on either side
        case(t, t, [(19, "M"), (1, "D")], want=BAD_ARG),
        case(t, t, [(20, "M"), (1, "I")], want=BAD_ARG),
        case(t, t, None, slot=b"10M0I10M", want=BAD_ARG),                                 # a zero-length element
        case(t, t, None, slot=b"10M00D10M", want=BAD_ARG),
        case(t, t, None, slot=b"20S", want=BAD_ARG),                                      # S, =, a digit-less element, what is no CIGAR
        case(t, t, None, slot=b"20=", want=BAD_ARG),
        case(t, t, None, slot=b"M19M", want=BAD_ARG),
        case(t, t, None, slot=b"10MM9M", want=BAD_ARG),
        case(t, t, None, slot=b"20M5", want=BAD_ARG),
        case(t, t, None, slot=b"20M ", want=BAD_ARG),
        case(t, t, None, slot=b"20M", cigar_len=-1, want=BAD_ARG),
        case(t, t, None, slot=b"20M", cigar_len=1 << 20, want=BAD_ARG),                   # cigar_len above the stride
        case(t, t, None, slot=b"4294967316M", want=BAD_ARG),                              # 2^32 + 20
        case(t, t, None, slot=b"2147483648M", want=BAD_ARG),
        case(t, t, None, slot=b"18446744073709551636M", want=BAD_ARG),                    # 2^64 + 20
        case(t, t, None, slot=b"\xff" * 24, cigar_len=0, status_in=5),                    # a status going in, over a poisoned slot
        case(t, t, None, slot=b"\xff" * 24, rec=(-9, 1 << 30, 77, -3), cigar_len=1 << 30, status_in=BAD_ARG),
    ]
    out = [good()]
    for b in bad:
        out += [b, good()]
    return out


def binary_refusals(rng):
    w = lambda *els: np.asarray([n << 4 | op for n, op in els], "<u4").tobytes()  # noqa: E731
    good = lambda: case(*random_alignment(rng, 5, p_mismatch=0.2))  # noqa: E731
    t = seq(rng, 20)
    bad = [
        case(t, t, [(20, "M")], rec=(1, 21, 0, 20), want=BAD_ARG),
        case(t, t, [(19, "M")], want=BAD_ARG),
        case(t, t, [(20, "M"), (1, "D")], want=BAD_ARG),
        case(t, t, None, slot=w((10, 0), (0, 1), (10, 0)), want=BAD_ARG),                 # a zero-length element
        case(t, t, None, slot=w((20, 4)), want=BAD_ARG),                                  # S
        case(t, t, None, slot=w((20, 7)), want=BAD_ARG),                                  # =
        case(t, t, None, slot=w((20, 0)), cigar_len=3, want=BAD_ARG),                     # no whole word
        case(t, t, None, slot=w((20, 0)), cigar_len=1 << 20, want=BAD_ARG),
        case(t, t, None, slot=w(((1 << 28) - 1, 0)) * 16 + w((16, 0), (20, 0)), want=BAD_ARG),  # the sums in 64 bits: 2^32 + 20 columns
        case(t, t, None, slot=b"\xff" * 24, cigar_len=0, status_in=5),
    ]
    out = [good()]
    for b in bad:
        out += [b, good()]
    return out


def mixed_batch(rng, n=300):
    """n alignments of every kind: more than the waves of one grid on a small part, so the persistent loop turns"""
    out = []
    for k in range(n):
        t, q, cg = random_alignment(rng, int(rng.integers(0, 30)), p_mismatch=float(rng.choice((0.0, 0.05, 0.5))), max_len=int(rng.choice((3, 40, 200))))
        c = embedded(rng, t, q, cg, int(rng.integers(0, 20)), int(rng.integers(0, 20)), int(rng.integers(0, 20)), int(rng.integers(0, 20)))
        if k % 37 == 5:
            c = c._replace(status_in=3)
        if k % 41 == 7 and cg:
            c = c._replace(cigar=cg + [(1, "M")], want=BAD_ARG)
        out.append(c)
    return out
