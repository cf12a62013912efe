"""Constructed inputs that tests/test_extend_adaptive_textbook.py (CPU) and tests/test_gpu_extend_adaptive.py (GPU) share: pairs whose path
drifts away from the main diagonal by more than the band, pairs whose band shifts by exactly +-band at a seam, and the noisy pairs of the
sweeps.  Seeded: both files see the same bytes."""
import numpy as np

GATK = (200, -150, 260, 11)
PARAM_SETS = [GATK, (25, -50, 110, 6), (10, -15, 30, 5), (3, -1, 4, 3), (1, -1, 1, 1), (1, -4, 6, 1), (5, -4, 10, 1)]  # tests/test_gpu_banded.py's
ACGT = np.frombuffer(b"ACGT", np.uint8)


def seq(rng, n, alphabet=ACGT):
    return alphabet[rng.integers(len(alphabet), size=n)].tobytes()


def noisy_pair(rng, tl, ql, alphabet=b"ACGT", rate=0.04, run=8):
    """a target and a noisy copy of it cut or padded to ql: substitutions, deleted runs and inserted runs of up to `run` bases"""
    a = np.frombuffer(alphabet, np.uint8)
    t = a[rng.integers(len(a), size=tl)]
    q, skip = [], 0
    for ch in t:
        if skip:
            skip -= 1
            continue
        r = rng.random()
        if r < rate:
            skip = int(rng.integers(0, run))
            continue
        if r < 2 * rate:
            q.extend(a[rng.integers(len(a), size=int(rng.integers(1, run + 1)))])
        q.append(a[rng.integers(len(a))] if rng.random() < 0.05 else ch)
    q = np.array(q[:ql] + list(a[rng.integers(len(a), size=max(0, ql - len(q)))]), np.uint8)
    return t.tobytes(), q.tobytes()


def drift_pairs(rows=3000, indels=10, size=20, seed=77):
    """{name: (t, q)}: about `rows` rows, identical except `indels` indels of `size` bases, evenly spaced (about 4 seams apart): deletions
    only (the path ends size x indels diagonals to the left), insertions only (to the right), and the first half deletions, the second
    half insertions (out and back)"""
    rng = np.random.default_rng(seed)
    base = seq(rng, rows)
    gap = rows // (indels + 1)
    out = {}
    for name, kinds in (("deletions", "D" * indels), ("insertions", "I" * indels), ("mixed", "D" * (indels // 2) + "I" * (indels - indels // 2))):
        q, at = bytearray(), 0
        for n, kind in enumerate(kinds):
            cut = gap * (n + 1) + 7 * n  # (not on a multiple of 64)
            q += base[at:cut]
            if kind == "D":
                at = cut + size
            else:
                q += seq(rng, size)
                at = cut
        q += base[at:]
        out[name] = (base, bytes(q))
    return out


def seam_shift_pairs(band, seed=5, tail=150):
    """[(t, q)]: the band moves by exactly +band (0), -band (1) at the first seam (an indel of `band` bases at the very start), by +band
    (2), -band (3) at the second (the same indel behind row 70), and out and back: +band at the first seam and -band at the second (4),
    and the reverse (5)"""
    rng = np.random.default_rng(seed)
    core, junk = seq(rng, 130 + tail), seq(rng, band, np.frombuffer(b"N", np.uint8))
    mid = core[:70] + junk + core[70:]
    return [(core, junk + core), (junk + core, core), (core, mid), (mid, core), (mid, junk + core), (junk + core, mid)]
