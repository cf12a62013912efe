"""The cases of mgl_sw_seed_batch_device that tests/test_seed_textbook.py (the textbook against a brute-force restatement) and
tests/test_gpu_seed.py (the kernels against the textbook) share.  A case is (name, (k, w, max_occ), T, Q); a batch is the cases of one
parameter set, since the parameters are the call's."""
import functools

import numpy as np

import seed_textbook as tb

CANARY = -777
K_ALL = tuple(range(4, 17))
W_ALL = (1, 2, 10, 32)

# what the kernel streams or sorts in (mgl_amd/csrc/sw_seed.h): tests place lengths around each, +- 1
SEED_BLOCK = 1024     # k-mer positions sketched at once
SEED_LDS_TAB = 4096   # entries of the query's table in LDS; above it the table moves to the workspace slot
SEED_LDS_HITS = 2048  # raw hits in LDS; above it they move to the workspace slot
SORT_SIZES = (64, 256, 1024)  # bitonic sorts pad to a power of two: sketches of 2^m - 1, 2^m, 2^m + 1 entries


def rand_seq(rng, n, alphabet=b"ACGT"):
    return bytes(np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), n)])


def mutate(rng, s, sub=0.03, indel=0.01):
    """a copy of s with substitutions and single-base insertions / deletions"""
    out = bytearray()
    for b in s:
        r = rng.random()
        if r < indel:
            continue
        if r < 2 * indel:
            out += rand_seq(rng, 1)
        out.append(b"ACGT"[rng.integers(4)] if rng.random() < sub else b)
    return bytes(out)


def gap_pair(d, k=8, w=12):
    """T = Q whose sketch has two neighbouring positions exactly d apart with no third hit near: found by a seeded search"""
    for seed in range(4000):
        s = rand_seq(np.random.default_rng(seed), 3 * k + w)
        pos = [i for i, _ in tb.sketch(s, k, w)]
        if any(b - a == d for a, b in zip(pos, pos[1:])):
            return s, s
    raise AssertionError(d)


def occ_query(rng, k, times):
    """a query in which one k-mer occurs exactly `times` times (w = 1: every position is in the sketch) -> (Q, the k-mer)"""
    while True:
        kmer = rand_seq(rng, k)
        q = b"".join(kmer + rand_seq(rng, int(rng.integers(3, 9))) for _ in range(times))
        if sum(q[i:i + k] == kmer for i in range(len(q))) == times:
            return q, kmer


@functools.lru_cache(maxsize=None)
def edge_cases():
    rng = np.random.default_rng(20241)
    out = []
    # lengths around k and k + w
    k, w = 6, 5
    base = rand_seq(rng, 40)
    for n in (k - 1, k, k + 1, k + w - 2, k + w - 1, k + w):
        out.append((f"len{n}", (k, w, 8), base[:n], base))
        out.append((f"qlen{n}", (k, w, 8), base, base[3:3 + n]))
    # a stray byte at every offset of a short sequence, and lower case
    short = rand_seq(rng, 14)
    for i in range(len(short)):
        out.append((f"N@{i}", (5, 3, 8), short[:i] + b"N" + short[i + 1:], short))
        out.append((f"n@{i}q", (5, 3, 8), short, short[:i] + b"n" + short[i + 1:]))
    out.append(("lower", (5, 3, 8), short.lower(), short))
    out.append(("lower1", (5, 3, 8), short[:6] + short[6:7].lower() + short[7:], short))
    # equal hashes across a window: the tie rule, and max_occ
    for occ in (8, 30, 64):
        out.append((f"homopolymer{occ}", (6, 4, occ), b"A" * 40, b"A" * 37))
        out.append((f"two-letter{occ}", (6, 4, occ), b"AC" * 25, b"CA" * 20 + b"C"))
    # a key exactly max_occ and max_occ + 1 times in the query's sketch
    for times in (3, 4):
        q, kmer = occ_query(rng, 9, times)
        out.append((f"occ{times}of3", (9, 1, 3), rand_seq(rng, 5) + kmer + rand_seq(rng, 5), q))
    # two hits on one diagonal k - 1, k, k + 1 apart
    for d in (7, 8, 9):
        out.append((f"gap{d}", (8, 12, 8)) + gap_pair(d))
    # runs on two diagonals interleaved in t
    x = rand_seq(rng, 60)
    out.append(("interleaved", (7, 1, 8), x, x + x[20:40]))
    # k = 16: all 32 bits of the key, the top bit set
    gt = rand_seq(rng, 80, b"GT")
    out.append(("k16-GT", (16, 3, 8), gt, gt[5:70]))
    out.append(("k16-T", (16, 1, 64), b"T" * 30, b"T" * 25))
    r16 = rand_seq(rng, 120)
    out.append(("k16-random", (16, 10, 8), r16, mutate(rng, r16, 0.01, 0.005)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def random_cases():
    """every k with every w of W_ALL: a window and a mutated read, alphabets of 2 to 4 letters, a stray N"""
    rng = np.random.default_rng(7)
    out = []
    for k in K_ALL:
        for w in W_ALL:
            t = bytearray(rand_seq(rng, int(rng.integers(60, 160)), b"ACGT"[:int(rng.integers(2, 5))]))
            if rng.random() < 0.5:
                t[int(rng.integers(len(t)))] = ord("N")
            out.append((f"random-k{k}-w{w}", (k, w, int(rng.integers(1, 12))), bytes(t), mutate(rng, bytes(t))))
    return tuple(out)


def by_params(cases):
    groups = {}
    for name, params, T, Q in cases:
        groups.setdefault(params, []).append((name, T, Q))
    return groups


def expected(Ts, Qs, k, w, max_occ, merge, max_cand, capacity, pad):
    """the textbook's arrays as the GPU test's canaried arrays must look: (cand_start, cand_t, cand_q, cand_len, status)"""
    start, ct, cq, cl, status = tb.seed_batch(Ts, Qs, k, w, max_occ, merge, max_cand, capacity)
    n = len(Ts)
    want = [np.full(n + 1 + pad, CANARY, np.int64)] + [np.full(capacity + pad, CANARY, np.int32) for _ in range(3)] + [np.full(n + pad, CANARY, np.int32)]
    want[0][:n + 1] = start
    for arr, vals in zip(want[1:4], (ct, cq, cl)):
        arr[:len(vals)] = vals
    want[4][:n] = status
    return want
