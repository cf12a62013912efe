"""mgl_sw_align_chain_batch_device against the textbook (tests/chain_textbook.py) on random chains: 1 .. 12 anchors (now and then 70 .. 140)
of 1 .. 40 bases, exact or not, gaps of 0 .. 150 bases on either side (noisy copies, unrelated, or empty on one side), flanks of 0 .. 300,
random bands, Z-drop thresholds, parameter sets and every flag, rows that many joined CIGARs do not fit, and gap bounds that some gaps
exceed: every output of every pair -- the record, both side records, the gap scores, CIGAR text or binary, length, status.  Not a test:
prints the pairs run, the calls and the mismatches (expected 0).

  python scripts/chain_align_fuzz.py --seconds 60 --seed 1
"""
import argparse, os, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import chain_textbook as ct
import extend_textbook as et
import seed_extend_textbook as stb
from chain_cases import chain_pair
from mgl_amd.smithwaterman import MicrosoftSmithWaterman

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=60)
ap.add_argument("--seed", type=int, default=1)
args = ap.parse_args()
rng = np.random.default_rng(args.seed)
a = MicrosoftSmithWaterman(0)
ALPHA = (b"ACGT", b"AC", b"A", b"ACGTN")


def length(top):
    """0 a fifth of the time, otherwise up to top, small values more often"""
    r = rng.random()
    return 0 if r < 0.2 else int(rng.integers(1, 6)) if r < 0.4 else int(rng.integers(1, top + 1))


def pair():
    K = int(rng.integers(70, 141)) if rng.random() < 0.03 else int(rng.integers(1, 13))
    top = 12 if K > 20 else int(rng.choice((8, 70, 150)))
    gaps = []
    for _ in range(K - 1):
        gt = length(top)
        gaps.append((gt, length(top) if rng.random() < 0.3 else max(0, gt + int(rng.integers(-4, 5)))))
    lt, rt = length(300), length(300)
    flanks = (lt, max(0, lt + int(rng.integers(-5, 6))) if rng.random() < 0.8 else length(300), rt, max(0, rt + int(rng.integers(-5, 6))) if rng.random() < 0.8 else length(300))
    return chain_pair(rng, flanks, gaps, [int(rng.integers(1, 41)) for _ in range(K)], ALPHA[rng.integers(len(ALPHA))], exact=rng.random() < 0.7)


pairs = bad = calls = dropped = overflow = unsupported = gaps_run = 0
t0 = time.time()
while time.time() - t0 < args.seconds:
    params = (int(rng.integers(0, 300)), -int(rng.integers(0, 300)), int(rng.integers(0, 400)), int(rng.integers(0, 40)))
    band = int(rng.choice((0, 1, 2, 3, 8, 30, 63, 64, 65, 130, 400)))
    zdrop = int(rng.choice((-1, 0, params[3], 2 * params[2] + 1, 10 * params[0] + 50, 400 * max(params[3], 1), 1 << 30)))
    to_qend, adaptive, binary, score_only = (bool(rng.integers(2)) for _ in range(4))
    score_only = score_only and rng.random() < 0.3
    Ts, Qs, chains = zip(*[pair() for _ in range(int(rng.integers(1, 60)))])
    stride = 2 * (max(len(t) for t in Ts) + max(len(q) for q in Qs)) + 32  # (a CIGAR has at most two characters per base it consumes)
    if rng.random() < 0.2:
        stride = int(rng.integers(4, 60))  # rows that many joined CIGARs do not fit
    if binary:
        stride *= 4
    max_gap = (150, 150) if rng.random() < 0.8 else (int(rng.integers(0, 100)), int(rng.integers(0, 100)))
    res, left, right, gs, st = a.align_chain(list(Ts), list(Qs), list(chains), band, zdrop, params, to_qend, cigar_stride=stride, binary_cigar=binary, score_only=score_only,
                                             return_status=True, adaptive_band=adaptive, return_sides=True, return_gap_scores=True, max_gap=max_gap)
    calls += 1
    at = 0
    for k, (T, Q, c) in enumerate(zip(Ts, Qs, chains)):
        aln, cigar, l, r, gaps = ct.chain_align(T, Q, c, *params, band, zdrop, to_qend, adaptive)
        size = 0 if score_only else 4 * len(stb.elements(cigar)) if binary else len(cigar)
        got = [int(st[k]), ct.ChainAln(*(int(res[x][k]) for x in range(8))), et.Ext(*map(int, left[k])), et.Ext(*map(int, right[k])), [int(x) for x in gs[at:at + len(c)]]]
        at += len(c)
        if not score_only:
            raw = res.cigars.slots[k, :res.cigar_len[k]]
            got += [int(res.cigar_len[k]), et.cigar_binary_to_text(raw.view("<u4")) if binary else raw.tobytes().decode()]
        zero = et.Ext(*[0] * 8)
        real = [(nt - s - n, nq - q - n) for (s, q, n), (nt, nq, _) in zip(c, c[1:]) if nt - s - n > 0 and nq - q - n > 0]
        gaps_run += len(real)
        if any(x > max_gap[0] or y > max_gap[1] for x, y in real):
            want = [5, ct.ChainAln(*[0] * 8), zero, zero, [0] * len(c)] + ([] if score_only else [0, ""])
            unsupported += 1
        elif size > (stride & ~3 if binary else stride):
            want = [2, ct.ChainAln(*[0] * 8), zero, zero, [0] * len(c), 0, ""]
            overflow += 1
        else:
            want = [0, aln, l, r, gaps] + ([] if score_only else [size, cigar])
        pairs += 1
        dropped += aln.dropped != 0
        if got != want:
            bad += 1
            if bad <= 5:
                print("MISMATCH", T, Q, c, params, band, zdrop, to_qend, adaptive, binary, score_only, stride, max_gap, got, want, flush=True)
print(f"chain_align_fuzz seed {args.seed}: {pairs} pairs, {gaps_run} filled gaps ({dropped} pairs with a dropped side, {overflow} CIGAR overflows, {unsupported} pairs with a gap above the bound) "
      f"in {calls} calls, {bad} mismatches", flush=True)
sys.exit(1 if bad else 0)
