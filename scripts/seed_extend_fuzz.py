"""mgl_sw_extend_seed_batch_device against the textbook (tests/seed_extend_textbook.py) on random geometries up to 700 x 700, random seeds
(exact or not, at the edges or inside), bands, Z-drop thresholds, parameter sets and every flag: every output of every pair -- the record,
both side records, CIGAR text or binary, length, status.  Not a test: prints the pairs run, the calls and the mismatches (expected 0).

  python scripts/seed_extend_fuzz.py --seconds 60 --seed 1
"""
import argparse, os, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import extend_textbook as et
import seed_extend_textbook as stb
from mgl_amd.smithwaterman import MicrosoftSmithWaterman

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=60)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--max-len", type=int, default=700)
args = ap.parse_args()
rng = np.random.default_rng(args.seed)
a = MicrosoftSmithWaterman(0)
ALPHA = [np.frombuffer(x, np.uint8) for x in (b"ACGT", b"AC", b"A", b"ACGTN")]


def flank(al, tl, ql):
    """a noisy copy, an unrelated pair, or a noisy copy whose tail is unrelated (what the Z-drop rule is for); either may be empty"""
    t = al[rng.integers(len(al), size=tl)]
    kind = rng.random()
    if kind < 0.2:
        return t.tobytes(), al[rng.integers(len(al), size=ql)].tobytes()
    q, rate, skip = [], rng.choice((0.01, 0.05, 0.15)), 0
    for ch in t[:int(tl * rng.random()) if kind < 0.6 else tl]:
        if skip:
            skip -= 1
            continue
        r = rng.random()
        if r < rate:
            skip = int(rng.integers(0, 30))
            continue
        if r < 2 * rate:
            q.extend(al[rng.integers(len(al), size=int(rng.integers(1, 30)))])
        q.append(al[rng.integers(len(al))] if rng.random() < rate else ch)
    q = (q + list(ALPHA[0][rng.integers(4, size=ql)]))[:ql]
    return t.tobytes(), np.array(q, np.uint8).tobytes()


def pair(top):
    """a window and a query of 1 .. top bases around a seed: (T, Q, (st, sq, sl))"""
    al = ALPHA[rng.integers(len(ALPHA))]
    tl, ql = int(rng.integers(1, top + 1)), int(rng.integers(1, top + 1))
    sl = int(rng.integers(1, min(tl, ql, 60) + 1))
    edge = rng.random()
    st = 0 if edge < 0.1 else tl - sl if edge < 0.2 else int(rng.integers(0, tl - sl + 1))
    edge = rng.random()
    sq = 0 if edge < 0.1 else ql - sl if edge < 0.2 else int(rng.integers(0, ql - sl + 1))
    lt, lq = flank(al, st, sq)
    rt, rq = flank(al, tl - st - sl, ql - sq - sl)
    seed_t = al[rng.integers(len(al), size=sl)]
    seed_q = seed_t.copy()
    if rng.random() < 0.3:
        seed_q[rng.integers(sl)] = ord("T")
    return lt[::-1] + seed_t.tobytes() + rt, lq[::-1] + seed_q.tobytes() + rq, (st, sq, sl)


pairs = bad = calls = dropped = overflow = 0
t0 = time.time()
while time.time() - t0 < args.seconds:
    params = (int(rng.integers(0, 300)), -int(rng.integers(0, 300)), int(rng.integers(0, 400)), int(rng.integers(0, 40)))
    band = int(rng.choice((0, 1, 2, 3, 8, 30, 63, 64, 65, 130, 400, 1000)))
    zdrop = int(rng.choice((-1, 0, params[3], 2 * params[2] + 1, 10 * params[0] + 50, 400 * max(params[3], 1), 1 << 30)))
    to_qend, adaptive, binary, score_only = (bool(rng.integers(2)) for _ in range(4))
    score_only = score_only and rng.random() < 0.3
    top = int(rng.choice((20, 70, 200, args.max_len)))
    Ts, Qs, seeds = zip(*[pair(top) for _ in range(int(rng.integers(1, 80)))])
    stride = 2 * (max(len(t) for t in Ts) + max(len(q) for q in Qs)) + 32  # (a CIGAR has at most two characters per base it consumes)
    if rng.random() < 0.2:
        stride = int(rng.integers(4, 40))  # rows that many joined CIGARs do not fit
    if binary:
        stride *= 4
    res, left, right, st = a.extend_seed(list(Ts), list(Qs), list(seeds), band, zdrop, params, to_qend, cigar_stride=stride, binary_cigar=binary,
                                         score_only=score_only, return_status=True, adaptive_band=adaptive, return_sides=True)
    calls += 1
    for k, (T, Q, s) in enumerate(zip(Ts, Qs, seeds)):
        aln, cigar, l, r = stb.seed_extend(T, Q, s, *params, band, zdrop, to_qend, adaptive)
        size = 0 if score_only else 4 * len(stb.elements(cigar)) if binary else len(cigar)
        got = [int(st[k]), stb.SeedAln(*(int(res[c][k]) for c in range(8))), et.Ext(*map(int, left[k])), et.Ext(*map(int, right[k]))]
        if not score_only:
            raw = res.cigars.slots[k, :res.cigar_len[k]]
            got += [int(res.cigar_len[k]), et.cigar_binary_to_text(raw.view("<u4")) if binary else raw.tobytes().decode()]
        if size > (stride & ~3 if binary else stride):
            zero = et.Ext(*[0] * 8)
            want = [2, stb.SeedAln(*[0] * 8), zero, zero, 0, ""]
            overflow += 1
        else:
            want = [0, aln, l, r] + ([] if score_only else [size, cigar])
        pairs += 1
        dropped += aln.dropped != 0
        if got != want:
            bad += 1
            if bad <= 5:
                print("MISMATCH", T, Q, s, params, band, zdrop, to_qend, adaptive, binary, score_only, stride, got, want, flush=True)
print(f"seed_extend_fuzz seed {args.seed}: {pairs} pairs ({dropped} with a dropped side, {overflow} CIGAR overflows) in {calls} calls, {bad} mismatches", flush=True)
sys.exit(1 if bad else 0)
