"""mgl_sw_align_batch_device_banded against the textbook (tests/banded_textbook.py) on random geometries, bands, parameter sets and
overhang strategies: every output of every pair.  Not a test: prints the pairs run and the mismatches (expected 0).

  python scripts/banded_fuzz.py --seconds 120 --seed 1
"""
import argparse, os, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import banded_textbook as bt
from mgl_amd.smithwaterman import MicrosoftSmithWaterman

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=120)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--max-len", type=int, default=700)
args = ap.parse_args()
rng = np.random.default_rng(args.seed)
a = MicrosoftSmithWaterman(0)
ALPHA = [np.frombuffer(x, np.uint8) for x in (b"ACGT", b"AC", b"A", b"ACGTN")]


def pair(tl, ql):
    al = ALPHA[rng.integers(len(ALPHA))]
    t = al[rng.integers(len(al), size=tl)]
    if rng.random() < 0.3:
        return t.tobytes(), al[rng.integers(len(al), size=ql)].tobytes()
    q, rate = [], rng.choice((0.01, 0.05, 0.15))
    for ch in t:
        r = rng.random()
        if r < rate:
            continue
        if r < 2 * rate:
            q.extend(al[rng.integers(len(al), size=int(rng.integers(1, 6)))])
        q.append(al[rng.integers(len(al))] if rng.random() < rate else ch)
    q = (q + list(al[rng.integers(len(al), size=ql)]))[:ql]
    return t.tobytes(), np.array(q, np.uint8).tobytes()


pairs = bad = calls = 0
t0 = time.time()
while time.time() - t0 < args.seconds:
    params = (int(rng.integers(0, 300)), -int(rng.integers(0, 300)), int(rng.integers(0, 400)), int(rng.integers(0, 40)))
    strategy = (1, 2, 4, 8)[rng.integers(4)]
    band = int(rng.choice((0, 1, 2, 3, 8, 30, 63, 64, 65, 130, 400, 5000)))
    top = int(rng.choice((20, 70, 200, args.max_len)))
    ts, qs = zip(*[pair(int(rng.integers(1, top + 1)), int(rng.integers(1, top + 1))) for _ in range(int(rng.integers(1, 80)))])
    # (a CIGAR has at most two characters per base it consumes, beside the clips)
    stride = 2 * (max(len(t) for t in ts) + max(len(q) for q in qs)) + 32
    res, st = a.align_banded(list(ts), list(qs), band, params, strategy, cigar_stride=stride, return_status=True)
    calls += 1
    for k, (t, q) in enumerate(zip(ts, qs)):
        f = bt.banded_align if len(t) * len(q) <= 3000 else bt.banded_align_np
        off, ez, cigar = f(t, q, *params, strategy, band)
        got = (int(st[k]), int(res.offsets[k]), tuple(int(x) for x in res.scores[k]), res.cigars[k])
        pairs += 1
        if got != (0, off, tuple(ez), cigar):
            bad += 1
            if bad <= 5:
                print("MISMATCH", t, q, params, strategy, band, got, (off, ez, cigar), flush=True)
print(f"banded_fuzz seed {args.seed}: {pairs} pairs in {calls} calls, {bad} mismatches", flush=True)
sys.exit(1 if bad else 0)
