"""mgl_sw_extend_batch_device with MGL_SW_FLAG_EXTEND_ADAPTIVE_BAND against the textbook (tests/extend_adaptive_textbook.py) on random
geometries, bands, Z-drop thresholds, parameter sets and both start modes: every output of every pair.  Not a test: prints the pairs
run, how many of them moved their band, and the mismatches (expected 0).

  python scripts/extend_adaptive_fuzz.py --seconds 60 --seed 1
"""
import argparse, os, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import extend_adaptive_textbook as at
import extend_textbook as et
from mgl_amd.smithwaterman import MicrosoftSmithWaterman

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=60)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--max-len", type=int, default=700)
args = ap.parse_args()
rng = np.random.default_rng(args.seed)
a = MicrosoftSmithWaterman(0)
ALPHA = [np.frombuffer(x, np.uint8) for x in (b"ACGT", b"AC", b"A", b"ACGTN")]


def pair(tl, ql):
    """a noisy copy, an unrelated pair, or a noisy copy whose tail is unrelated (what the Z-drop rule is for)"""
    al = ALPHA[rng.integers(len(ALPHA))]
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


pairs = bad = calls = dropped = moved = 0
t0 = time.time()
while time.time() - t0 < args.seconds:
    params = (int(rng.integers(0, 300)), -int(rng.integers(0, 300)), int(rng.integers(0, 400)), int(rng.integers(0, 40)))
    band = int(rng.choice((0, 1, 2, 3, 8, 30, 63, 64, 65, 130, 400, 1000)))
    zdrop = int(rng.choice((-1, 0, params[3], 2 * params[2] + 1, 10 * params[0] + 50, 400 * max(params[3], 1), 1 << 30)))
    to_qend = bool(rng.integers(2))
    top = int(rng.choice((20, 70, 200, args.max_len)))
    ts, qs = zip(*[pair(int(rng.integers(1, top + 1)), int(rng.integers(1, top + 1))) for _ in range(int(rng.integers(1, 80)))])
    stride = 2 * (max(len(t) for t in ts) + max(len(q) for q in qs)) + 32  # (a CIGAR has at most two characters per base it consumes)
    res, st = a.extend(list(ts), list(qs), band, zdrop, params, to_qend, cigar_stride=stride, return_status=True, adaptive_band=True)
    calls += 1
    for k, (t, q) in enumerate(zip(ts, qs)):
        f = at.extend_adaptive_align if len(t) * min(len(q), 2 * band + 1) <= 3000 else at.extend_adaptive_align_np
        centres = []
        ext, cigar = f(t, q, *params, band, zdrop, to_qend, centres=centres)
        moved += len(set(centres)) > 1
        got = (int(st[k]), et.Ext(*(int(res[c][k]) for c in range(8))), res.cigars[k], int(res.cigar_len[k]))
        pairs += 1
        dropped += ext.dropped
        if got != (0, ext, cigar, len(cigar)):
            bad += 1
            if bad <= 5:
                print("MISMATCH", t, q, params, band, zdrop, to_qend, got, (ext, cigar), flush=True)
print(f"extend_adaptive_fuzz seed {args.seed}: {pairs} pairs ({dropped} dropped, {moved} with a band that moved) in {calls} calls, {bad} mismatches", flush=True)
sys.exit(1 if bad else 0)
