"""mgl_sw_extend_seed_batch_device next to what a caller had to do before it: --pairs pairs, each a ~10 kb window with a 50-base exact
seed near its middle, the flanks on either side made by the generator of scripts/extend_adaptive_bench.py (5 % substitutions, 1 % + 1 %
indels of 1 .. 3 bases, --jumps insertions of --jump bases per flank; restated here: that script runs on import), band 512 fixed, Z-drop
off, GATK parameters, 32 distinct pairs cycled.  Two lines in ONE run, on the same pairs:

  (a) two mgl_sw_extend_batch_device calls on the four flanks, split and (the left ones) reversed BEFORE the timed region; no join
  (b) mgl_sw_extend_seed_batch_device on the unsplit inputs: split, reversed copies, both extensions, seed score and joined CIGAR

(b) does strictly more than (a).  Before the timing, (b)'s score must be (a)'s left score + the seed's + (a)'s right score for every
pair.  A warm-up pass of each, then passes of (a) and (b) in turn until each has --seconds of GPU time (events around the
calls).

  python scripts/seed_extend_bench.py --pairs 2048 --seconds 15
"""
import argparse, json, os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=2048)
ap.add_argument("--length", type=int, default=10000)
ap.add_argument("--seed-len", type=int, default=50)
ap.add_argument("--band", type=int, default=512)
ap.add_argument("--seconds", type=float, default=15)
ap.add_argument("--distinct", type=int, default=32, help="distinct synthetic pairs (the batch cycles through them)")
ap.add_argument("--jumps", type=int, default=5)
ap.add_argument("--jump", type=int, default=30)
args = ap.parse_args()
n = args.pairs
ACGT = np.frombuffer(b"ACGT", np.uint8)


def make_flank(rng, length):
    """scripts/extend_adaptive_bench.py's make_pair at `length` bases"""
    t = ACGT[rng.integers(4, size=length)]
    jumps = {(length // (args.jumps + 1)) * (x + 1) + 11 * x for x in range(args.jumps)}
    q, skip = [], 0
    for pos, ch in enumerate(t):
        if pos in jumps:
            q.extend(ACGT[rng.integers(4, size=args.jump)])
        if skip:
            skip -= 1
            continue
        r = rng.random()
        if r < 0.01:
            skip = int(rng.integers(0, 3))
            continue
        if r < 0.02:
            q.extend(ACGT[rng.integers(4, size=int(rng.integers(1, 4)))])
        q.append(ACGT[rng.integers(4)] if rng.random() < 0.05 else ch)
    return t.tobytes(), np.array(q, np.uint8).tobytes()


rng = np.random.default_rng(43)
base = []
for k in range(min(n, args.distinct)):
    left_len = (args.length - args.seed_len) // 2 + int(rng.integers(-200, 201))  # near the middle
    (lt, lq), (rt, rq) = make_flank(rng, left_len), make_flank(rng, args.length - args.seed_len - left_len)
    seed = ACGT[rng.integers(4, size=args.seed_len)].tobytes()
    base.append((lt[::-1] + seed + rt, lq[::-1] + seed + rq, (len(lt), len(lq), args.seed_len)))

import torch
from mgl_amd.smithwaterman import MicrosoftSmithWaterman, GATK_PARAMETERS, concat

pick = [base[k % len(base)] for k in range(n)]
Ts, Qs, seeds = [p[0] for p in pick], [p[1] for p in pick], np.array([p[2] for p in pick], np.int32)
dev = torch.device("cuda", 0)
a = MicrosoftSmithWaterman(0)
g = lambda x, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(x).astype(dt))).to(dev)  # noqa: E731


def device(seqs):
    d, off = concat(seqs)
    ln = np.diff(off)
    return (g(np.concatenate([d, np.zeros(8, np.uint8)]), np.uint8), g(off[:-1], np.int64), g(ln, np.int32)), int(ln.max())


def timed(calls):
    """a warm-up pass of each, then passes of the calls in turn until each has args.seconds of GPU time: (seconds per pass, passes) each"""
    for call in calls:
        call()
    torch.cuda.synchronize()
    total, reps = [0.0] * len(calls), [0] * len(calls)
    while min(total) < args.seconds:
        for x, call in enumerate(calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); call(); e1.record(); torch.cuda.synchronize()
            total[x] += e0.elapsed_time(e1) * 1e-3
            reps[x] += 1
    return [(t / r, r) for t, r in zip(total, reps)]


def outputs(stride, records):
    return tuple(torch.zeros((n, 8), dtype=torch.int32, device=dev) for _ in range(records)) + (
        torch.zeros(n * stride, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev))


# ---- (a): the flanks as a caller cuts them, before the timed region
(T, max_tl), (Q, max_ql) = device(Ts), device(Qs)
(LT, max_lt), (LQ, max_lq) = device([t[:s[0]][::-1] for t, s in zip(Ts, seeds)]), device([q[:s[1]][::-1] for q, s in zip(Qs, seeds)])
(RT, max_rt), (RQ, max_rq) = device([t[s[0] + s[2]:] for t, s in zip(Ts, seeds)]), device([q[s[1] + s[2]:] for q, s in zip(Qs, seeds)])
side_stride, stride = 2 * (args.length // 2 + 1500), 2 * (args.length + 2000)
out_l, out_r, out_b = outputs(side_stride, 1), outputs(side_stride, 1), outputs(stride, 3)
sd = [g(seeds[:, c], np.int32) for c in range(3)]


def call_a():
    a.extend_device(*LT, *LQ, max_lt, max_lq, args.band, -1, GATK_PARAMETERS, False, side_stride, False, False, out=out_l)
    a.extend_device(*RT, *RQ, max_rt, max_rq, args.band, -1, GATK_PARAMETERS, False, side_stride, False, False, out=out_r)


def call_b():
    a.extend_seed_device(*T, *Q, *sd, max_tl, max_ql, args.band, -1, GATK_PARAMETERS, False, stride, False, False, out=out_b, sides=True)


call_a(); call_b(); torch.cuda.synchronize()
assert int((out_l[3] != 0).sum()) == int((out_r[3] != 0).sum()) == int((out_b[5] != 0).sum()) == 0
assert bool((out_b[0][:, 0] == out_l[0][:, 0] + 200 * args.seed_len + out_r[0][:, 0]).all()) and bool((out_b[1] == out_l[0]).all()) and bool((out_b[2] == out_r[0]).all())
span = (out_b[0][:, 2] - out_b[0][:, 1]).float().mean().item()
names = ("(a) two extend calls on pre-split flanks", "(b) extend_seed on the unsplit inputs")
rows = []
for name, (sec, reps) in zip(names, timed((call_a, call_b))):
    rows.append({"line": name, "band": args.band, "pairs": n, "pairs_per_s": round(n / sec, 1), "us_per_pair": round(sec / n * 1e6, 2),
                 "ms_per_pass": round(sec * 1e3, 2), "passes": reps, "mean_target_span": round(span, 1)})
rows[1]["pairs_per_s_vs_a"] = round(rows[1]["pairs_per_s"] / rows[0]["pairs_per_s"], 4)
for row in rows:
    print(json.dumps(row), flush=True)
