"""mgl_sw_align_chain_batch_device next to what a caller had before it: --pairs pairs, each a ~10 kb window made by the generator of
scripts/seed_extend_bench.py (5 % substitutions, 1 % + 1 % indels of 1 .. 3 bases, --jumps insertions of --jump bases per flank, a
50-base exact seed near the middle; restated here: that script runs on import) with one change: about every --every target bases --anchor
bases are copied exactly, and the generator, which knows where they went, records them as anchors.  GATK parameters, Z-drop off, to the
query's end, 32 distinct pairs cycled.  Two lines in ONE run, on the same pairs, in turn after an equal warm-up:

  (a) mgl_sw_extend_seed_batch_device from the middle anchor (the seed) at --seed-band (512): the band absorbs all drift
  (b) mgl_sw_align_chain_batch_device through all anchors at --band (64)

Printed per line: pairs/s over all passes, and the spread -- the slowest and the fastest pass against the median pass; and once the
share of pairs whose two scores agree (they are different functions: (a) is free to leave the anchors, (b) is not limited by drift).

  python scripts/chain_align_bench.py --pairs 2048 --seconds 10
"""
import argparse, json, os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=2048)
ap.add_argument("--length", type=int, default=10000)
ap.add_argument("--seed-len", type=int, default=50)
ap.add_argument("--seed-band", type=int, default=512)
ap.add_argument("--band", type=int, default=64)
ap.add_argument("--every", type=int, default=200)
ap.add_argument("--anchor", type=int, default=20)
ap.add_argument("--seconds", type=float, default=10)
ap.add_argument("--distinct", type=int, default=32, help="distinct synthetic pairs (the batch cycles through them)")
ap.add_argument("--jumps", type=int, default=5)
ap.add_argument("--jump", type=int, default=30)
args = ap.parse_args()
n = args.pairs
ACGT = np.frombuffer(b"ACGT", np.uint8)


def make_flank(rng, length):
    """scripts/seed_extend_bench.py's make_flank with exact stretches: -> (t, q, [(start in t, start in q)] of the stretches)"""
    t = ACGT[rng.integers(4, size=length)]
    jumps = {(length // (args.jumps + 1)) * (x + 1) + 11 * x for x in range(args.jumps)}
    q, skip, exact, marks, pending = [], 0, 0, [], False
    for pos, ch in enumerate(t):
        pending = pending or pos in jumps
        if pending and not exact:  # (a jump that falls into an exact stretch comes behind it)
            q.extend(ACGT[rng.integers(4, size=args.jump)])
            pending = False
        if pos % args.every == args.every // 2 and pos + args.anchor <= length and not skip:
            exact = args.anchor
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
            q.extend(ACGT[rng.integers(4, size=int(rng.integers(1, 4)))])
        q.append(ACGT[rng.integers(4)] if rng.random() < 0.05 else ch)
    return t.tobytes(), np.array(q, np.uint8).tobytes(), marks


rng = np.random.default_rng(43)
base = []
for k in range(min(n, args.distinct)):
    left_len = (args.length - args.seed_len) // 2 + int(rng.integers(-200, 201))  # near the middle
    (lt, lq, lm), (rt, rq, rm) = make_flank(rng, left_len), make_flank(rng, args.length - args.seed_len - left_len)
    seed = ACGT[rng.integers(4, size=args.seed_len)].tobytes()
    # the left flank was made outwards from the seed and is laid down reversed: a stretch at (u, v) lies at (len - u - anchor, ...)
    chain = sorted((len(lt) - u - args.anchor, len(lq) - v - args.anchor, args.anchor) for u, v in lm)
    chain.append((len(lt), len(lq), args.seed_len))
    chain += [(len(lt) + args.seed_len + u, len(lq) + args.seed_len + v, args.anchor) for u, v in rm]
    T, Q = lt[::-1] + seed + rt, lq[::-1] + seed + rq
    assert all(T[a:a + l] == Q[b:b + l] for a, b, l in chain)
    base.append((T, Q, (len(lt), len(lq), args.seed_len), chain))

import torch
from mgl_amd.smithwaterman import MicrosoftSmithWaterman, GATK_PARAMETERS, concat

pick = [base[k % len(base)] for k in range(n)]
Ts, Qs, seeds, chains = [p[0] for p in pick], [p[1] for p in pick], np.array([p[2] for p in pick], np.int32), [p[3] for p in pick]
dev = torch.device("cuda", 0)
a = MicrosoftSmithWaterman(0)
g = lambda x, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(x).astype(dt))).to(dev)  # noqa: E731


def device(seqs):
    d, off = concat(seqs)
    ln = np.diff(off)
    return (g(np.concatenate([d, np.zeros(8, np.uint8)]), np.uint8), g(off[:-1], np.int64), g(ln, np.int32)), int(ln.max())


def timed(calls):
    """a warm-up pass of each, then passes of the calls in turn until each has args.seconds of GPU time: the seconds of every pass, per call"""
    for call in calls:
        call()
    torch.cuda.synchronize()
    secs = [[] for _ in calls]
    while min(sum(s) for s in secs) < args.seconds:
        for x, call in enumerate(calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); call(); e1.record(); torch.cuda.synchronize()
            secs[x].append(e0.elapsed_time(e1) * 1e-3)
    return secs


(T, max_tl), (Q, max_ql) = device(Ts), device(Qs)
stride = 2 * (args.length + 2000)
rec = lambda: torch.zeros((n, 8), dtype=torch.int32, device=dev)  # noqa: E731
tail = lambda: (torch.zeros(n * stride, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev))  # noqa: E731
out_a = (rec(), None, None) + tail()
sd = [g(seeds[:, c], np.int32) for c in range(3)]
flat = np.array([x for c in chains for x in c], np.int32)
start = np.concatenate([[0], np.cumsum([len(c) for c in chains])])
gaps = [(nt - st - sl, nq - sq - sl) for c in chains for (st, sq, sl), (nt, nq, _) in zip(c, c[1:])]
max_gap = (max(x for x, _ in gaps), max(y for _, y in gaps))
out_b = (rec(), None, None, None) + tail()
ch = [g(start, np.int64)] + [g(flat[:, c], np.int32) for c in range(3)]


def call_a():
    a.extend_seed_device(*T, *Q, *sd, max_tl, max_ql, args.seed_band, -1, GATK_PARAMETERS, True, stride, False, False, out=out_a)


def call_b():
    a.align_chain_device(*T, *Q, *ch, max_tl, max_ql, max_gap[0], max_gap[1], args.band, -1, GATK_PARAMETERS, True, stride, False, False, out=out_b)


call_a(); call_b(); torch.cuda.synchronize()
assert int((out_a[5] != 0).sum()) == int((out_b[6] != 0).sum()) == 0
agree = float((out_a[0][:, 0] == out_b[0][:, 0]).float().mean().item())
chain_better = float((out_b[0][:, 0] > out_a[0][:, 0]).float().mean().item())
cells_a = sum(len(t) * min(len(q), 2 * args.seed_band + 1) for t, q in zip(Ts, Qs)) / n
names = ("(a) extend_seed from the middle anchor", "(b) align_chain through all anchors")
rows = []
for name, band, secs in zip(names, (args.seed_band, args.band), timed((call_a, call_b))):
    s = np.sort(np.array(secs))
    med = float(np.median(s))
    rows.append({"line": name, "band": band, "pairs": n, "pairs_per_s": round(n * len(s) / float(s.sum()), 1), "us_per_pair": round(float(s.sum()) / len(s) / n * 1e6, 2),
                 "ms_per_pass_median": round(med * 1e3, 2), "passes": len(s), "spread_pct": [round((s[0] / med - 1) * 100, 2), round((s[-1] / med - 1) * 100, 2)]})
rows[1]["pairs_per_s_vs_a"] = round(rows[1]["pairs_per_s"] / rows[0]["pairs_per_s"], 4)
rows[1].update({"anchors_per_pair": round(len(flat) / n, 1), "max_gap": list(max_gap), "mean_gap_cells_per_pair": round(sum(x * min(y, 2 * args.band + abs(y - x) + 1) for x, y in gaps) / n),
                "mean_band_cells_per_pair_a": round(cells_a), "scores_agree": round(agree, 4), "chain_score_higher": round(chain_better, 4)})
for row in rows:
    print(json.dumps(row), flush=True)
