"""Reads -> seeds -> chain -> alignment next to the same without the seed stage: --pairs pairs of DESIGN.md section 9g's kind (about 10 kb, a
true 20-base anchor about every 200 bases; mgl_amd.synth.chain_pairs, 32 distinct pairs cycled), seeded with (k, w) = (15, 10), max_occ 8,
merged; GATK parameters, band 64, Z-drop off, to the query's end; section 9g's chaining parameters.  Three lines in ONE run, on the same
pairs, in turn after a warm-up each:

  (a) align_candidates_device on the seed stage's own output, left on the device by an earlier call -- the yardstick
  (b) align_reads_device: seed_device, then align_candidates_device on what it wrote
  (c) seed_device alone

Printed per line: pairs/s over all passes, the median pass and the spread -- the fastest and the slowest pass against the median pass; for
(b) its rate against (a)'s, the candidates per pair and the share of pairs whose alignment score equals that of align_chain_device on the
generator's true anchors.

  python scripts/seed_bench.py --pairs 2048 --seconds 10
"""
import argparse, json, os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=2048)
ap.add_argument("--length", type=int, default=10000)
ap.add_argument("--band", type=int, default=64)
ap.add_argument("--seconds", type=float, default=10)
ap.add_argument("--distinct", type=int, default=32, help="distinct synthetic pairs (the batch cycles through them)")
ap.add_argument("-k", type=int, default=15)
ap.add_argument("-w", type=int, default=10)
ap.add_argument("--max-occ", type=int, default=8)
ap.add_argument("--no-merge", action="store_true")
ap.add_argument("--max-cand", type=int, default=2048, help="the bound on a pair's raw hits")
ap.add_argument("--max-pred", type=int, default=64)
ap.add_argument("--max-dist", type=int, default=1000, help="also the chain entry's gap bounds, which size its rows: 8 max_dist bytes per candidate")
ap.add_argument("--bw", type=int, default=500)
ap.add_argument("--pen-gap", type=int, default=38)
ap.add_argument("--pen-skip", type=int, default=0)
args = ap.parse_args()
n = args.pairs

import torch
from mgl_amd import synth
from mgl_amd.smithwaterman import MicrosoftSmithWaterman, GATK_PARAMETERS, concat

base = synth.chain_pairs(43, min(n, args.distinct), args.length)
pick = [base[i % len(base)] for i in range(n)]
Ts, Qs, chains = ([p[c] for p in pick] for c in range(3))
dev = torch.device("cuda", 0)
a = MicrosoftSmithWaterman(0)
g = lambda x, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(x).astype(dt))).to(dev)  # noqa: E731


def device(seqs):
    d, off = concat(seqs)
    ln = np.diff(off)
    return (g(np.concatenate([d, np.zeros(8, np.uint8)]), np.uint8), g(off[:-1], np.int64), g(ln, np.int32)), int(ln.max())


def timed(calls):
    """a warm-up pass of each, then passes of the calls in turn until the first has args.seconds of GPU time: the seconds of every pass, per call"""
    for call in calls:
        call()
    torch.cuda.synchronize()
    secs = [[] for _ in calls]
    while sum(secs[0]) < args.seconds:
        for x, call in enumerate(calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); call(); e1.record(); torch.cuda.synchronize()
            secs[x].append(e0.elapsed_time(e1) * 1e-3)
    return secs


(T, max_tl), (Q, max_ql) = device(Ts), device(Qs)
stride = 2 * (args.length + 2000)
seed_par = (args.k, args.w, args.max_occ, not args.no_merge, args.max_cand)
chain_par = dict(max_pred=args.max_pred, max_dist=args.max_dist, bw=args.bw, pen_gap=args.pen_gap, pen_skip=args.pen_skip)
i32 = lambda m: torch.zeros(m, dtype=torch.int32, device=dev)  # noqa: E731
rec = lambda: torch.zeros((n, 8), dtype=torch.int32, device=dev)  # noqa: E731
tail = lambda: (torch.zeros(n * stride, dtype=torch.uint8, device=dev), i32(n), i32(n))  # noqa: E731

# the seed stage once at a capacity that surely holds the batch, to size the arrays of the timed calls by what it found
first = a.seed_device(*T, *Q, *seed_par)
torch.cuda.synchronize()
assert int((first[4] != 0).sum()) == 0, "a pair was refused: raise --max-cand"
total = int(first[0][n].item())
counts = (first[0][1:] - first[0][:-1])
del first
seeds = lambda: (torch.zeros(n + 1, dtype=torch.int64, device=dev), i32(total), i32(total), i32(total), i32(n))  # noqa: E731
kept, seed_b, seed_c = seeds(), seeds(), seeds()
a.seed_device(*T, *Q, *seed_par, total, out=kept)  # (a)'s candidates: they stay on the device
chain = lambda: (torch.zeros(n + 1, dtype=torch.int64, device=dev), i32(total), i32(total), i32(total), i32(n), None, None, i32(n))  # noqa: E731
chain_a, chain_b = chain(), chain()
out_a, out_b, out_true = ((rec(), None, None, None) + tail() for _ in range(3))
align = dict(chain_par, to_query_end=True, cigar_stride=stride)


def call_a():
    a.align_candidates_device(*T, *Q, *kept[:4], max_tl, max_ql, args.max_cand, args.band, -1, GATK_PARAMETERS, chain_out=chain_a, out=out_a, **align)


def call_b():
    a.align_reads_device(*T, *Q, max_tl, max_ql, args.band, -1, GATK_PARAMETERS, *seed_par, total, seed_out=seed_b, chain_out=chain_b, out=out_b, **align)


def call_c():
    a.seed_device(*T, *Q, *seed_par, total, out=seed_c)


# the generator's true anchors through align_chain_device: what (b)'s scores are held against
flat = np.array([x for c in chains for x in c], np.int32)
true = [g(np.concatenate([[0], np.cumsum([len(c) for c in chains])]), np.int64)] + [g(flat[:, c], np.int32) for c in range(3)]
gaps = [(nt - st - sl, nq - sq - sl) for c in chains for (st, sq, sl), (nt, nq, _) in zip(c, c[1:])]
a.align_chain_device(*T, *Q, *true, max_tl, max_ql, max(x for x, _ in gaps), max(y for _, y in gaps), args.band, -1, GATK_PARAMETERS, True, stride, False, False,
                     out=out_true)
call_a(); call_b(); torch.cuda.synchronize()
assert int((out_a[6] != 0).sum()) == int((out_b[6] != 0).sum()) == int((out_true[6] != 0).sum()) == int((seed_b[4] != 0).sum()) == 0
assert all(bool((x == y).all()) for x, y in zip(kept, seed_b)) and bool((out_a[0] == out_b[0]).all())
agree = float((out_true[0][:, 0] == out_b[0][:, 0]).float().mean().item())
chain_len = float(chain_b[0][n].item()) / n
names = ("(a) align_candidates on the seed stage's output", "(b) align_reads", "(c) seed alone")
rows = []
for name, secs in zip(names, timed((call_a, call_b, call_c))):
    s = np.sort(np.array(secs))
    med = float(np.median(s))
    rows.append({"line": name, "pairs": n, "pairs_per_s": round(n * len(s) / float(s.sum()), 1), "us_per_pair": round(float(s.sum()) / len(s) / n * 1e6, 2),
                 "ms_per_pass_median": round(med * 1e3, 3), "passes": len(s), "spread_pct": [round((s[0] / med - 1) * 100, 2), round((s[-1] / med - 1) * 100, 2)]})
rows[0].update({"band": args.band, "k": args.k, "w": args.w, "max_occ": args.max_occ, "merge": not args.no_merge, "max_cand": args.max_cand})
rows[1].update({"pairs_per_s_vs_a": round(rows[1]["pairs_per_s"] / rows[0]["pairs_per_s"], 4), "candidates_per_pair": round(total / n, 1),
                "candidates_per_pair_range": [int(counts.min().item()), int(counts.max().item())], "chained_per_pair": round(chain_len, 1),
                "scores_equal_true_anchors": round(agree, 4)})
rows[2].update({"bases_per_s": round(rows[2]["pairs_per_s"] * float(sum(len(t) + len(q) for t, q in zip(Ts, Qs))) / n, 1)})
for row in rows:
    print(json.dumps(row), flush=True)
