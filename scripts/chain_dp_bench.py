"""Candidates -> chain -> alignment next to the alignment of a finished chain: --pairs pairs of DESIGN.md section 9f's kind (about 10 kb, a
true 20-base anchor about every 200 bases; mgl_amd.synth.chain_pairs, 32 distinct pairs cycled) and, per pair, the candidates a seeding
stage would hand over (synth.noisy_candidates: the true anchors, overlapping hits on their diagonal, repeat copies, off-diagonal decoys,
sorted by target position).  GATK parameters, band 64, Z-drop off, to the query's end; minimap2-like chaining parameters, with
max_dist at 1 000: it is also the gap bound the chain entry is given, and that entry stages a CIGAR row of 4 (max_gap_tl + max_gap_ql)
bytes per anchor index -- 14 GB for 356 000 candidates at 5 000.  Three lines
in ONE run, on the same pairs, in turn after a warm-up each:

  (a) align_chain_device on the true anchors, already on the device -- what a caller with a finished chain has
  (b) align_candidates_device from the noisy candidates: chain_anchors_device, then align_chain_device on what it wrote
  (c) chain_anchors_device alone

Printed per line: pairs/s over all passes and the spread -- the fastest and the slowest pass against the median pass; for (b) its rate
against (a)'s and the share of pairs whose alignment score equals (a)'s.

  python scripts/chain_dp_bench.py --pairs 2048 --seconds 10
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

rng = np.random.default_rng(1043)
base = []
for T, Q, chain in synth.chain_pairs(43, min(n, args.distinct), args.length):
    cands, kind = synth.noisy_candidates(rng, len(T), len(Q), chain)
    base.append((T, Q, chain, cands))
pick = [base[k % len(base)] for k in range(n)]
Ts, Qs, chains, cands = ([p[c] for p in pick] for c in range(4))
dev = torch.device("cuda", 0)
a = MicrosoftSmithWaterman(0)
g = lambda x, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(x).astype(dt))).to(dev)  # noqa: E731


def device(seqs):
    d, off = concat(seqs)
    ln = np.diff(off)
    return (g(np.concatenate([d, np.zeros(8, np.uint8)]), np.uint8), g(off[:-1], np.int64), g(ln, np.int32)), int(ln.max())


def csr(lists):
    flat = np.array([x for c in lists for x in c], np.int32)
    start = np.concatenate([[0], np.cumsum([len(c) for c in lists])])
    return [g(start, np.int64)] + [g(flat[:, c], np.int32) for c in range(3)], len(flat)


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
rec = lambda: torch.zeros((n, 8), dtype=torch.int32, device=dev)  # noqa: E731
tail = lambda: (torch.zeros(n * stride, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev))  # noqa: E731
true, total_true = csr(chains)
cand, total_cand = csr(cands)
max_cand = max(len(c) for c in cands)
gaps = [(nt - st - sl, nq - sq - sl) for c in chains for (st, sq, sl), (nt, nq, _) in zip(c, c[1:])]
max_gap = (max(x for x, _ in gaps), max(y for _, y in gaps))
out_a, out_b = (rec(), None, None, None) + tail(), (rec(), None, None, None) + tail()
i32 = lambda k: torch.zeros(k, dtype=torch.int32, device=dev)  # noqa: E731
chain_out = (torch.zeros(n + 1, dtype=torch.int64, device=dev), i32(total_cand), i32(total_cand), i32(total_cand), i32(n), None, None, i32(n))
chain_par = (args.max_pred, args.max_dist, args.bw, args.pen_gap, args.pen_skip)


def call_a():
    a.align_chain_device(*T, *Q, *true, max_tl, max_ql, max_gap[0], max_gap[1], args.band, -1, GATK_PARAMETERS, True, stride, False, False, out=out_a)


def call_b():
    a.align_candidates_device(*T, *Q, *cand, max_tl, max_ql, max_cand, args.band, -1, GATK_PARAMETERS, *chain_par, chain_out=chain_out, to_query_end=True,
                              cigar_stride=stride, out=out_b)


def call_c():
    a.chain_anchors_device(T[2], Q[2], *cand, max_cand, *chain_par, out=chain_out)


call_a(); call_b(); torch.cuda.synchronize()
assert int((out_a[6] != 0).sum()) == int((out_b[6] != 0).sum()) == int((chain_out[7] != 0).sum()) == 0
agree = float((out_a[0][:, 0] == out_b[0][:, 0]).float().mean().item())
chain_len = float(chain_out[0][n].item()) / n
names = ("(a) align_chain on the true anchors", "(b) align_candidates from the noisy candidates", "(c) chain_anchors alone")
rows = []
for name, secs in zip(names, timed((call_a, call_b, call_c))):
    s = np.sort(np.array(secs))
    med = float(np.median(s))
    rows.append({"line": name, "pairs": n, "pairs_per_s": round(n * len(s) / float(s.sum()), 1), "us_per_pair": round(float(s.sum()) / len(s) / n * 1e6, 2),
                 "ms_per_pass_median": round(med * 1e3, 3), "passes": len(s), "spread_pct": [round((s[0] / med - 1) * 100, 2), round((s[-1] / med - 1) * 100, 2)]})
rows[0].update({"band": args.band, "anchors_per_pair": round(total_true / n, 1), "max_gap": list(max_gap)})
rows[1].update({"pairs_per_s_vs_a": round(rows[1]["pairs_per_s"] / rows[0]["pairs_per_s"], 4), "candidates_per_pair": round(total_cand / n, 1), "max_cand": max_cand,
                "chained_per_pair": round(chain_len, 1), "scores_equal_a": round(agree, 4)})
rows[2].update({"candidates_per_s": round(rows[2]["pairs_per_s"] * total_cand / n, 1)})
for row in rows:
    print(json.dumps(row), flush=True)
