"""What secondary chains and a mapping quality cost the read mapper: section 9j's workload -- --reads reads of
mgl_amd.synth.mapping_set (about 10 kb; --distinct of them laid into one reference, the batch cycles through them), every odd read
reverse-complemented; (k, w) = (15, 10), max_occ 8, max_occ_ref 64, merged; GATK parameters, band 64, Z-drop off, to the query's end;
section 9i's chaining parameters; max_chains 4, min_score 40, min_cnt 3, mask_level 128.  With --copies C the windows of the first C distinct
reads stand a second time in the reference (synth.repeat_mapping_set at --divergence).  Lines in ONE run, in turn after a warm-up each:

  (a)  map_reads_device -- the parent's path and the yardstick
  (b)  map_reads_ranked_device
  (c)  chain_anchors_device alone on (a)'s candidates, and (c') the same with f and pred written
  (d)  rank_chains_device alone on (c')'s f and pred, and (d') the same with the anchor outputs

Printed per line: reads/s over all passes, the median pass and the spread -- the fastest and the slowest pass against the median pass; for
(b) its time against (a)'s; and of the reads whose window has a copy the share with mapq 0, of the others the share with mapq 60.

  python scripts/rank_bench.py --reads 2048 --distinct 2048 --seconds 10
"""
import argparse, json, os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=2048)
ap.add_argument("--length", type=int, default=10000)
ap.add_argument("--spacer", type=int, default=3000)
ap.add_argument("--band", type=int, default=64)
ap.add_argument("--seconds", type=float, default=10)
ap.add_argument("--distinct", type=int, default=128, help="distinct reads and places in the reference (the batch cycles through them)")
ap.add_argument("--copies", type=int, default=0, help="the windows of this many of the distinct reads stand twice in the reference")
ap.add_argument("--divergence", type=float, default=0.0)
ap.add_argument("-k", type=int, default=15)
ap.add_argument("-w", type=int, default=10)
ap.add_argument("--max-occ", type=int, default=8)
ap.add_argument("--max-occ-ref", type=int, default=64)
ap.add_argument("--max-cand", type=int, default=2048)
ap.add_argument("--slack", type=int, default=200)
ap.add_argument("--max-dist", type=int, default=1000)
ap.add_argument("--max-chains", type=int, default=4)
ap.add_argument("--min-score", type=int, default=40)
ap.add_argument("--min-cnt", type=int, default=3)
ap.add_argument("--mask-level", type=int, default=128)
args = ap.parse_args()
n = args.reads

import torch
from mgl_amd import synth
from mgl_amd.smithwaterman import MicrosoftSmithWaterman, GATK_PARAMETERS, concat

distinct = min(n, args.distinct)
ref, base_reads, base_truth, copy = synth.repeat_mapping_set(43, distinct, args.length, args.spacer, args.copies, args.divergence)
reads = [base_reads[i % distinct] for i in range(n)]
copied = np.array([i % distinct < args.copies for i in range(n)])
dev = torch.device("cuda", 0)
a = MicrosoftSmithWaterman(0)
g = lambda x, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(x).astype(dt))).to(dev)  # noqa: E731
d, off = concat(reads)
ln = np.diff(off)
Q, max_ql = (g(np.concatenate([d, np.zeros(8, np.uint8)]), np.uint8), g(off[:-1], np.int64), g(ln, np.int32)), int(ln.max())
ref_dev = g(np.concatenate([np.frombuffer(ref, np.uint8), np.zeros(8, np.uint8)]), np.uint8)[:len(ref)]
index = a.build_index(ref_dev, args.k, args.w)
map_tl = max(len(ref[p:p + m]) for p, m, _ in base_truth) + 2 * args.slack + 500
stride = 2 * (args.length + 2000)
index_par = (2, args.max_occ, args.max_occ_ref, True, args.max_cand)
chain_par = dict(max_pred=64, max_dist=args.max_dist, bw=500, pen_gap=38, pen_skip=0)
rank_par = (args.max_chains, args.min_score, args.min_cnt, args.mask_level)
i32 = lambda m: torch.zeros(m, dtype=torch.int32, device=dev)  # noqa: E731
i64 = lambda m: torch.zeros(m, dtype=torch.int64, device=dev)  # noqa: E731
aligned = lambda: (torch.zeros((n, 8), dtype=torch.int32, device=dev), None, None, None, torch.zeros(n * stride, dtype=torch.uint8, device=dev), i32(n), i32(n))  # noqa: E731

# the seed stage once at a capacity that surely holds the batch, to size the arrays of the timed calls by what it found
first = a.seed_index_device(index, *Q, *index_par)
torch.cuda.synchronize()
assert int((first[6] != 0).sum()) == 0, "a row was refused: raise --max-cand"
total = int(first[0][2 * n].item())
del first
rows = lambda: (i64(2 * n + 1), i32(total), i32(total), i32(total), i32(2 * n), i32(2 * n), i32(2 * n))  # noqa: E731
chains = lambda dp: (i64(2 * n + 1), i32(total), i32(total), i32(total), i32(2 * n), i32(total) if dp else None, i32(total) if dp else None, i32(2 * n))  # noqa: E731
chosen = lambda: (i32(n), torch.zeros_like(Q[0]), i64(n + 1), i32(total), i32(total), i32(total), i32(n), i32(n))  # noqa: E731
located = lambda: (i64(n), i32(n), i32(total), i32(n))  # noqa: E731
ranked = lambda anchors: (i32(n), torch.zeros((n, args.max_chains, 12), dtype=torch.int32, device=dev), i64(n + 1) if anchors else None,  # noqa: E731
                          *((i32(total) if anchors else None) for _ in range(3)), i32(n))
seed_a, seed_b = rows(), rows()
chain_a, chain_b, chain_c, chain_c2 = chains(False), chains(True), chains(False), chains(True)
pick_a, pick_b, where_a, where_b, out_a, out_b = chosen(), chosen(), located(), located(), aligned(), aligned()
rank_b, rank_d, rank_d2 = ranked(False), ranked(False), ranked(True)
align = dict(to_query_end=True, cigar_stride=stride)


def call_a():
    a.map_reads_device(index, *Q, map_tl, max_ql, args.band, -1, GATK_PARAMETERS, args.slack, *index_par, total, seed_out=seed_a, chain_out=chain_a,
                       select_out=pick_a, locate_out=where_a, out=out_a, **chain_par, **align)


def call_b():
    a.map_reads_ranked_device(index, *Q, map_tl, max_ql, args.band, -1, GATK_PARAMETERS, 2, args.max_cand, total, seed_b, chain_b, *rank_par, rank_out=rank_b,
                              slack=args.slack, max_occ=args.max_occ, max_occ_ref=args.max_occ_ref, merge=True, select_out=pick_b, locate_out=where_b, out=out_b,
                              **chain_par, **align)


def call_c():
    a.chain_anchors_device(seed_a[4], seed_a[5], *seed_a[:4], args.max_cand, out=chain_c, **chain_par)


def call_c2():
    a.chain_anchors_device(seed_a[4], seed_a[5], *seed_a[:4], args.max_cand, out=chain_c2, **chain_par)


def call_d():
    a.rank_chains_device(seed_a[5], *seed_a[:4], chain_c2[5], chain_c2[6], chain_c2[7], 2, args.max_cand, *rank_par, out=rank_d)


def call_d2():
    a.rank_chains_device(seed_a[5], *seed_a[:4], chain_c2[5], chain_c2[6], chain_c2[7], 2, args.max_cand, *rank_par, out=rank_d2)


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


call_a(); call_b(); torch.cuda.synchronize()
assert int((seed_b[6] != 0).sum()) == int((pick_b[7] != 0).sum()) == int((rank_b[6] != 0).sum()) == 0
assert all(bool((x == y).all()) for x, y in zip((out_a[0], out_a[5], out_a[6], pick_a[0]), (out_b[0], out_b[5], out_b[6], pick_b[0]))), "the alignment changed"
n_chains, rec = rank_b[0].cpu().numpy(), rank_b[1].cpu().numpy()
mapq = np.where(n_chains > 0, rec[:, 0, 10], 0)
names = ("(a) map_reads_device", "(b) map_reads_ranked_device", "(c) chain_anchors_device alone", "(c') chain_anchors_device alone, f and pred written",
         "(d) rank_chains_device alone", "(d') rank_chains_device alone, anchors written")
out = []
for name, secs in zip(names, timed((call_a, call_b, call_c, call_c2, call_d, call_d2))):
    s = np.sort(np.array(secs))
    med = float(np.median(s))
    out.append({"line": name, "reads": n, "reads_per_s": round(n * len(s) / float(s.sum()), 1), "us_per_read": round(float(s.sum()) / len(s) / n * 1e6, 3),
                "ms_per_pass_median": round(med * 1e3, 4), "passes": len(s), "spread_pct": [round((s[0] / med - 1) * 100, 2), round((s[-1] / med - 1) * 100, 2)]})
out[0].update({"distinct": distinct, "copies": args.copies, "divergence": args.divergence, "ref_len": len(ref), "candidates_per_read_both_rows": round(total / n, 1)})
out[1].update({"ms_median_vs_a": round(out[1]["ms_per_pass_median"] / out[0]["ms_per_pass_median"], 4), "chains_per_read": round(float(n_chains.mean()), 3),
               "copied_reads": int(copied.sum()), "copied_with_mapq_0": round(float((mapq[copied] == 0).mean()), 4) if copied.any() else None,
               "others_with_mapq_60": round(float((mapq[~copied] == 60).mean()), 4) if (~copied).any() else None})
for row in out:
    print(json.dumps(row), flush=True)
index.close()
