"""Reads in, positions out: mapping against a minimizer index of the whole reference next to the same reads
aligned against their TRUE windows, the parent's path.  --reads reads of mgl_amd.synth.mapping_set (about 10 kb, section 9h's noise; --distinct
of them laid into one reference with 3 000 random bases between them, the batch cycles through them), every odd read reverse-complemented;
(k, w) = (15, 10), max_occ 8, max_occ_ref 64, merged; GATK parameters, band 64, Z-drop off, to the query's end; section 9i's chaining
parameters.  Five lines in ONE run, in turn after a warm-up each:

  (a) align_reads_strands_device on the true windows -- the yardstick: the cost when the window is known
  (b) map_reads_device against the index of the whole reference
  (c) seed_index_device alone
  (d) seed_strands_device alone on the true windows -- what (c) replaces
  (e) select_strand_device + locate_window_device alone, on (b)'s chains

Printed per line: reads/s over all passes, the median pass and the spread -- the fastest and the slowest pass against the median pass; for
(b) its time against (a)'s, the share of reads with the true strand and a window that holds the true span, and the shares whose alignment
score also equals (a)'s and is at least (a)'s; for (c) its time against (d)'s; and the index: build time, entries, bytes.

  python scripts/index_bench.py --reads 2048 --seconds 10
"""
import argparse, json, os, sys, time
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
ap.add_argument("-k", type=int, default=15)
ap.add_argument("-w", type=int, default=10)
ap.add_argument("--max-occ", type=int, default=8)
ap.add_argument("--max-occ-ref", type=int, default=64)
ap.add_argument("--no-merge", action="store_true")
ap.add_argument("--max-cand", type=int, default=2048, help="the bound on a row's raw hits")
ap.add_argument("--slack", type=int, default=200)
ap.add_argument("--max-pred", type=int, default=64)
ap.add_argument("--max-dist", type=int, default=1000, help="also the chain entry's gap bounds, which size its rows: 8 max_dist bytes per candidate")
ap.add_argument("--bw", type=int, default=500)
ap.add_argument("--pen-gap", type=int, default=38)
ap.add_argument("--pen-skip", type=int, default=0)
args = ap.parse_args()
n = args.reads

import torch
from mgl_amd import synth
from mgl_amd.smithwaterman import MicrosoftSmithWaterman, GATK_PARAMETERS, concat

ref, base_reads, base_truth = synth.mapping_set(43, min(n, args.distinct), args.length, args.spacer)
reads = [base_reads[i % len(base_reads)] for i in range(n)]
truth = [base_truth[i % len(base_truth)] for i in range(n)]
windows = [ref[pos:pos + m] for pos, m, _ in truth]
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


(T, max_tl), (Q, max_ql) = device(windows), device(reads)
ref_dev = g(np.concatenate([np.frombuffer(ref, np.uint8), np.zeros(8, np.uint8)]), np.uint8)[:len(ref)]
torch.cuda.synchronize()
t0 = time.perf_counter()
index = a.build_index(ref_dev, args.k, args.w)
torch.cuda.synchronize()
build_ms = (time.perf_counter() - t0) * 1e3
t0 = time.perf_counter()
a.build_index(ref_dev, args.k, args.w).close()  # (the first build also loads the code objects)
torch.cuda.synchronize()
build_again_ms = (time.perf_counter() - t0) * 1e3
info = index.info
map_tl = max_tl + 2 * args.slack + 500
stride = 2 * (args.length + 2000)
seed_par = (args.k, args.w, args.max_occ, not args.no_merge, args.max_cand)
index_par = (2, args.max_occ, args.max_occ_ref, not args.no_merge, args.max_cand)
chain_par = dict(max_pred=args.max_pred, max_dist=args.max_dist, bw=args.bw, pen_gap=args.pen_gap, pen_skip=args.pen_skip)
i32 = lambda m: torch.zeros(m, dtype=torch.int32, device=dev)  # noqa: E731
i64 = lambda m: torch.zeros(m, dtype=torch.int64, device=dev)  # noqa: E731
aligned = lambda: (torch.zeros((n, 8), dtype=torch.int32, device=dev), None, None, None, torch.zeros(n * stride, dtype=torch.uint8, device=dev), i32(n), i32(n))  # noqa: E731

# each seed stage once at a capacity that surely holds the batch, to size the arrays of the timed calls by what it found
first = a.seed_strands_device(*T, *Q, *seed_par)
mapped = a.seed_index_device(index, *Q, *index_par)
torch.cuda.synchronize()
assert int((first[6] != 0).sum()) == int((mapped[6] != 0).sum()) == 0, "a row was refused: raise --max-cand"
total_a, total_b = int(first[0][2 * n].item()), int(mapped[0][2 * n].item())
del first, mapped
rows = lambda total: (i64(2 * n + 1), i32(total), i32(total), i32(total), i32(2 * n), i32(2 * n), i32(2 * n))  # noqa: E731
chains = lambda total: (i64(2 * n + 1), i32(total), i32(total), i32(total), i32(2 * n), None, None, i32(2 * n))  # noqa: E731
chosen = lambda total: (i32(n), torch.zeros_like(Q[0]), i64(n + 1), i32(total), i32(total), i32(total), i32(n), i32(n))  # noqa: E731
located = lambda total: (i64(n), i32(n), i32(total), i32(n))  # noqa: E731
seed_a, seed_b, seed_c, seed_d = rows(total_a), rows(total_b), rows(total_b), rows(total_a)
chain_a, chain_b = chains(total_a), chains(total_b)
pick_a, pick_b, pick_e = chosen(total_a), chosen(total_b), chosen(total_b)
where_b, where_e = located(total_b), located(total_b)
out_a, out_b = aligned(), aligned()
align = dict(to_query_end=True, cigar_stride=stride)


def call_a():
    a.align_reads_strands_device(*T, *Q, max_tl, max_ql, args.band, -1, GATK_PARAMETERS, *seed_par, total_a, seed_out=seed_a, chain_out=chain_a,
                                 select_out=pick_a, out=out_a, **chain_par, **align)


def call_b():
    a.map_reads_device(index, *Q, map_tl, max_ql, args.band, -1, GATK_PARAMETERS, args.slack, *index_par, total_b, seed_out=seed_b, chain_out=chain_b,
                       select_out=pick_b, locate_out=where_b, out=out_b, **chain_par, **align)


def call_c():
    a.seed_index_device(index, *Q, *index_par, total_b, out=seed_c)


def call_d():
    a.seed_strands_device(*T, *Q, *seed_par, total_a, out=seed_d)


def call_e():
    a.select_strand_device(*Q, *chain_b[:5], out=pick_e)
    a.locate_window_device(index, Q[2], *pick_e[2:6], args.slack, map_tl, out=where_e)


call_a(); call_b(); torch.cuda.synchronize()
assert int((out_a[6] != 0).sum()) == 0 and int((seed_b[6] != 0).sum()) == int((pick_b[7] != 0).sum()) == 0
pos, span, strand = (np.array([t[c] for t in truth]) for c in range(3))
t_start, t_len = where_b[0].cpu().numpy(), where_b[1].cpu().numpy()
placed = (pick_b[0].cpu().numpy() == strand) & (t_start <= pos) & (pos + span <= t_start + t_len) & (where_b[3].cpu().numpy() == 0)
score_ok = ((out_a[0][:, 0] == out_b[0][:, 0]) & (out_b[6] == 0)).cpu().numpy()
score_ge = ((out_b[0][:, 0] >= out_a[0][:, 0]) & (out_b[6] == 0)).cpu().numpy()  # (a window with slack gives the end extensions room the true window cuts off)
names = ("(a) align_reads_strands on the true windows", "(b) map_reads against the index", "(c) seed_index alone", "(d) seed_strands alone on the true windows",
         "(e) select_strand + locate_window alone")
out = []
for name, secs in zip(names, timed((call_a, call_b, call_c, call_d, call_e))):
    s = np.sort(np.array(secs))
    med = float(np.median(s))
    out.append({"line": name, "reads": n, "reads_per_s": round(n * len(s) / float(s.sum()), 1), "us_per_read": round(float(s.sum()) / len(s) / n * 1e6, 2),
                "ms_per_pass_median": round(med * 1e3, 3), "passes": len(s), "spread_pct": [round((s[0] / med - 1) * 100, 2), round((s[-1] / med - 1) * 100, 2)]})
out[0].update({"band": args.band, "k": args.k, "w": args.w, "max_occ": args.max_occ, "merge": not args.no_merge, "max_cand": args.max_cand,
               "candidates_per_read_both_rows": round(total_a / n, 1)})
out[1].update({"ms_median_vs_a": round(out[1]["ms_per_pass_median"] / out[0]["ms_per_pass_median"], 4), "max_occ_ref": args.max_occ_ref, "slack": args.slack,
               "candidates_per_read_both_rows": round(total_b / n, 1), "true_strand_and_window_holds_true_span": round(float(placed.mean()), 4),
               "and_score_equals_a": round(float((placed & score_ok).mean()), 4), "and_score_at_least_a": round(float((placed & score_ge).mean()), 4)})
out[2].update({"ms_median_vs_d": round(out[2]["ms_per_pass_median"] / out[3]["ms_per_pass_median"], 4)})
out.append({"line": "the index", "ref_len": info.ref_len, "distinct_places": len(base_reads), "entries": info.entries, "bytes": info.bytes,
            "build_ms_first": round(build_ms, 2), "build_ms_again": round(build_again_ms, 2)})
for row in out:
    print(json.dumps(row), flush=True)
index.close()
