"""What aligning EVERY ranked chain costs the read mapper, on section 9k's two workloads: --reads reads of
mgl_amd.synth.repeat_mapping_set (about 10 kb, each from a place of its own in one reference, every odd read reverse-complemented),
without copies (one chain a read) and with --copies of the windows standing twice in the reference (1.5 chains a read at 1 024 of
2 048); (k, w) = (15, 10), max_occ 8, max_occ_ref 64, merged; GATK parameters, band 64, Z-drop off, to the query's end; section 9i's
chaining parameters; max_chains 4, min_score 40, min_cnt 3, mask_level 128.  Lines in ONE run per workload, passes taken in turn after
a warm-up each, every call allocating its own outputs (the caching allocator's) as the yardstick does:

  (a)  map_reads_described_device -- one chain a read aligned: the yardstick
  (b)  map_reads_all_device, keep_secondary = 0
  (c)  map_reads_all_device, keep_secondary = 1
  (d)  expand_chains_device alone on (c)'s rank output; (d') classify_alignments_device alone on (c)'s alignments

The stages behind the expansion run over job_capacity = --capacity-factor * reads pairs, the empty ones refused.  Printed per line:
reads/s over all passes, the median pass and the spread -- the fastest and the slowest pass against the median pass; for (b), (c)
the median against (a)'s, and the jobs a read.  On the workload without copies it asserts that every read's primary line in (b) is
(a)'s alignment: record, CIGAR, describe record.

  python scripts/all_chains_bench.py --reads 2048 --copies 1024 --seconds 3
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
ap.add_argument("--seconds", type=float, default=3)
ap.add_argument("--copies", type=int, default=1024)
ap.add_argument("--divergence", type=float, default=0.01)
ap.add_argument("--max-cand", type=int, default=2048)
ap.add_argument("--slack", type=int, default=200)
ap.add_argument("--max-dist", type=int, default=1000)
ap.add_argument("--capacity-factor", type=int, default=4, help="job_capacity = this many jobs a read (max_chains: every read fits)")
args = ap.parse_args()
n = args.reads

import torch
from mgl_amd import synth
from mgl_amd.smithwaterman import MicrosoftSmithWaterman, GATK_PARAMETERS, concat

dev = torch.device("cuda", 0)
a = MicrosoftSmithWaterman(0)
g = lambda x, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(x).astype(dt))).to(dev)  # noqa: E731
K, W = 15, 10
stride = 2 * (args.length + 2000)
stages = dict(max_occ=8, max_occ_ref=64, merge=True, max_cand=args.max_cand, max_pred=64, max_dist=args.max_dist, bw=500, pen_gap=38, pen_skip=0, max_chains=4,
              min_score=40, min_cnt=3, mask_level=128, slack=args.slack, strands=2, to_query_end=True, cigar_stride=stride)


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


def rows(names, secs, first=None):
    out = []
    for name, s in zip(names, secs):
        s = np.sort(np.array(s))
        med = float(np.median(s))
        out.append({"line": name, "reads": n, "reads_per_s": round(n * len(s) / float(s.sum()), 1), "ms_per_pass_median": round(med * 1e3, 4), "passes": len(s),
                    "spread_pct": [round((s[0] / med - 1) * 100, 2), round((s[-1] / med - 1) * 100, 2)]})
    for row in out[(1 if first is None else 0):]:
        row["ms_median_vs_(a)"] = round(row["ms_per_pass_median"] / (out[0]["ms_per_pass_median"] if first is None else first), 4)
    return out


def workload(copies):
    ref, reads, truth, _ = synth.repeat_mapping_set(43, n, args.length, args.spacer, copies, args.divergence)
    d, off = concat(reads)
    ln = np.diff(off)
    Q, max_ql = (g(np.concatenate([d, np.zeros(8, np.uint8)]), np.uint8), g(off[:-1], np.int64), g(ln, np.int32)), int(ln.max())
    index = a.build_index(g(np.frombuffer(ref, np.uint8), np.uint8), K, W)
    map_tl = max(m for _, m, _ in truth) + 2 * args.slack + 500
    cap = args.capacity_factor * n
    head = (index, *Q, map_tl, max_ql, args.band, -1, GATK_PARAMETERS)
    call_a = lambda: a.map_reads_described_device(*head, **stages)  # noqa: E731
    call_b = lambda: a.map_reads_all_device(*head, keep_secondary=False, job_capacity=cap, **stages)  # noqa: E731
    call_c = lambda: a.map_reads_all_device(*head, keep_secondary=True, job_capacity=cap, **stages)  # noqa: E731
    base, own, full = call_a(), call_b(), call_c()
    torch.cuda.synchronize()
    info = {"copies": copies, "divergence": args.divergence, "ref_len": len(ref), "job_capacity": cap}
    for name, t in (("(b)", own), ("(c)", full)):
        assert int((t[3][10] != 0).sum()) == 0, "a read was refused by the expansion: raise --capacity-factor"
        info["jobs_per_read " + name] = round(int(t[3][0].item()) / n, 4)
        info["lines_per_read " + name] = round(float(t[7][1].sum().item()) / n, 4)
    if copies == 0:  # every read's primary line in (b) is (a)'s alignment
        prim = own[7][2].long()
        ok = (base[4][6] == 0)
        assert bool(((prim >= 0) == ok).all()), "the mapped reads differ"
        j = prim[ok]
        assert bool((own[5][0][j] == base[4][0][ok]).all()) and bool((own[5][5][j] == base[4][5][ok]).all()), "a primary line's record differs from (a)'s"
        assert bool((own[6][0][j] == base[6][0][ok]).all()), "a primary line's describe record differs from (a)'s"
        cg_b, cg_a = own[5][4].view(cap, stride)[j], base[4][4].view(n, stride)[ok]
        keep = torch.arange(stride, device=dev)[None, :] < base[4][5][ok][:, None]
        assert bool(((cg_b == cg_a) | ~keep).all()), "a primary line's CIGAR differs from (a)'s"
        info["primary_lines_equal_(a)"] = int(ok.sum())
    out = rows(["(a) map_reads_described_device", "(b) map_reads_all_device, keep_secondary = 0", "(c) map_reads_all_device, keep_secondary = 1"],
               timed([call_a, call_b, call_c]))
    out[0].update(info)
    ranked, jobs, aln = full[2], full[3], full[5]
    alone = [lambda: a.expand_chains_device(*Q, ranked[6], ranked[0], ranked[1], *ranked[2:6], 4, True, cap),
             lambda: a.classify_alignments_device(jobs[1], jobs[2], aln[0], aln[6], GATK_PARAMETERS[0], 40, 128)]
    out += rows(["(d) expand_chains_device alone", "(d') classify_alignments_device alone"], timed(alone), first=out[0]["ms_per_pass_median"])
    for row in out:
        print(json.dumps(row), flush=True)
    index.close()


workload(0)
workload(args.copies)
