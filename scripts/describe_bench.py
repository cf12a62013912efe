"""What describing the alignments costs the read mapper: section 9j's workload -- --reads reads of
mgl_amd.synth.mapping_set (about 10 kb; --distinct of them laid into one reference, the batch cycles through them), every odd read
reverse-complemented -- with section 9k's parameters.  Lines in ONE run, in turn after a warm-up each:

  (a)  map_reads_ranked_device -- the parent's path and the yardstick
  (b)  map_reads_described_device
  (c)  describe_device alone on (a)'s alignments, and (c') the same without the extended CIGAR
  (d)  the host alternative: the records, the windows' starts, the oriented reads and the CIGARs copied back and walked with numpy and
       Python against the reference the caller holds (NM, MD, matches and block length; no extended CIGAR), the copies inside its time.
       Wall-clock, --host-passes passes after the device lines.

Printed per line: reads/s over all passes, the median pass and the spread -- the fastest and the slowest pass against the median pass; for
(b) its time against (a)'s, for (d) its time against (c)'s.  (d)'s NM and MD are compared with the device's on every read.

  python scripts/describe_bench.py --reads 2048 --distinct 2048 --seconds 10
"""
import argparse, json, os, re, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=2048)
ap.add_argument("--length", type=int, default=10000)
ap.add_argument("--spacer", type=int, default=3000)
ap.add_argument("--band", type=int, default=64)
ap.add_argument("--seconds", type=float, default=10)
ap.add_argument("--host-passes", type=int, default=3)
ap.add_argument("--distinct", type=int, default=128, help="distinct reads and places in the reference (the batch cycles through them)")
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
ref, base_reads, base_truth, _ = synth.repeat_mapping_set(43, distinct, args.length, args.spacer, 0, 0.0)
reads = [base_reads[i % distinct] for i in range(n)]
dev = torch.device("cuda", 0)
a = MicrosoftSmithWaterman(0)
g = lambda x, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(x).astype(dt))).to(dev)  # noqa: E731
d, off = concat(reads)
ln = np.diff(off)
Q, max_ql = (g(np.concatenate([d, np.zeros(8, np.uint8)]), np.uint8), g(off[:-1], np.int64), g(ln, np.int32)), int(ln.max())
ref_host = np.frombuffer(ref, np.uint8)
ref_dev = g(np.concatenate([ref_host, np.zeros(8, np.uint8)]), np.uint8)[:len(ref)]
index = a.build_index(ref_dev, args.k, args.w)
map_tl = max(len(ref[p:p + m]) for p, m, _ in base_truth) + 2 * args.slack + 500
stride = 2 * (args.length + 2000)
index_par = (2, args.max_occ, args.max_occ_ref, True, args.max_cand)
chain_par = dict(max_pred=64, max_dist=args.max_dist, bw=500, pen_gap=38, pen_skip=0)
rank_par = (args.max_chains, args.min_score, args.min_cnt, args.mask_level)
i32 = lambda m: torch.zeros(m, dtype=torch.int32, device=dev)  # noqa: E731
i64 = lambda m: torch.zeros(m, dtype=torch.int64, device=dev)  # noqa: E731
u8 = lambda m: torch.zeros(m, dtype=torch.uint8, device=dev)  # noqa: E731
aligned = lambda: (torch.zeros((n, 8), dtype=torch.int32, device=dev), None, None, None, u8(n * stride), i32(n), i32(n))  # noqa: E731

first = a.seed_index_device(index, *Q, *index_par)
torch.cuda.synchronize()
assert int((first[6] != 0).sum()) == 0, "a row was refused: raise --max-cand"
total = int(first[0][2 * n].item())
del first
rows = lambda: (i64(2 * n + 1), i32(total), i32(total), i32(total), i32(2 * n), i32(2 * n), i32(2 * n))  # noqa: E731
chains = lambda: (i64(2 * n + 1), i32(total), i32(total), i32(total), i32(2 * n), i32(total), i32(total), i32(2 * n))  # noqa: E731
chosen = lambda: (i32(n), torch.zeros_like(Q[0]), i64(n + 1), i32(total), i32(total), i32(total), i32(n), i32(n))  # noqa: E731
located = lambda: (i64(n), i32(n), i32(total), i32(n))  # noqa: E731
ranked = lambda: (i32(n), torch.zeros((n, args.max_chains, 12), dtype=torch.int32, device=dev), None, None, None, None, i32(n))  # noqa: E731
described = lambda xc: (torch.zeros((n, 8), dtype=torch.int32, device=dev), u8(n * stride), u8(n * stride) if xc else None, i32(n))  # noqa: E731
seed_a, seed_b, chain_a, chain_b = rows(), rows(), chains(), chains()
pick_a, pick_b, where_a, where_b, out_a, out_b, rank_a, rank_b = chosen(), chosen(), located(), located(), aligned(), aligned(), ranked(), ranked()
desc_b, desc_c, desc_c2 = described(True), described(True), described(False)
align = dict(to_query_end=True, cigar_stride=stride)


def call_a():
    a.map_reads_ranked_device(index, *Q, map_tl, max_ql, args.band, -1, GATK_PARAMETERS, 2, args.max_cand, total, seed_a, chain_a, *rank_par, rank_out=rank_a,
                              slack=args.slack, max_occ=args.max_occ, max_occ_ref=args.max_occ_ref, merge=True, select_out=pick_a, locate_out=where_a, out=out_a,
                              **chain_par, **align)


def call_b():
    a.map_reads_described_device(index, *Q, map_tl, max_ql, args.band, -1, GATK_PARAMETERS, md_stride=stride, xcigar_stride=stride, describe_out=desc_b, strands=2,
                                 max_cand=args.max_cand, cand_capacity=total, seed_out=seed_b, chain_out=chain_b, max_chains=rank_par[0], min_score=rank_par[1],
                                 min_cnt=rank_par[2], mask_level=rank_par[3], rank_out=rank_b, slack=args.slack, max_occ=args.max_occ, max_occ_ref=args.max_occ_ref,
                                 merge=True, select_out=pick_b, locate_out=where_b, out=out_b, **chain_par, **align)


def call_c():
    a.describe_device(ref_dev, where_a[0], where_a[1], pick_a[1], Q[1], Q[2], out_a[0], out_a[4], stride, out_a[5], out_a[6], stride, stride, out=desc_c)


def call_c2():
    a.describe_device(ref_dev, where_a[0], where_a[1], pick_a[1], Q[1], Q[2], out_a[0], out_a[4], stride, out_a[5], out_a[6], stride, stride, out=desc_c2)


ELEMENT = re.compile(rb"(\d+)([MID])")


def host_describe():
    """-> (nm [n], n_match [n], [md bytes]) from what the device holds, copied back here"""
    rec, t_start, st = out_a[0].cpu().numpy(), where_a[0].cpu().numpy(), out_a[6].cpu().numpy()
    cg, cl = out_a[4].cpu().numpy().reshape(n, stride), out_a[5].cpu().numpy()
    oriented, q_start = pick_a[1].cpu().numpy(), off
    nm, match, mds = np.zeros(n, np.int64), np.zeros(n, np.int64), []
    for p in range(n):
        if st[p]:
            mds.append(b"")
            continue
        i, j = int(t_start[p]) + int(rec[p, 1]), int(q_start[p]) + int(rec[p, 3])
        md, run, edits, same = [], 0, 0, 0
        for num, op in ELEMENT.findall(cg[p, :cl[p]].tobytes()):
            k = int(num)
            if op == b"M":
                t = ref_host[i:i + k]
                miss = np.flatnonzero(t != oriented[j:j + k])
                last = -1
                for c in miss.tolist():
                    md.append(b"%d%c" % (run + c - last - 1, int(t[c])))
                    run, last = 0, c
                run += k - 1 - last
                edits += len(miss)
                same += k - len(miss)
                i, j = i + k, j + k
            elif op == b"I":
                edits, j = edits + k, j + k
            else:
                md.append(b"%d^" % run + ref_host[i:i + k].tobytes())
                run, edits, i = 0, edits + k, i + k
        md.append(b"%d" % run)
        nm[p], match[p] = edits, same
        mds.append(b"".join(md))
    return nm, match, mds


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


call_a(); call_b(); call_c(); torch.cuda.synchronize()
assert int((seed_b[6] != 0).sum()) == int((pick_b[7] != 0).sum()) == int((rank_b[6] != 0).sum()) == 0
assert all(bool((x == y).all()) for x, y in zip((out_a[0], out_a[5], out_a[6], pick_a[0]), (out_b[0], out_b[5], out_b[6], pick_b[0]))), "the alignment changed"
assert bool((desc_b[0] == desc_c[0]).all()) and bool((desc_b[3] == desc_c[3]).all()) and bool((desc_b[3] == out_a[6]).all()), "a text beyond its stride"
names = ["(a) map_reads_ranked_device", "(b) map_reads_described_device", "(c) describe_device alone", "(c') describe_device alone, no extended CIGAR"]
all_secs = timed((call_a, call_b, call_c, call_c2))
host = []
for _ in range(args.host_passes):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    nm, match, mds = host_describe()
    host.append(time.perf_counter() - t0)
stats, md_dev = desc_c[0].cpu().numpy(), desc_c[1].cpu().numpy().reshape(n, stride)
agree = bool((stats[:, 1] + stats[:, 2] + stats[:, 3] == nm).all() and (stats[:, 0] == match).all() and all(md_dev[p, :stats[p, 6]].tobytes() == mds[p] for p in range(n)))
if args.host_passes:
    names.append("(d) the host alternative")
    all_secs.append(host)
out = []
for name, secs in zip(names, all_secs):
    s = np.sort(np.array(secs))
    med = float(np.median(s))
    out.append({"line": name, "reads": n, "reads_per_s": round(n * len(s) / float(s.sum()), 1), "us_per_read": round(float(s.sum()) / len(s) / n * 1e6, 3),
                "ms_per_pass_median": round(med * 1e3, 4), "passes": len(s), "spread_pct": [round((s[0] / med - 1) * 100, 2), round((s[-1] / med - 1) * 100, 2)]})
ok = stats[desc_c[3].cpu().numpy() == 0]
out[0].update({"distinct": distinct, "ref_len": len(ref), "mapped": int(len(ok))})
out[1].update({"ms_median_vs_a": round(out[1]["ms_per_pass_median"] / out[0]["ms_per_pass_median"], 4)})
out[2].update({"columns_per_read": round(float(ok[:, :4].sum(axis=1).mean()), 1), "nm_per_read": round(float(ok[:, 1:4].sum(axis=1).mean()), 1),
               "md_bytes_per_read": round(float(ok[:, 6].mean()), 1), "xcigar_bytes_per_read": round(float(ok[:, 7].mean()), 1),
               "cigar_bytes_per_read": round(float(out_a[5].float().mean().item()), 1)})
if args.host_passes:
    out[4].update({"ms_median_vs_c": round(out[4]["ms_per_pass_median"] / out[2]["ms_per_pass_median"], 1), "agrees_with_the_device": agree})
for row in out:
    print(json.dumps(row), flush=True)
index.close()
sys.exit(0 if agree or not args.host_passes else 1)
