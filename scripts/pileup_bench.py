"""What the pileup costs behind the read mapper, on section 9n's workload: --reads reads of
mgl_amd.synth.repeat_mapping_set (about 10 kb, each from a place of its own in one reference of 26.6 Mb at 2 048 reads, every odd read
reverse-complemented), no copies; (k, w) = (15, 10), max_occ 8, max_occ_ref 64, merged; GATK parameters, band 64, Z-drop off, to the
query's end; section 9i's chaining parameters; max_chains 4, min_score 40, min_cnt 3, mask_level 128.  Every comparison is ONE run
with both sides in it, passes taken in turn after a warm-up each:

  (a)  map_reads_all_device against map_reads_pileup_device adding into one table
  (b)  pileup_device alone on (a)'s tensors, as adds per second and as added bytes per second (docs/history.md has the M step's other
       form, measured by this script's lines on a build that kept both)
  (c)  the same alignments all laid on one window of the reference: the high-coverage, contended case
  (d)  pileup_sites_device over the whole table against a device copy of the same table
  (e)  the same counts with numpy on the host, one pass, and the two tables compared

Printed per line: the median pass and the spread -- the fastest and the slowest pass against the median pass.

  python scripts/pileup_bench.py --reads 2048 --seconds 2
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
ap.add_argument("--seconds", type=float, default=2)
ap.add_argument("--max-cand", type=int, default=2048)
ap.add_argument("--slack", type=int, default=200)
ap.add_argument("--max-dist", type=int, default=1000)
ap.add_argument("--no-host", action="store_true", help="skip (e)")
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
              min_score=40, min_cnt=3, mask_level=128, slack=args.slack, strands=2, to_query_end=True, cigar_stride=stride, job_capacity=4 * n)


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


def rows(names, secs, **more):
    out = []
    for name, s in zip(names, secs):
        s = np.sort(np.array(s))
        med = float(np.median(s))
        out.append(dict({"line": name, "ms_per_pass_median": round(med * 1e3, 4), "passes": len(s),
                         "spread_pct": [round((s[0] / med - 1) * 100, 2), round((s[-1] / med - 1) * 100, 2)]}, **more))
    for row in out[1:]:
        row["ms_median_vs_first"] = round(row["ms_per_pass_median"] / out[0]["ms_per_pass_median"], 4)
    for row in out:
        print(json.dumps(row), flush=True)
    return out


ref, reads, truth, _ = synth.repeat_mapping_set(43, n, args.length, args.spacer, 0, 0.0)
d, off = concat(reads)
ln = np.diff(off)
Q, max_ql = (g(np.concatenate([d, np.zeros(8, np.uint8)]), np.uint8), g(off[:-1], np.int64), g(ln, np.int32)), int(ln.max())
index = a.build_index(g(np.frombuffer(ref, np.uint8), np.uint8), K, W)
ref_len = len(ref)
map_tl = max(m for _, m, _ in truth) + 2 * args.slack + 500
head = (index, *Q, map_tl, max_ql, args.band, -1, GATK_PARAMETERS)
table = torch.zeros((8, ref_len), dtype=torch.int32, device=dev)

# ---- (a) the pipeline with and without the pileup
res = a.map_reads_pileup_device(*head, counts=table, **stages)
torch.cuda.synchronize()
jobs, window, aln, lines = res[3], res[4], res[5], res[7][0]
counted = int((res[8][1] == 0).sum().item())
one = table.clone()
adds = int(one[:6].sum(dtype=torch.int64).item() + 2 * one[6].sum(dtype=torch.int64).item())
info = {"reads": n, "ref_len": ref_len, "table_bytes": 32 * ref_len, "alignments_counted": counted, "adds_per_pass": adds}
rows(["(a) map_reads_all_device", "(a) map_reads_pileup_device, adding into one table"],
     timed([lambda: a.map_reads_all_device(*head, **stages), lambda: a.map_reads_pileup_device(*head, counts=table, **stages)]), **info)

# ---- (b), (c) the pileup alone: spread over the reference, and laid on one window
select = ((lines[:, 0] >= 0) & ((lines[:, 1] & 0x100) == 0)).to(torch.int32)
for name, t_start in (("(b) pileup_device alone", window[0]), ("(c) pileup_device, every alignment on one window", torch.full_like(window[0], int(window[0][0].item())))):
    call = lambda t_start=t_start: a.pileup_device(index.ref, t_start, window[1], jobs[9], jobs[3], jobs[4], aln[0], aln[4], stride, aln[5], aln[6], select,  # noqa: E731
                                                   (0, ref_len), table)
    s = timed([call])[0]
    med = float(np.median(s))
    rows([name], [s], adds_per_s=round(adds / med, 1), added_bytes_per_s=round(4 * adds / med, 1))

# ---- (d) the sites over the whole table against a device copy of it
table.copy_(one)
spare = torch.empty_like(table)
out = a.pileup_sites_device(table, index.ref, site_capacity=1 << 20)
torch.cuda.synchronize()
rows(["(d) a device copy of the table", "(d) pileup_sites_device over the whole reference"],
     timed([lambda: spare.copy_(table), lambda: a.pileup_sites_device(table, index.ref, site_capacity=1 << 20, out=out)]), n_sites=int(out[3][0].item()))

# ---- (e) the same counts with numpy on the host, from the device's own alignments read back
if not args.no_host:
    cap = 4 * n
    keep = np.flatnonzero((res[8][1].cpu().numpy() == 0) & (select.cpu().numpy() != 0))
    rec, cg, cl = aln[0].cpu().numpy(), aln[4].cpu().numpy().reshape(cap, stride), aln[5].cpu().numpy()
    ts, qs, ori = window[0].cpu().numpy(), jobs[3].cpu().numpy(), jobs[9].cpu().numpy()
    lut = np.full(256, 4, np.int64)
    for k, pair in enumerate((b"Aa", b"Cc", b"Gg", b"Tt")):
        lut[list(pair)] = k
    import re
    t0 = time.perf_counter()
    host = np.zeros((8, ref_len), np.uint32)
    for j in keep:
        pos, qat = int(ts[j]) + int(rec[j, 1]), int(qs[j]) + int(rec[j, 3])
        for num, op in re.findall(r"(\d+)([MID])", cg[j, :cl[j]].tobytes().decode()):
            m = int(num)
            if op == "M":
                np.add.at(host, (lut[ori[qat:qat + m]], np.arange(pos, pos + m)), 1)
                pos, qat = pos + m, qat + m
            elif op == "D":
                host[5, pos:pos + m] += 1
                pos += m
            else:
                if pos > 0:
                    host[6, pos - 1] += 1
                    host[7, pos - 1] += m
                qat += m
    sec = time.perf_counter() - t0
    same = bool((host.view(np.int32) == one.cpu().numpy()).all())
    print(json.dumps({"line": "(e) the same counts with numpy on the host, one pass", "ms": round(sec * 1e3, 1), "equal_to_the_device_table": same}), flush=True)
    assert same
index.close()
