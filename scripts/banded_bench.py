"""The banded entry against the full-matrix path on the long-read workload of scripts/long_read_bench.py (ONT-style
~10 kb x ~10 kb pairs, 5 % substitutions / insertions / deletions, GATK parameters, SOFTCLIP, seeded), in ONE run:

  line 1   the full-matrix path (DeviceBatch.run on the pairs): pairs/s, GCUPS
  line 2+  mgl_sw_align_batch_device_banded at band = 128, 256, 512, 1024, 2048: pairs/s, GCUPS over the cells in the band, and the
           share of pairs whose offset and CIGAR equal line 1's (1.0 once the band holds the paths: relation R2)

Every line: a warm-up pass, then passes until --seconds of GPU time (events around the calls) have gone by.

  python scripts/banded_bench.py --pairs 2048 --seconds 30
"""
import argparse, json, os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np
import torch
from mgl_amd import device_batch, synth
from mgl_amd.smithwaterman import MicrosoftSmithWaterman, GATK_PARAMETERS, SWOverhangStrategy, concat

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=2048)
ap.add_argument("--length", type=int, default=10000)
ap.add_argument("--seconds", type=float, default=30)
ap.add_argument("--distinct", type=int, default=32, help="distinct synthetic pairs (the batch cycles through them)")
ap.add_argument("--workspace-gib", type=float, default=0, help="0: the context's default")
ap.add_argument("--bands", default="128,256,512,1024,2048")
ap.add_argument("--skip-full", action="store_true")
args = ap.parse_args()
n = args.pairs

rng = synth.rng_for(11)
base = [synth.ont_pair(rng, args.length) for _ in range(min(n, args.distinct))]
ts = [base[k % len(base)][0].tobytes() for k in range(n)]
qs = [base[k % len(base)][1].tobytes() for k in range(n)]
td, toff = concat(ts); qd, qoff = concat(qs)
stride = 2 * (args.length + 2000)
b = device_batch.from_host(td, toff, qd, qoff, "cuda:0", cigar_stride=stride)
dev = b.targets.device
a = MicrosoftSmithWaterman(0)
if args.workspace_gib > 0:
    a.set_workspace(int(args.workspace_gib * (1 << 30)))
tl = np.diff(toff).astype(np.int64); ql = np.diff(qoff).astype(np.int64)


def timed(call):
    """a warm-up pass, then passes until args.seconds of GPU time: seconds per pass"""
    call(); torch.cuda.synchronize()
    total, reps = 0.0, 0
    while total < args.seconds:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record(); torch.cuda.synchronize()
        total += e0.elapsed_time(e1) * 1e-3
        reps += 1
    return total / reps, reps


def band_cells(band):
    out = 0
    for k in range(min(n, len(base))):
        t_, q_ = int(tl[k]), int(ql[k])
        lo, hi = min(0, q_ - t_) - band, max(0, q_ - t_) + band
        i = np.arange(1, t_ + 1)
        cells = int((np.minimum(q_, i + hi) - np.maximum(1, i + lo) + 1).sum())
        out += cells * len(range(k, n, len(base)))
    return out


rows = []
full_cells = int((tl * ql).sum())
if not args.skip_full:
    sec, reps = timed(lambda: b.run(a))
    assert int((b.status != 0).sum()) == 0
    rows.append({"line": "full matrix", "kernel": a.fill_kernel_name(a.timing()), "pairs_per_s": round(n / sec, 1), "gcups": round(full_cells / sec / 1e9, 1),
                 "ms_per_pass": round(sec * 1e3, 2), "passes": reps})
    print(json.dumps(rows[-1]), flush=True)
g = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x.astype(dt))).to(dev)  # noqa: E731
tdev = g(np.concatenate([td, np.zeros(8, np.uint8)]), np.uint8); qdev = g(np.concatenate([qd, np.zeros(8, np.uint8)]), np.uint8)
tst, qst, tln, qln = g(toff[:-1], np.int64), g(qoff[:-1], np.int64), g(tl, np.int32), g(ql, np.int32)
out = (torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros((n, 6), dtype=torch.int32, device=dev), torch.zeros(n * stride, dtype=torch.uint8, device=dev),
       torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev))
for band in [int(x) for x in args.bands.split(",")]:
    out[2].zero_()
    call = lambda: a.align_banded_device(tdev, tst, tln, qdev, qst, qln, int(tl.max()), int(ql.max()), band, GATK_PARAMETERS, SWOverhangStrategy.SOFTCLIP,  # noqa: E731
                                         stride, False, False, out=out)
    sec, reps = timed(call)
    assert int((out[4] != 0).sum()) == 0, "a pair with a status"
    cells = band_cells(band)
    row = {"line": f"band {band}", "kernel": a.fill_kernel_name(a.timing()), "pairs_per_s": round(n / sec, 1), "gcups_in_band": round(cells / sec / 1e9, 1),
           "band_share_of_cells": round(cells / full_cells, 4), "ms_per_pass": round(sec * 1e3, 2), "passes": reps}
    if not args.skip_full:
        same = (out[0] == b.offsets) & (out[3] == b.cigar_len) & (out[2].view(n, stride) == b.cigars).all(dim=1)
        row["share_equal_to_full"] = round(float(same.float().mean()), 4)
        row["speedup"] = round(row["pairs_per_s"] / rows[0]["pairs_per_s"], 2)
    rows.append(row)
    print(json.dumps(row), flush=True)
