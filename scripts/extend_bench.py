"""mgl_sw_extend_batch_device next to the banded entry on the long-read workload of scripts/banded_bench.py (SURVEY.md 8d config 4:
ONT-style ~10 kb x ~10 kb pairs, GATK parameters, seeded), at one band, in ONE run:

  line 1  mgl_sw_align_batch_device_banded (SOFTCLIP)
  line 2  (a) the extension, Z-drop off
  line 3  (b) the extension of the same targets by queries whose second half is unrelated random ACGT, zdrop = --zdrop (default
          400 x gext = 4400): the mean rows_done / tl, and the time per pair against the prediction ceil(rows_done / 64) / ceil(tl / 64)
  line 4  (c) the same with a second half that shares no byte with the targets (lower case): under the GATK parameters random ACGT
          against random ACGT does not lose score (gext = 11 buys a match of 200 cheaply), so (b) never drops; (c) does

Every line: a warm-up pass, then passes until --seconds of GPU time (events around the calls).  Also the workspace per slot of both.

  python scripts/extend_bench.py --pairs 2048 --seconds 30
"""
import argparse, json, os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import torch
import banded_textbook as bt
import extend_textbook as et
from mgl_amd import synth
from mgl_amd.smithwaterman import MicrosoftSmithWaterman, GATK_PARAMETERS, SWOverhangStrategy, concat

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=2048)
ap.add_argument("--length", type=int, default=10000)
ap.add_argument("--seconds", type=float, default=30)
ap.add_argument("--distinct", type=int, default=32, help="distinct synthetic pairs (the batch cycles through them)")
ap.add_argument("--band", type=int, default=512)
ap.add_argument("--zdrop", type=int, default=400 * 11)
args = ap.parse_args()
n, band = args.pairs, args.band

rng = synth.rng_for(11)
base = [synth.ont_pair(rng, args.length) for _ in range(min(n, args.distinct))]
junk = np.random.default_rng(12)
ts = [base[k % len(base)][0].tobytes() for k in range(n)]
qs = [base[k % len(base)][1].tobytes() for k in range(n)]
half = [q[:len(q) // 2] + np.frombuffer(b"ACGT", np.uint8)[junk.integers(4, size=len(q) - len(q) // 2)].tobytes() for q in qs[:len(base)]]
qs_b = [half[k % len(base)] for k in range(n)]
qs_c = [q[:len(q) // 2] + q[len(q) // 2:].lower() for q in qs_b]
dev = torch.device("cuda", 0)
a = MicrosoftSmithWaterman(0)
stride = 2 * (args.length + 2000)
g = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x.astype(dt))).to(dev)  # noqa: E731


def device(seqs):
    d, off = concat(seqs)
    ln = np.diff(off)
    return g(np.concatenate([d, np.zeros(8, np.uint8)]), np.uint8), g(off[:-1], np.int64), g(ln, np.int32), ln


tdev, tst, tln, tl = device(ts)
qdev, qst, qln, ql = device(qs)
max_tl, max_ql = int(tl.max()), int(ql.max())


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


def line(name, sec, reps, **more):
    row = {"line": name, "kernel": a.fill_kernel_name(a.timing()), "band": band, "pairs_per_s": round(n / sec, 1), "us_per_pair": round(sec / n * 1e6, 2),
           "ms_per_pass": round(sec * 1e3, 2), "passes": reps, **more}
    print(json.dumps(row), flush=True)
    return row


out_b = (torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros((n, 6), dtype=torch.int32, device=dev), torch.zeros(n * stride, dtype=torch.uint8, device=dev),
         torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev))
sec, reps = timed(lambda: a.align_banded_device(tdev, tst, tln, qdev, qst, qln, max_tl, max_ql, band, GATK_PARAMETERS, SWOverhangStrategy.SOFTCLIP, stride, False, False,
                                                out=out_b))
assert int((out_b[4] != 0).sum()) == 0
r0 = line("banded", sec, reps, slot_bytes=bt.banded_slot_bound(max_tl, max_ql, band))
out = (torch.zeros((n, 8), dtype=torch.int32, device=dev), out_b[2], out_b[3], out_b[4])
sec, reps = timed(lambda: a.extend_device(tdev, tst, tln, qdev, qst, qln, max_tl, max_ql, band, -1, GATK_PARAMETERS, False, stride, False, False, out=out))
assert int((out[3] != 0).sum()) == 0
ext = out[0].cpu().numpy()
assert (ext[:, 5] == tl).all() and not ext[:, 6].any()
r1 = line("(a) extend, zdrop off", sec, reps, slot_bytes=et.extend_slot_bytes(max_tl, max_ql, band), time_vs_banded=round(sec / (n / r0["pairs_per_s"]), 3))
strips = lambda rows: (rows + 63) // 64  # noqa: E731
for name, seqs in (("(b) extend, second half unrelated ACGT", qs_b), ("(c) extend, second half of another alphabet", qs_c)):
    qdev_x, qst_x, qln_x, ql_x = device(seqs)
    sec, reps = timed(lambda: a.extend_device(tdev, tst, tln, qdev_x, qst_x, qln_x, max_tl, int(ql_x.max()), band, args.zdrop, GATK_PARAMETERS, False, stride, False,
                                              False, out=out))
    assert int((out[3] != 0).sum()) == 0
    ext = out[0].cpu().numpy()
    # the strips a wave sweeps: through the one that holds the first dropping row (rows_done + 1), all of them without a drop
    swept = np.where(ext[:, 6] == 1, strips(ext[:, 5] + 1), strips(tl))
    line(name, sec, reps, zdrop=args.zdrop, dropped_share=round(float(ext[:, 6].mean()), 4), mean_rows_done_over_tl=round(float((ext[:, 5] / tl).mean()), 4),
         predicted_time_vs_a=round(float((strips(ext[:, 5]) / strips(tl)).mean()), 4), strips_swept_vs_a=round(float((swept / strips(tl)).mean()), 4),
         measured_time_vs_a=round(sec / (n / r1["pairs_per_s"]), 4))
