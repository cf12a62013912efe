"""MGL_SW_FLAG_EXTEND_ADAPTIVE_BAND next to the fixed band of mgl_sw_extend_batch_device on long reads whose path drifts: ~10 kb targets,
queries derived from them with substitutions, short indels either way and --jumps insertions of --jump bases, evenly spaced, so that
the net drift over the pair exceeds 128 diagonals and no indel between two re-centrings does.  (Insertions only: with deletions of 30
bases for every other pair 12 of 16 such pairs lost the path at band 128 -- under the GATK parameters the row maximum behind a long
deletion lies to the RIGHT of the path, see DESIGN.md section 9d -- and the generator was changed, as its check demands.)  GATK parameters, Z-drop off, 32 distinct pairs cycled, in ONE run:

  (a) fixed band 512      (b) adaptive band 512      (c) adaptive band 128      (d) fixed band 128: wrong on these pairs, printed as
                                                                                    the bound on what the narrower band can give

First, on the CPU with the row-wise textbooks, for the distinct pairs: adaptive at 128 and fixed at 512 must both give the score of the
fixed textbook at a band that covers the pair (tl + ql); the count is printed and must be all of them (--verify none skips this, for a
second run of the same seed; --verify only stops behind it and needs no GPU).  Every line: a warm-up pass, then passes until --seconds
of GPU time (events around the calls).

  python scripts/extend_adaptive_bench.py --pairs 2048 --seconds 30
"""
import argparse, json, os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import extend_adaptive_textbook as at
import extend_textbook as et

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=2048)
ap.add_argument("--length", type=int, default=10000)
ap.add_argument("--seconds", type=float, default=30)
ap.add_argument("--distinct", type=int, default=32, help="distinct synthetic pairs (the batch cycles through them)")
ap.add_argument("--jumps", type=int, default=10)
ap.add_argument("--jump", type=int, default=30)
ap.add_argument("--verify", choices=("full", "none", "only"), default="full")
args = ap.parse_args()
n = args.pairs
GATK = (200, -150, 260, 11)
ACGT = np.frombuffer(b"ACGT", np.uint8)


def make_pair(rng, k):
    """5 % substitutions, 1 % + 1 % indels of 1 .. 3 bases, and args.jumps insertions of args.jump bases"""
    t = ACGT[rng.integers(4, size=args.length)]
    jumps = {(args.length // (args.jumps + 1)) * (x + 1) + 11 * x for x in range(args.jumps)}
    q, skip = [], 0
    for pos, ch in enumerate(t):
        if pos in jumps:
            q.extend(ACGT[rng.integers(4, size=args.jump)])
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
    return t.tobytes(), np.array(q, np.uint8).tobytes()


rng = np.random.default_rng(41)
base = [make_pair(rng, k) for k in range(min(n, args.distinct))]
if args.verify != "none":
    good = 0
    for k, (t, q) in enumerate(base):
        full = et.extend_align_np(t, q, *GATK, len(t) + len(q), -1)[0]
        ad = at.extend_adaptive_align_np(t, q, *GATK, 128, -1)[0]
        st512 = et.extend_align_np(t, q, *GATK, 512, -1)[0]
        st128 = et.extend_align_np(t, q, *GATK, 128, -1)[0]
        ok = ad.score == full.score == st512.score
        good += ok
        print(json.dumps({"pair": k, "tl": len(t), "ql": len(q), "net_drift": full.q_end - full.t_end, "score_full": full.score, "score_adaptive_128": ad.score,
                          "score_fixed_512": st512.score, "score_fixed_128": st128.score, "ok": bool(ok)}), flush=True)
    print(json.dumps({"verified": good, "of": len(base)}), flush=True)
    if good != len(base):
        sys.exit("the generator must be changed: not every pair has the property")
    if args.verify == "only":
        sys.exit(0)

import torch
from mgl_amd.smithwaterman import MicrosoftSmithWaterman, GATK_PARAMETERS, concat

ts = [base[k % len(base)][0] for k in range(n)]
qs = [base[k % len(base)][1] for k in range(n)]
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


out = (torch.zeros((n, 8), dtype=torch.int32, device=dev), torch.zeros(n * stride, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
       torch.zeros(n, dtype=torch.int32, device=dev))
rows, scores = {}, {}
for name, band, adaptive in (("(a) fixed 512", 512, False), ("(b) adaptive 512", 512, True), ("(c) adaptive 128", 128, True), ("(d) fixed 128 (wrong on these pairs)", 128, False)):
    sec, reps = timed(lambda: a.extend_device(tdev, tst, tln, qdev, qst, qln, max_tl, max_ql, band, -1, GATK_PARAMETERS, False, stride, False, False, out=out,
                                              adaptive_band=adaptive))
    assert int((out[3] != 0).sum()) == 0
    scores[name] = out[0][:, 0].cpu().numpy().astype(np.int64)
    slot = (at.extend_adaptive_slot_bytes if adaptive else et.extend_slot_bytes)(max_tl, max_ql, band)
    rows[name] = {"line": name, "kernel": a.fill_kernel_name(a.timing()), "band": band, "pairs_per_s": round(n / sec, 1), "us_per_pair": round(sec / n * 1e6, 2),
                  "ms_per_pass": round(sec * 1e3, 2), "passes": reps, "slot_bytes": slot, "score_equal_to_a": int((scores[name] == scores["(a) fixed 512"]).sum())}
    if name != "(a) fixed 512":
        rows[name]["pairs_per_s_vs_a"] = round(rows[name]["pairs_per_s"] / rows["(a) fixed 512"]["pairs_per_s"], 4)
    print(json.dumps(rows[name]), flush=True)
assert (scores["(b) adaptive 512"] == scores["(a) fixed 512"]).all() and (scores["(c) adaptive 128"] == scores["(a) fixed 512"]).all()
