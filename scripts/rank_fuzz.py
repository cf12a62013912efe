"""mgl_sw_rank_chains_batch_device against the textbook (tests/rank_textbook.py) on random batches: 1 .. 40 reads of one or two rows of
0 .. 200 candidates (now and then 300 .. 900, rarely 4 000 .. 8 192) with a made-up forest for f and pred or the chain textbook's own,
random parameters (max_chains 1 .. 16, min_score, min_cnt, mask_level 1 .. 256), max_cand below some rows' counts, and bad reads -- a bad
pred of each kind, a length below 1, a row with a status over poisoned f / pred; now and then without the optional arrays: every output
of every read -- the chain counts, the records, the anchor arrays, the status -- and the canaries behind them.  Not a test: prints the
reads run, their candidates, the refused reads, the kept chains, the calls and the mismatches (expected 0).

  python scripts/rank_fuzz.py --seconds 60 --seed 1
"""
import argparse, os, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import torch
import rank_cases as rc
from mgl_amd.smithwaterman import MicrosoftSmithWaterman

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=60)
ap.add_argument("--seed", type=int, default=1)
args = ap.parse_args()
rng = np.random.default_rng(args.seed)
a = MicrosoftSmithWaterman(0)
dev = torch.device("cuda", 0)
PAD = 16
NAMES = ("n_chains", "records", "ranked_start", "ranked_t", "ranked_q", "ranked_len", "status")


def row():
    r = rng.random()
    n = 0 if r < 0.08 else int(rng.integers(4000, 8193)) if r < 0.085 else int(rng.integers(300, 901)) if r < 0.13 else int(rng.integers(1, 201))
    ql, cands, f, pred, st = rc.forest_row(rng, n, roots=float(rng.choice((0.02, 0.1, 0.5)))) if rng.random() < 0.7 or n > 900 else rc.dp_row(rng, n)
    if n and rng.random() < 0.05:  # a bad pred of one kind, a length below 1, or a status over poison
        kind, k = int(rng.integers(6)), int(rng.integers(n))
        if kind < 4:
            pred = list(pred)
            pred[k] = [k, k + 1 + int(rng.integers(3)), -2 - int(rng.integers(3)), k - 65][kind]
        elif kind == 4:
            ql = -int(rng.integers(2))
        else:
            f, pred, st = [rc.POISON] * n, [rc.POISON] * n, int(rng.choice((1, 5)))
    return (ql, cands, f, pred, st)


reads = cands = refused = kept = calls = bad = 0
t0 = time.time()
while time.time() - t0 < args.seconds:
    strands = int(rng.integers(1, 3))
    b = rc.batch([[row() for _ in range(strands)] for _ in range(int(rng.integers(1, 41)))], strands)
    n, total = len(b[1]) // strands, len(b[3])
    counts = np.diff(b[2])
    max_cand = min(8192, int(counts.max())) if rng.random() < 0.7 else int(rng.integers(0, 250))
    params = (max_cand, int(rng.integers(1, 17)), int(rng.integers(1, 90)), int(rng.integers(1, 6)), int(rng.choice((1, 64, 128, 200, 256))))
    bare = rng.random() < 0.2
    sizes = (n, n * params[1] * 12, n + 1, total, total, total, n)
    full = [torch.full((s + (PAD * 12 if k == 1 else PAD),), rc.CANARY, dtype=torch.int64 if k == 2 else torch.int32, device=dev) for k, s in enumerate(sizes)]
    out = [x[:s] for x, s in zip(full, sizes)]
    out[1] = out[1].view(n, params[1], 12)
    if bare:
        out[2:7] = [None] * 5
    g = lambda x, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=dt))).to(dev)  # noqa: E731
    a.rank_chains_device(g(b[1], np.int32), g(b[2], np.int64), *(g(x, np.int32) for x in b[3:8]), None if bare else g(b[8], np.int32), strands, *params,
                         out=tuple(out))
    torch.cuda.synchronize()
    got = [x.cpu().numpy() for x in full]
    want = list(rc.expected(b, params, PAD, not bare))
    calls += 1
    reads += n
    cands += total
    refused += int((want[6][:n] != 0).sum())
    kept += int(want[0][:n].sum())
    if bare:
        for k in range(2, 7):
            want[k][:] = rc.CANARY
    for name, x, y in zip(NAMES, got, want):
        if (x != y).any():
            bad += 1
            if bad <= 5:
                k = np.flatnonzero(x != y)[:6]
                print("MISMATCH", name, strands, params, bare, k, x[k], y[k], b[2], flush=True)
print(f"rank_fuzz seed {args.seed}: {reads} reads, {cands} candidates ({refused} refused reads, {kept} kept chains) in {calls} calls, {bad} mismatches", flush=True)
sys.exit(1 if bad else 0)
