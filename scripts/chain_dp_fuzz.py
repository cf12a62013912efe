"""mgl_sw_chain_anchors_batch_device against the textbook (tests/chain_dp_textbook.py) on random batches: 1 .. 60 reads of 0 .. 200
candidates (now and then 300 .. 700), random parameters (max_pred 1 .. 64, distances, bw and penalties from 0 up), max_cand below some
reads' counts, and bad reads -- a bad candidate of each kind, a length below 1: every output of every read -- d_chain_start_out, the chain
arrays, the score, f, pred, the status -- and the canaries behind them.  Not a test: prints the reads run, their candidates, the refused
reads, the calls and the mismatches (expected 0).

  python scripts/chain_dp_fuzz.py --seconds 60 --seed 1
"""
import argparse, os, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import torch
import chain_dp_cases as cases
from mgl_amd.smithwaterman import MicrosoftSmithWaterman

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=60)
ap.add_argument("--seed", type=int, default=1)
args = ap.parse_args()
rng = np.random.default_rng(args.seed)
a = MicrosoftSmithWaterman(0)
dev = torch.device("cuda", 0)
PAD = 16
NAMES = ("chain_start", "chain_t", "chain_q", "chain_len", "score", "f", "pred", "status")


def read():
    r = rng.random()
    n = 0 if r < 0.08 else int(rng.integers(300, 701)) if r < 0.12 else int(rng.integers(1, 201))
    tl, ql, c = cases.random_read(rng, n, spread=int(rng.choice((3, 40, 300))), jitter=int(rng.choice((0, 6, 40))))
    if n and rng.random() < 0.06:  # one bad candidate, or a length below 1
        k = int(rng.integers(n))
        t, q, l = c[k]
        kind = int(rng.integers(7))
        if kind < 5:
            c[k] = [(t, q, 0), (-1, q, l), (t, -1, l), (tl - l + 1, q, l), (t, ql - l + 1, l)][kind]
        else:
            tl, ql = (0, ql) if kind == 5 else (tl, -3)
    return tl, ql, c


reads = cands = refused = calls = bad = 0
t0 = time.time()
while time.time() - t0 < args.seconds:
    batch = cases.csr([read() for _ in range(int(rng.integers(1, 61)))])
    n, total = len(batch[0]), len(batch[3])
    params = cases.random_params(rng, int(rng.integers(1, 65)))
    counts = np.diff(batch[2])
    max_cand = int(counts.max()) if rng.random() < 0.7 else int(rng.integers(0, 250))
    sizes = (n + 1, total, total, total, n, total, total, n)
    full = [torch.full((s + PAD,), cases.CANARY, dtype=torch.int64 if k == 0 else torch.int32, device=dev) for k, s in enumerate(sizes)]
    g = lambda x, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=dt))).to(dev)  # noqa: E731
    a.chain_anchors_device(g(batch[0], np.int32), g(batch[1], np.int32), g(batch[2], np.int64), g(batch[3], np.int32), g(batch[4], np.int32), g(batch[5], np.int32),
                           max_cand, params[0], params[1:3], *params[3:], out=tuple(x[:s] for x, s in zip(full, sizes)))
    torch.cuda.synchronize()
    got = [x.cpu().numpy() for x in full]
    want = cases.expected(batch, max_cand, params, PAD)
    calls += 1
    reads += n
    cands += total
    refused += int((want[7][:n] != 0).sum())
    for name, x, y in zip(NAMES, got, want):
        if (x != y).any():
            bad += 1
            if bad <= 5:
                k = np.flatnonzero(x != y)[:6]
                print("MISMATCH", name, params, max_cand, k, x[k], y[k], batch[2], flush=True)
print(f"chain_dp_fuzz seed {args.seed}: {reads} reads, {cands} candidates ({refused} refused reads) in {calls} calls, {bad} mismatches", flush=True)
sys.exit(1 if bad else 0)
