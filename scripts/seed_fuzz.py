"""mgl_sw_seed_batch_device against the textbook (tests/seed_textbook.py) on random batches: 1 .. 40 pairs of 0 .. 600 bases (now and then
1 000 .. 3 000) over alphabets of 2 to 4 letters with a stray N or lower-case byte now and then, the read a mutated copy of the window, a
piece of it or unrelated; random k (4 .. 16), w (1 .. 32), max_occ (1 .. 64), merge, max_cand (now and then below some pairs' raw hits) and
a capacity that now and then cuts the batch: every output -- d_cand_start_out, the candidate arrays, the status -- and the canaries
behind them.  Not a test: prints the pairs run, their candidates, the refused pairs, the calls and the mismatches (expected 0).

  python scripts/seed_fuzz.py --seconds 60 --seed 1
"""
import argparse, os, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import torch
import seed_cases as cases
import seed_textbook as tb
from mgl_amd.smithwaterman import MicrosoftSmithWaterman, _pack_pairs

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=60)
ap.add_argument("--seed", type=int, default=1)
args = ap.parse_args()
rng = np.random.default_rng(args.seed)
a = MicrosoftSmithWaterman(0)
dev = torch.device("cuda", 0)
PAD = 16
NAMES = ("cand_start", "cand_t", "cand_q", "cand_len", "status")


def pair():
    r = rng.random()
    n = 0 if r < 0.04 else int(rng.integers(1000, 3001)) if r < 0.10 else int(rng.integers(1, 601))
    T = bytearray(cases.rand_seq(rng, n, b"ACGT"[:int(rng.integers(2, 5))]))
    r = rng.random()
    Q = bytearray(cases.mutate(rng, bytes(T)) if r < 0.6 else bytes(T[len(T) // 3:2 * len(T) // 3 + 1]) if r < 0.8 else cases.rand_seq(rng, int(rng.integers(0, 400))))
    for s in (T, Q):
        while len(s) and rng.random() < 0.3:
            s[int(rng.integers(len(s)))] = int(rng.choice(list(b"Nacgt-")))
    return bytes(T), bytes(Q)


pairs = cands = refused = calls = bad = 0
t0 = time.time()
while time.time() - t0 < args.seconds:
    batch = [pair() for _ in range(int(rng.integers(1, 41)))]
    Ts, Qs = [p[0] for p in batch], [p[1] for p in batch]
    k, w, max_occ, merge = int(rng.integers(4, 17)), int(rng.integers(1, 33)), int(rng.integers(1, 65)), int(rng.integers(2))
    max_cand = int(rng.choice((8192, 4096, 2048, 300, 40)))
    total = tb.seed_batch(Ts, Qs, k, w, max_occ, merge, max_cand, 1 << 30)[0][-1]
    cap = total + int(rng.integers(0, 9)) if rng.random() < 0.7 else int(rng.integers(0, total + 1))
    want = cases.expected(Ts, Qs, k, w, max_occ, merge, max_cand, cap, PAD)
    n, packed, _ = _pack_pairs(Ts, Qs, dev, 16, False)
    sizes = (n + 1, cap, cap, cap, n)
    full = [torch.full((s + PAD,), cases.CANARY, dtype=torch.int64 if i == 0 else torch.int32, device=dev) for i, s in enumerate(sizes)]
    a.seed_device(*packed[:6], k, w, max_occ, merge, max_cand, cap, out=tuple(x[:s] for x, s in zip(full, sizes)))
    torch.cuda.synchronize()
    got = [x.cpu().numpy() for x in full]
    calls += 1
    pairs += n
    cands += int(want[0][n])
    refused += int((want[4][:n] != 0).sum())
    for name, x, y in zip(NAMES, got, want):
        if (x != y).any():
            bad += 1
            if bad <= 5:
                i = np.flatnonzero(x != y)[:6]
                print("MISMATCH", name, (k, w, max_occ, merge, max_cand, cap), i, x[i], y[i], [len(t) for t in Ts], flush=True)
print(f"seed_fuzz seed {args.seed}: {pairs} pairs, {cands} candidates ({refused} refused pairs) in {calls} calls, {bad} mismatches", flush=True)
sys.exit(1 if bad else 0)
