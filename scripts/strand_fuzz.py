"""mgl_sw_seed_strands_batch_device and mgl_sw_select_strand_batch_device against the textbook (tests/strand_textbook.py) on random
batches, scripts/seed_fuzz.py's kind: 1 .. 30 pairs of 0 .. 600 bases (now and then 1 000 .. 3 000) over alphabets of 2 to 4 letters
with a stray N or lower-case byte now and then; the read a mutated copy of the window or a piece of it, given on either strand, or
unrelated; now and then a window that holds both strands of its read; random k, w, max_occ, merge, max_cand and a capacity that now and
then cuts the rows.  Every output of the seed stage over the 2n rows and the canaries behind them; then the textbook's chains of those rows
through the choice: every output of that too.  Not a test: prints the pairs run, the candidates, the refused rows, the reads chosen on
strand 1, the calls and the mismatches (expected 0).

  python scripts/strand_fuzz.py --seconds 60 --seed 1
"""
import argparse, os, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import torch
import seed_cases as cases
import strand_textbook as stb
from mgl_amd.smithwaterman import MicrosoftSmithWaterman, _pack_pairs

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=60)
ap.add_argument("--seed", type=int, default=1)
args = ap.parse_args()
rng = np.random.default_rng(args.seed)
a = MicrosoftSmithWaterman(0)
dev = torch.device("cuda", 0)
PAD = 16
SEED_NAMES = ("cand_start", "cand_t", "cand_q", "cand_len", "row_t_len", "row_q_len", "status")
PICK_NAMES = ("strand", "queries_out", "anchor_start", "anchor_t", "anchor_q", "anchor_len", "score", "status")


def pair():
    r = rng.random()
    n = 0 if r < 0.04 else int(rng.integers(1000, 3001)) if r < 0.10 else int(rng.integers(1, 601))
    T = bytearray(cases.rand_seq(rng, n, b"ACGT"[:int(rng.integers(2, 5))] if rng.random() < 0.7 else b"AT"))
    r = rng.random()
    Q = cases.mutate(rng, bytes(T)) if r < 0.6 else bytes(T[len(T) // 3:2 * len(T) // 3 + 1]) if r < 0.8 else cases.rand_seq(rng, int(rng.integers(0, 400)))
    if rng.random() < 0.5:
        Q = stb.revcomp(Q)
    if rng.random() < 0.15:
        T += stb.revcomp(bytes(T[len(T) // 2:]))
    Q = bytearray(Q)
    for s in (T, Q):
        while len(s) and rng.random() < 0.3:
            s[int(rng.integers(len(s)))] = int(rng.choice(list(b"Nacgt-")))
    return bytes(T), bytes(Q)


def differ(names, got, want, what):
    global bad
    for name, x, y in zip(names, got, want):
        if (x != y).any():
            bad += 1
            if bad <= 5:
                i = np.flatnonzero(x != y)[:6]
                print("MISMATCH", name, what, i, x[i], y[i], flush=True)


pairs = cands = refused = reverse = calls = bad = 0
g = lambda x, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=dt))).to(dev)  # noqa: E731
t0 = time.time()
while time.time() - t0 < args.seconds:
    batch = [pair() for _ in range(int(rng.integers(1, 31)))]
    Ts, Qs = [p[0] for p in batch], [p[1] for p in batch]
    k, w, max_occ, merge = int(rng.integers(4, 17)), int(rng.integers(1, 33)), int(rng.integers(1, 65)), int(rng.integers(2))
    max_cand = int(rng.choice((8192, 4096, 2048, 300, 40)))
    total = stb.seed_strands_batch(Ts, Qs, k, w, max_occ, merge, max_cand, 1 << 30)[0][-1]
    cap = total + int(rng.integers(0, 9)) if rng.random() < 0.7 else int(rng.integers(0, total + 1))
    seeded = stb.seed_strands_batch(Ts, Qs, k, w, max_occ, merge, max_cand, cap)
    n, packed, _ = _pack_pairs(Ts, Qs, dev, 16, False)
    sizes = (2 * n + 1, cap, cap, cap, 2 * n, 2 * n, 2 * n)
    want = [np.full(s + PAD, cases.CANARY, np.int64 if i == 0 else np.int32) for i, s in enumerate(sizes)]
    for arr, vals in zip(want, (seeded[0], seeded[1], seeded[2], seeded[3], seeded[5], seeded[6], seeded[4])):
        arr[:len(vals)] = vals
    full = [torch.full((s + PAD,), cases.CANARY, dtype=torch.int64 if i == 0 else torch.int32, device=dev) for i, s in enumerate(sizes)]
    a.seed_strands_device(*packed[:6], k, w, max_occ, merge, max_cand, cap, out=tuple(x[:s] for x, s in zip(full, sizes)))
    torch.cuda.synchronize()
    differ(SEED_NAMES, [x.cpu().numpy() for x in full], want, (k, w, max_occ, merge, max_cand, cap, [len(t) for t in Ts]))
    # the textbook's chains of the rows through the choice
    cs, ct, cq, cl, score = stb.chain_rows(seeded, max_cand, 64, 1000, 1000, 500, 38, 0)[:5]
    tot = len(ct) + int(rng.integers(0, 4))
    buf = packed[3].cpu().numpy().tobytes()
    pick = stb.select_strand(buf, packed[4].cpu().numpy(), packed[5].cpu().numpy(), cs, ct, cq, cl, score, total_chain=tot)
    sizes = (n, len(buf), n + 1, tot, tot, tot, n, n)
    kinds = (np.int32, np.uint8, np.int64, np.int32, np.int32, np.int32, np.int32, np.int32)
    want = [np.full(s + PAD, 0xA5 if i == 1 else cases.CANARY, kind) for i, (s, kind) in enumerate(zip(sizes, kinds))]
    for i in (0, 2, 3, 4, 5, 6, 7):
        want[i][:len(pick[i])] = pick[i]
    for p in range(n):
        if pick[7][p] == 0:
            s, m = int(packed[4][p]), len(Qs[p])
            want[1][s:s + m] = np.frombuffer(pick[1][s:s + m], np.uint8)
    full = [torch.from_numpy(np.full(s + PAD, 0xA5 if i == 1 else cases.CANARY, kind)).to(dev) for i, (s, kind) in enumerate(zip(sizes, kinds))]
    pad = [0] * (tot - len(ct))
    a.select_strand_device(packed[3], packed[4], packed[5], g(cs, np.int64), g(ct + pad, np.int32), g(cq + pad, np.int32), g(cl + pad, np.int32),
                           g(score, np.int32), out=tuple(x[:s] for x, s in zip(full, sizes)))
    torch.cuda.synchronize()
    differ(PICK_NAMES, [x.cpu().numpy() for x in full], want, (k, w, max_occ, merge, max_cand, cap, [len(q) for q in Qs]))
    calls += 1
    pairs += n
    cands += int(seeded[0][-1])
    refused += sum(1 for s in seeded[4] if s)
    reverse += sum(pick[0])
print(f"strand_fuzz seed {args.seed}: {pairs} pairs, {cands} candidates ({refused} refused rows), {reverse} reads chosen on strand 1 in {calls} calls, "
      f"{bad} mismatches", flush=True)
sys.exit(1 if bad else 0)
