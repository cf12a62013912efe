"""mgl_sw_index_build_device, mgl_sw_seed_index_batch_device and mgl_sw_locate_window_batch_device against the textbook
(tests/index_textbook.py) on random inputs, scripts/strand_fuzz.py's kind: a reference of 1 .. 6 000 bases (now and then 20 000) over an
alphabet of 2 to 4 letters with repeats copied in and stray N or lower-case bytes; random k and w; the exported index bit for bit; then
1 .. 30 reads -- mutated pieces of the reference on either strand, or unrelated, or empty -- with random strands, max_occ, max_occ_ref,
merge, max_cand and a capacity that now and then cuts the rows: every output of the seed stage and the canaries behind them; then the
textbook's chains of those rows, through the textbook's choice, through locate with a random slack and max_tl, in place or not: every
output of that too.  Not a test: prints the references, reads, index entries, candidates, refused rows, windows, the calls and the
mismatches (expected 0).

  python scripts/index_fuzz.py --seconds 60 --seed 1
"""
import argparse, os, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import torch
import index_textbook as itb
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
WHERE_NAMES = ("t_start", "t_len", "anchor_t", "status")


def reference():
    r = rng.random()
    n = int(rng.integers(1, 40)) if r < 0.05 else int(rng.integers(15000, 20001)) if r < 0.12 else int(rng.integers(40, 6001))
    ref = bytearray(cases.rand_seq(rng, n, b"ACGT"[:int(rng.integers(2, 5))] if rng.random() < 0.7 else b"AT"))
    while n > 100 and rng.random() < 0.5:  # a repeat: a piece copied elsewhere, on either strand
        m = int(rng.integers(20, min(n // 2, 400)))
        x, y = int(rng.integers(0, n - m)), int(rng.integers(0, n - m))
        piece = bytes(ref[x:x + m])
        ref[y:y + m] = stb.revcomp(piece) if rng.random() < 0.3 else piece
    while rng.random() < 0.4:
        ref[int(rng.integers(n))] = int(rng.choice(list(b"Nacgt-")))
    return bytes(ref)


def read(ref):
    r = rng.random()
    if r < 0.05:
        return b""
    if r < 0.2:
        return cases.rand_seq(rng, int(rng.integers(1, 400)))
    m = int(rng.integers(1, min(len(ref), 1500) + 1))
    x = int(rng.integers(0, len(ref) - m + 1))
    q = cases.mutate(rng, ref[x:x + m]) if rng.random() < 0.8 else ref[x:x + m]
    q = bytearray(stb.revcomp(q) if rng.random() < 0.5 else q)
    while len(q) and rng.random() < 0.2:
        q[int(rng.integers(len(q)))] = int(rng.choice(list(b"Nacgt-")))
    return bytes(q)


def differ(names, got, want, what):
    global bad
    for name, x, y in zip(names, got, want):
        if x.shape != y.shape or (x != y).any():
            bad += 1
            if bad <= 5:
                i = np.flatnonzero(x != y)[:6] if x.shape == y.shape else None
                print("MISMATCH", name, what, i, None if i is None else (x[i], y[i]), flush=True)


refs = reads = entries = cands = refused = windows = calls = bad = 0
g = lambda x, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=dt))).to(dev)  # noqa: E731
t0 = time.time()
while time.time() - t0 < args.seconds:
    ref = reference()
    k, w = int(rng.integers(4, 17)), int(rng.integers(1, 33))
    want_index = itb.build_index(ref, k, w)
    table = itb.by_key(want_index)
    index = a.build_index(ref, k, w)
    keys, pos = (x.cpu().numpy() for x in index.export())
    differ(("keys", "positions"), (keys.astype(np.int64), pos.astype(np.int64)),
           (np.array([e[0] for e in want_index], np.int64), np.array([e[1] for e in want_index], np.int64)), (k, w, len(ref)))
    refs += 1
    entries += len(want_index)
    for _ in range(int(rng.integers(1, 4))):
        Qs = [read(ref) for _ in range(int(rng.integers(1, 31)))]
        strands, max_occ, merge = int(rng.integers(1, 3)), int(rng.integers(1, 65)), int(rng.integers(2))
        max_occ_ref = int(rng.choice((1, 2, 5, 64, 500, 8192)))
        max_cand = int(rng.choice((8192, 4096, 2048, 300, 40)))
        par = (k, w, strands, max_occ, max_occ_ref, merge, max_cand)
        total = itb.seed_index_batch(table, len(ref), Qs, *par, 1 << 30)[0][-1]
        cap = total + int(rng.integers(0, 9)) if rng.random() < 0.7 else int(rng.integers(0, total + 1))
        seeded = itb.seed_index_batch(table, len(ref), Qs, *par, cap)
        n, packed, _ = _pack_pairs(Qs, Qs, dev, 16, False)
        rows = strands * n
        sizes = (rows + 1, cap, cap, cap, rows, rows, rows)
        want = [np.full(s + PAD, cases.CANARY, np.int64 if i == 0 else np.int32) for i, s in enumerate(sizes)]
        for arr, vals in zip(want, (seeded[0], seeded[1], seeded[2], seeded[3], seeded[5], seeded[6], seeded[4])):
            arr[:len(vals)] = vals
        full = [torch.full((s + PAD,), cases.CANARY, dtype=torch.int64 if i == 0 else torch.int32, device=dev) for i, s in enumerate(sizes)]
        a.seed_index_device(index, *packed[3:6], strands, max_occ, max_occ_ref, merge, max_cand, cap, out=tuple(x[:s] for x, s in zip(full, sizes)))
        torch.cuda.synchronize()
        differ(SEED_NAMES, [x.cpu().numpy() for x in full], want, par + (cap, len(ref), [len(q) for q in Qs]))
        # the textbook's chains of the rows, its choice, and locate on the device
        chained = stb.chain_rows(seeded, max_cand, 64, 1000, 1000, 500, 38, 0)
        buf, q_start, q_len = itb.concat(Qs)
        start, at, aq, al = stb.select_strand(buf, q_start, q_len, *chained[:5])[2:6] if strands == 2 else chained[:4]
        slack, max_tl, in_place = int(rng.integers(0, 300)), int(rng.choice((100, 1000, 3000))), bool(rng.integers(2))
        where = itb.locate_window(len(ref), q_len, start, at, aq, al, slack, max_tl)
        tot = len(at)
        t_in = torch.full((tot + PAD,), cases.CANARY, dtype=torch.int32, device=dev)
        t_in[:tot] = g(at, np.int32)
        full = [torch.full((n + PAD,), cases.CANARY, dtype=torch.int64, device=dev), torch.full((n + PAD,), cases.CANARY, dtype=torch.int32, device=dev),
                t_in if in_place else torch.full((tot + PAD,), cases.CANARY, dtype=torch.int32, device=dev),
                torch.full((n + PAD,), cases.CANARY, dtype=torch.int32, device=dev)]
        a.locate_window_device(index, packed[5], g(start, np.int64), t_in[:tot], g(aq, np.int32), g(al, np.int32), slack, max_tl,
                               out=(full[0][:n], full[1][:n], full[2][:tot], full[3][:n]))
        torch.cuda.synchronize()
        want_t = [(at[i] if in_place else cases.CANARY) if v is None else v for i, v in enumerate(where[2])]
        want = [np.array(list(x) + [cases.CANARY] * PAD, np.int64) for x in (where[0], where[1], want_t, where[3])]
        differ(WHERE_NAMES, [x.cpu().numpy().astype(np.int64) for x in full], want, par + (slack, max_tl, in_place, len(ref)))
        calls += 1
        reads += n
        cands += int(seeded[0][-1])
        refused += sum(1 for s in seeded[4] if s)
        windows += sum(1 for x in where[1] if x > 0)
    index.close()
print(f"index_fuzz seed {args.seed}: {refs} references ({entries} index entries), {reads} reads, {cands} candidates ({refused} refused rows), "
      f"{windows} windows in {calls} calls, {bad} mismatches", flush=True)
sys.exit(1 if bad else 0)
