"""Random tiles and pairs through mgl_sw_local_batch_device_matrix, compared with the textbook DP (tests/local_textbook.py): kernel A's
scores on shared-target tiles (mixed query lengths, holes, random asymmetric matrices and gap models, o < e among them; one case in ten
with targets of up to 5 000 residues, checked a tile at a time with local_scores_np), kernel B's five fields and CIGAR on ragged pairs.
Prints the number of pairs compared and of mismatches; exits 1 on any mismatch.
    python scripts/local_fuzz.py --pairs 100000 [--seed 1] [--threads 16]"""
import argparse
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import local_textbook as lt  # noqa: E402

PROT = np.frombuffer(b"ARNDCQEGHILKMFPSTWYV", np.uint8)


def _want(job):
    t, q, code, mat, o, e, full = job
    r = lt.local_align_np(t, q, code, mat, o, e)
    return r if full else r[0]


def _want_tile(job):
    t, qs, code, mat, o, e = job
    return lt.local_scores_np(t, qs, code, mat, o, e)


def _mutate(rng, s):
    s = bytearray(s)
    for _ in range(int(rng.integers(0, 1 + len(s) // 6))):
        k = int(rng.integers(0, len(s) + 1))
        op = rng.integers(0, 3)
        if op == 0 and k < len(s):
            s[k] = int(PROT[rng.integers(20)])
        elif op == 1:
            s[k:k] = bytes(PROT[rng.integers(20, size=int(rng.integers(1, 6)))])
        elif k < len(s):
            del s[k:k + int(rng.integers(1, 6))]
    return bytes(s)


def _params(rng, protein):
    if rng.random() < 0.5:
        code, mat = protein.blosum62()
    else:
        mat = rng.integers(-int(rng.integers(1, 12)), int(rng.integers(1, 16)), size=(32, 32)).astype(np.int8)
        code = rng.integers(0, 32, 256).astype(np.uint8)
    o, e = [(11, 1), (10, 2), (5, 5), (9, 0), (0, 0), (3, 1), (1, 1), (1, 4)][int(rng.integers(8))]
    return code, mat, o, e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1))
    args = ap.parse_args()
    import torch

    from mgl_amd import protein, smithwaterman as sw

    rng = np.random.default_rng(args.seed)
    dev = torch.device("cuda", 0)
    a = sw.MicrosoftSmithWaterman(0)
    assert a.load()
    g = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    done = bad = rounds = 0
    t0 = time.time()
    with ProcessPoolExecutor(args.threads) as pool:
        while done < args.pairs:
            code, mat, o, e = _params(rng, protein)
            lane = rounds % 2 == 0
            long_t = rounds % 10 == 0  # one case in ten: kernel A over targets of thousands of residues (hundreds of strips)
            rounds += 1
            if long_t and o < e:
                o, e = e, o  # (the tile checker has no fast form for o < e)
            if lane:  # kernel A: tiles sharing their target
                n_tiles = int(rng.integers(1, 5 if long_t else 12))
                targets = [bytes(PROT[rng.integers(20, size=int(rng.integers(1, 5001 if long_t else 400)))]) for _ in range(n_tiles)]
                tix, qs = [], []
                for k in range(n_tiles):
                    for _ in range(128 if k < n_tiles - 1 else int(rng.integers(1, 129))):
                        r = rng.random()
                        cut = targets[k][int(rng.integers(0, len(targets[k]))):][: int(rng.integers(1, 400)) if long_t else None]
                        q = b"" if r < 0.03 else _mutate(rng, cut) if r < 0.5 else bytes(PROT[rng.integers(20, size=int(rng.integers(1, 400)))])
                        tix.append(k)
                        qs.append(q)
                ts = [targets[k] for k in tix]
                starts = np.concatenate([[0], np.cumsum([len(t) for t in targets])])[:-1][tix]
                tbytes = np.frombuffer(b"".join(targets) + b"\0" * 8, np.uint8).copy()
            else:  # kernel B: ragged pairs with everything
                n = int(rng.integers(64, 1500))
                ts, qs = [], []
                for _ in range(n):
                    t = bytes(PROT[rng.integers(20, size=int(rng.integers(0, 400)))])
                    q = _mutate(rng, t[int(rng.integers(0, len(t) + 1)):]) if rng.random() < 0.5 else bytes(PROT[rng.integers(20, size=int(rng.integers(0, 400)))])
                    ts.append(t)
                    qs.append(q)
                starts = np.concatenate([[0], np.cumsum([len(t) for t in ts])])[:-1]
                tbytes = np.frombuffer(b"".join(ts) + b"\0" * 8, np.uint8).copy()
            qoff = np.concatenate([[0], np.cumsum([len(q) for q in qs])])[:-1]
            b = protein.LocalBatch(g(tbytes), g(starts.astype(np.int64)), g(np.array([len(t) for t in ts], np.int32)),
                                   g(np.frombuffer(b"".join(qs) + b"\0" * 8, np.uint8).copy()), g(qoff.astype(np.int64)),
                                   g(np.array([len(q) for q in qs], np.int32)), max(1, max(len(t) for t in ts)), max(1, max(len(q) for q in qs)),
                                   0 if lane else 2048)
            protein.run_local(b, a, code, mat, o, e, score_only=lane, shared_target=lane)
            torch.cuda.synchronize()
            hits, st = b.hits.cpu().numpy(), b.status.cpu().numpy()
            cig = None if lane else b.cigar_strings()
            if long_t:
                per_tile = pool.map(_want_tile, [(targets[k], [q for x, q in zip(tix, qs) if x == k], code, mat, o, e) for k in range(n_tiles)])
                want = [int(w) for tile in per_tile for w in tile]
            else:
                want = list(pool.map(_want, [(t, q, code, mat, o, e, not lane) for t, q in zip(ts, qs)], chunksize=32))
            for k, w in enumerate(want):
                ok = st[k] == 0 and (hits[k, 0] == w and (hits[k, 1:] == 0).all() if lane else tuple(int(x) for x in hits[k]) == w[:5] and cig[k] == w[5])
                if not ok:
                    bad += 1
                    if bad <= 5:
                        print("MISMATCH", "A" if lane else "B", (o, e), ts[k], qs[k], hits[k], st[k], w, flush=True)
            done += len(qs)
            print(f"{done} pairs compared, {bad} mismatches ({time.time() - t0:.0f} s)", flush=True)
    a.close()
    print(f"local_fuzz: {done} pairs, {bad} mismatches")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
