"""Local Smith-Waterman database search (protein.LocalSearch) on the configs[4] shape: the score pass (kernel A, sw_local_lane.hip), the
top-k selection and the full alignments of the top hits (kernel B, sw_local.hip).  Three workloads, the database seeded as in
scripts/protein_bench.py (log-normal lengths, BLOSUM62 11/1):
    Q400      400 queries of 300 residues against 5 000 database sequences (score pass repeated for at least --seconds)
    Q1280     the same with 1 280 queries
    mixed     400 queries of 100 .. 500 residues
Per workload: score-pass GCUPS, the top-k time for K = --top-k, kernel B's GCUPS over the K * Q hit pairs.
    python scripts/local_search_bench.py [--seconds 30] [--top-k 10] [--only Q400,Q1280,mixed] [--json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mgl_amd import protein, smithwaterman as sw  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--db", type=int, default=5000)
ap.add_argument("--seconds", type=float, default=30.0, help="repeat Q400's score pass for at least this long (the others: --steps)")
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--top-k", type=int, default=10)
ap.add_argument("--only", default="Q400,Q1280,mixed")
ap.add_argument("--json", action="store_true")
args = ap.parse_args()

rng = np.random.default_rng(42)
code, mat = protein.blosum62()
lens = np.clip(np.exp(rng.normal(5.7, 0.55, size=args.db)).astype(np.int64), 40, 2000)
lens.sort()
db_off = np.zeros(args.db + 1, np.int64)
np.cumsum(lens, out=db_off[1:])
db = protein.random_proteins(rng, 1, int(db_off[-1]))[0]


def queries_of(Q, lengths):
    qs = []
    for k in range(Q):
        L = int(lengths[k])
        q = protein.random_proteins(rng, 1, L)[0]
        if k % 5 == 0:  # a fifth are diverged fragments of database sequences
            d = int(rng.integers(0, args.db))
            if lens[d] >= L:
                s = int(rng.integers(0, lens[d] - L + 1))
                q = db[db_off[d] + s: db_off[d] + s + L].copy()
                mut = rng.random(L) < 0.4
                q[mut] = protein.random_proteins(rng, 1, int(mut.sum()))[0]
        qs.append(q.tobytes())
    return qs


dev = torch.device("cuda", 0)
a = sw.MicrosoftSmithWaterman(0)
assert a.load()
out = {}
for name in args.only.split(","):
    if name == "Q400":
        qs = queries_of(400, np.full(400, 300))
    elif name == "Q1280":
        qs = queries_of(1280, np.full(1280, 300))
    else:
        qs = queries_of(400, rng.integers(100, 501, 400))
    s = protein.LocalSearch(db, db_off, qs, dev)
    scores = s.score_pass(a, code, mat, 11, 1)  # warm-up
    torch.cuda.synchronize()
    assert a.fill_kernel_name(a.timing()) == "sw_local_lane_kernel", a.fill_kernel_name(a.timing())
    assert int(s.score_batch.status.abs().max()) == 0
    reps, t0 = 0, time.perf_counter()
    while True:
        scores = s.score_pass(a, code, mat, 11, 1)
        reps += 1
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        if (name == "Q400" and el >= args.seconds) or (name != "Q400" and reps >= args.steps):
            break
    score_s = el / reps
    for _ in range(2):  # top-k: warm-up, then timed
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        idx, top = s.top_k(scores, args.top_k)
        torch.cuda.synchronize()
        topk_s = time.perf_counter() - t1
    b = s.align_hits(a, code, mat, idx, 11, 1)  # warm-up
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    b = s.align_hits(a, code, mat, idx, 11, 1)
    torch.cuda.synchronize()
    b_s = time.perf_counter() - t2
    assert int(b.status.abs().max()) == 0 and torch.equal(b.hits[:, 0].view(len(qs), -1), top.to(torch.int32))
    idx_np = idx.cpu().numpy()
    b_cells = int(sum(lens[idx_np[q]].sum() * len(qs[q]) for q in range(len(qs))))
    out[name] = dict(queries=len(qs), cells=s.cells, score_pass_ms=score_s * 1e3, score_gcups=s.cells / score_s / 1e9, reps=reps,
                     topk_ms=topk_s * 1e3, k=args.top_k, align_ms=b_s * 1e3, align_pairs=int(idx_np.size), align_gcups=b_cells / b_s / 1e9)
    print(f"{name:6s} score pass {score_s * 1e3:8.2f} ms = {out[name]['score_gcups']:8.1f} GCUPS ({reps} reps)   top-{args.top_k} "
          f"{topk_s * 1e3:6.2f} ms   kernel B {b_s * 1e3:7.2f} ms over {idx_np.size} pairs = {out[name]['align_gcups']:6.1f} GCUPS", flush=True)
a.close()
if args.json:
    print(json.dumps(out))
