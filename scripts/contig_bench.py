"""What a reference of contigs costs the read mapper: section 9k's workload -- --reads reads of
mgl_amd.synth.mapping_set (about 10 kb, --distinct of them laid into one reference, every odd read reverse-complemented); (k, w) =
(15, 10), max_occ 8, max_occ_ref 64, merged; GATK parameters, band 64, Z-drop off, to the query's end; section 9i's chaining parameters;
max_chains 4, min_score 40, min_cnt 3, mask_level 128.  Lines in ONE run, passes taken in turn after a warm-up each:

  (a)  map_reads_ranked_device on the index of build_index -- the parent's path and the yardstick
  (b)  the same reference as ONE contig through the contig stages (contig_of, the grouped chain kernel, the clipped window)
  (c)  the reference cut into 64 contigs inside its spacers (synth.contig_cuts), the byte at every cut overwritten with N
  (d)  the same with 4 097 contigs: the table no longer fits LDS
  (e)  chain_anchors_device alone on (a)'s candidates, f and pred written; (e') the same grouped, every candidate in group 0;
       (e'') grouped by the 64 contigs
  (f)  contig_of_device alone on those candidates against 1, 64 and 4 097 contigs

Printed per line: reads/s over all passes, the median pass and the spread -- the fastest and the slowest pass against the median pass;
for (b), (c), (d) the median against (a)'s, for (e'), (e'') against (e)'s.

  python scripts/contig_bench.py --reads 2048 --distinct 2048 --seconds 3
"""
import argparse, json, os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=2048)
ap.add_argument("--length", type=int, default=10000)
ap.add_argument("--spacer", type=int, default=3000)
ap.add_argument("--band", type=int, default=64)
ap.add_argument("--seconds", type=float, default=3)
ap.add_argument("--distinct", type=int, default=2048)
ap.add_argument("--contigs", type=int, nargs=2, default=(64, 4097))
ap.add_argument("--max-cand", type=int, default=2048)
ap.add_argument("--slack", type=int, default=200)
ap.add_argument("--max-dist", type=int, default=1000)
args = ap.parse_args()
n = args.reads

import torch
from mgl_amd import synth
from mgl_amd.smithwaterman import MicrosoftSmithWaterman, GATK_PARAMETERS, concat

distinct = min(n, args.distinct)
ref, base_reads, base_truth = synth.mapping_set(43, distinct, args.length, args.spacer)
reads = [base_reads[i % distinct] for i in range(n)]
dev = torch.device("cuda", 0)
a = MicrosoftSmithWaterman(0)
g = lambda x, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(x).astype(dt))).to(dev)  # noqa: E731
d, off = concat(reads)
ln = np.diff(off)
Q, max_ql = (g(np.concatenate([d, np.zeros(8, np.uint8)]), np.uint8), g(off[:-1], np.int64), g(ln, np.int32)), int(ln.max())
K, W = 15, 10


def cut(count):
    """-> (the reference with N at the cuts, starts, lens)"""
    cuts = synth.contig_cuts(distinct, base_truth, args.spacer, count)
    buf = np.frombuffer(ref, np.uint8).copy()
    buf[cuts] = ord("N")
    edges = [-1] + cuts + [len(ref)]
    return g(buf, np.uint8), [e + 1 for e in edges[:-1]], [b - e - 1 for e, b in zip(edges, edges[1:])]


plain = a.build_index(g(np.frombuffer(ref, np.uint8), np.uint8), K, W)
indexes = [plain, a.build_index_contigs_device(plain.ref, [0], [len(ref)], k=K, w=W)] + [a.build_index_contigs_device(*cut(c), k=K, w=W) for c in args.contigs]
map_tl = max(m for _, m, _ in base_truth) + 2 * args.slack + 500
stride = 2 * (args.length + 2000)
index_par = dict(max_occ=8, max_occ_ref=64, merge=True)
chain_par = dict(max_pred=64, max_dist=args.max_dist, bw=500, pen_gap=38, pen_skip=0)
rank_par = (4, 40, 3, 128)
i32 = lambda m: torch.zeros(m, dtype=torch.int32, device=dev)  # noqa: E731
i64 = lambda m: torch.zeros(m, dtype=torch.int64, device=dev)  # noqa: E731

# the seed stage once at a capacity that surely holds the batch, to size the arrays of the timed calls by what it found
first = a.seed_index_device(plain, *Q, 2, 8, 64, True, args.max_cand)
torch.cuda.synchronize()
assert int((first[6] != 0).sum()) == 0, "a row was refused: raise --max-cand"
total = int(first[0][2 * n].item())
del first


def mapper(index):
    """-> (the call, its output tuples): buffers of its own"""
    seed = (i64(2 * n + 1), i32(total), i32(total), i32(total), i32(2 * n), i32(2 * n), i32(2 * n))
    chain = (i64(2 * n + 1), i32(total), i32(total), i32(total), i32(2 * n), i32(total), i32(total), i32(2 * n))
    pick = (i32(n), torch.zeros_like(Q[0]), i64(n + 1), i32(total), i32(total), i32(total), i32(n), i32(n))
    where = (i64(n), i32(n), i32(total), i32(n)) + ((i32(n),) if index.contigs is not None else ())
    out = (torch.zeros((n, 8), dtype=torch.int32, device=dev), None, None, None, torch.zeros(n * stride, dtype=torch.uint8, device=dev), i32(n), i32(n))
    rank = (i32(n), torch.zeros((n, 4, 12), dtype=torch.int32, device=dev), None, None, None, None, i32(n))

    def call():
        a.map_reads_ranked_device(index, *Q, map_tl, max_ql, args.band, -1, GATK_PARAMETERS, 2, args.max_cand, total, seed, chain, *rank_par, rank_out=rank,
                                  slack=args.slack, select_out=pick, locate_out=where, out=out, to_query_end=True, cigar_stride=stride, **index_par, **chain_par)
    return call, (seed, chain, pick, where, out, rank)


mappers = [mapper(ix) for ix in indexes]
for call, _ in mappers:
    call()
torch.cuda.synchronize()
(seed_a, chain_a, pick_a, where_a, out_a, rank_a), (_, chain_b, pick_b, where_b, out_b, rank_b) = mappers[0][1], mappers[1][1]
assert all(bool((x == y).all()) for x, y in zip((chain_a[0], chain_a[4], pick_a[0], where_a[0], where_a[1], out_a[0], out_a[5], out_a[6], rank_a[0], rank_a[1]),
                                                 (chain_b[0], chain_b[4], pick_b[0], where_b[0], where_b[1], out_b[0], out_b[5], out_b[6], rank_b[0], rank_b[1]))), \
    "one contig does not map as the plain index does"
mapped = [int((m[1][4][6] == 0).sum()) for m in mappers]
rid_ok = []
for (_, (_, _, _, where, out, _)), ix in zip(mappers[2:], indexes[2:]):  # every mapped read in the contig that holds its true place
    truth_rid = np.searchsorted(ix.contigs.starts, [base_truth[i % distinct][0] for i in range(n)], side="right") - 1
    ok = (out[6] == 0).cpu().numpy()
    rid_ok.append(int((where[4].cpu().numpy()[ok] == truth_rid[ok]).sum()))

groups = [ix.contig_of_device(seed_a[1], seed_a[3]) for ix in indexes[1:]]
chain_e, chain_e1, chain_e2 = ((i64(2 * n + 1), i32(total), i32(total), i32(total), i32(2 * n), i32(total), i32(total), i32(2 * n)) for _ in range(3))
group_out = i32(total)


def chain_call(out, group):
    return lambda: a.chain_anchors_device(seed_a[4], seed_a[5], *seed_a[:4], args.max_cand, out=out, group=group, **chain_par)


def timed(calls):
    """a warm-up pass of each, then passes of the calls in turn until the first has args.seconds of GPU time: the seconds of every pass, per call"""
    for call in calls:
        call()
    torch.cuda.synchronize()
    secs = [[] for _ in calls]
    while sum(secs[0]) < args.seconds:
        for x, call in enumerate(calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); call(); e1.record(); torch.cuda.synchronize()
            secs[x].append(e0.elapsed_time(e1) * 1e-3)
    return secs


def rows(names, secs):
    out = []
    for name, s in zip(names, secs):
        s = np.sort(np.array(s))
        med = float(np.median(s))
        out.append({"line": name, "reads": n, "reads_per_s": round(n * len(s) / float(s.sum()), 1), "ms_per_pass_median": round(med * 1e3, 4), "passes": len(s),
                    "spread_pct": [round((s[0] / med - 1) * 100, 2), round((s[-1] / med - 1) * 100, 2)]})
    for row in out[1:]:
        row["ms_median_vs_first"] = round(row["ms_per_pass_median"] / out[0]["ms_per_pass_median"], 4)
    return out


names = ["(a) map_reads_ranked_device, no contigs", "(b) ONE contig through the contig stages"] + ["(%s) %d contigs" % (x, c) for x, c in zip("cd", args.contigs)]
out = rows(names, timed([m[0] for m in mappers]))
out[0].update({"ref_len": len(ref), "candidates_per_read_both_rows": round(total / n, 1)})
for row, m, c in zip(out, mapped, [None, None] + rid_ok):
    row.update({"mapped": m, "in_the_true_contig": c})
out += rows(["(e) chain_anchors_device alone, f and pred written", "(e') grouped, one group", "(e'') grouped by %d contigs" % args.contigs[0]],
            timed([chain_call(chain_e, None), chain_call(chain_e1, groups[0]), chain_call(chain_e2, groups[1])]))
assert all(bool((x == y).all()) for x, y in zip(chain_e, chain_e1)), "one group does not chain as no groups do"
out += rows(["(f) contig_of_device alone, %d contigs, %d anchors" % (len(ix.contigs.starts), total) for ix in indexes[1:]],
            timed([(lambda ix=ix: ix.contig_of_device(seed_a[1], seed_a[3], out=group_out)) for ix in indexes[1:]]))
for row in out:
    print(json.dumps(row), flush=True)
for ix in indexes:
    ix.close()
