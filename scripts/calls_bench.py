"""What calling variants costs behind the pileup, on section 9o's workload: --reads reads of
mgl_amd.synth.repeat_mapping_set (about 10 kb, each from a place of its own in one reference of 26.6 Mb at 2 048 reads, every odd read
reverse-complemented), no copies; the mapper's parameters are scripts/pileup_bench.py's.  The reads lie one deep, so the sites are taken
with min_depth = min_alt = 1: every difference of a read is a site.  Every comparison is ONE run with both sides in it, passes taken
in turn after a warm-up each:

  (a)  map_reads_pileup_device against map_reads_calls_device (both allocate and zero their table), and the three new stages alone
       behind them -- pileup_sites_device into --sites slots, pileup_insertions_device, genotype_sites_device -- whose sum stands
       beside the difference
  (b)  pileup_device alone against pileup_insertions_device alone on the same tensors
  (c)  genotype_sites_device alone
  (d)  the same calls with numpy on the host, one pass, and the two compared record for record

Printed per line: the median pass and the spread -- the fastest and the slowest pass against the median pass.

  python scripts/calls_bench.py --reads 2048 --seconds 2
"""
import argparse, json, os, re, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=2048)
ap.add_argument("--length", type=int, default=10000)
ap.add_argument("--spacer", type=int, default=3000)
ap.add_argument("--band", type=int, default=64)
ap.add_argument("--seconds", type=float, default=2)
ap.add_argument("--max-cand", type=int, default=2048)
ap.add_argument("--slack", type=int, default=200)
ap.add_argument("--max-dist", type=int, default=1000)
ap.add_argument("--sites", type=int, default=0, help="site slots; 0: sized from a sizing pass, rounded up to a multiple of 65 536")
ap.add_argument("--max-ins", type=int, default=16)
ap.add_argument("--max-del", type=int, default=64)
ap.add_argument("--no-host", action="store_true", help="skip (d)")
args = ap.parse_args()
n = args.reads

import torch
from mgl_amd import synth
from mgl_amd.smithwaterman import MicrosoftSmithWaterman, GATK_PARAMETERS, concat, genotype_costs

dev = torch.device("cuda", 0)
a = MicrosoftSmithWaterman(0)
g = lambda x, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(x).astype(dt))).to(dev)  # noqa: E731
K, W = 15, 10
stride = 2 * (args.length + 2000)
stages = dict(max_occ=8, max_occ_ref=64, merge=True, max_cand=args.max_cand, max_pred=64, max_dist=args.max_dist, bw=500, pen_gap=38, pen_skip=0, max_chains=4,
              min_score=40, min_cnt=3, mask_level=128, slack=args.slack, strands=2, to_query_end=True, cigar_stride=stride, job_capacity=4 * n)
SITES = (1, 1, 64)
calling = dict(min_depth=1, min_alt=1, min_frac=64, max_ins=args.max_ins, max_del=args.max_del, error_phred=20)


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


def rows(names, secs, **more):
    out = []
    for name, s in zip(names, secs):
        s = np.sort(np.array(s))
        med = float(np.median(s))
        out.append(dict({"line": name, "ms_per_pass_median": round(med * 1e3, 4), "passes": len(s),
                         "spread_pct": [round((s[0] / med - 1) * 100, 2), round((s[-1] / med - 1) * 100, 2)]}, **more))
    for row in out[1:]:
        row["ms_median_vs_first"] = round(row["ms_per_pass_median"] / out[0]["ms_per_pass_median"], 4)
    for row in out:
        print(json.dumps(row), flush=True)
    return out


ref, reads, truth, _ = synth.repeat_mapping_set(43, n, args.length, args.spacer, 0, 0.0)
d, off = concat(reads)
ln = np.diff(off)
Q, max_ql = (g(np.concatenate([d, np.zeros(8, np.uint8)]), np.uint8), g(off[:-1], np.int64), g(ln, np.int32)), int(ln.max())
index = a.build_index(g(np.frombuffer(ref, np.uint8), np.uint8), K, W)
ref_len = len(ref)
map_tl = max(m for _, m, _ in truth) + 2 * args.slack + 500
head = (index, *Q, map_tl, max_ql, args.band, -1, GATK_PARAMETERS)

# ---- (a) the pipeline up to the pileup, and up to the calls
if args.sites <= 0:
    piled = a.map_reads_pileup_device(*head, **stages)
    sized = a.pileup_sites_device(piled[8][0], index.ref, 0, *SITES, 0, call=False, flags=False)
    args.sites = (int(sized[3][0].item()) + 65536) // 65536 * 65536
    del piled, sized
calling["site_capacity"] = args.sites
res = a.map_reads_calls_device(*head, **calling, **stages)
torch.cuda.synchronize()
jobs, window, aln, lines, table = res[3], res[4], res[5], res[7][0], res[8][0]
found, ins, called = res[9], res[10], res[11]
n_sites, n_calls = int(found[3][0].item()), int(called[1][0].item())
assert n_sites <= args.sites, "more sites than --sites slots"
kinds = np.bincount(called[0].cpu().numpy()[:n_calls, 1], minlength=4)[1:].tolist()
info = {"reads": n, "ref_len": ref_len, "alignments_counted": int((res[8][1] == 0).sum().item()), "site_slots": args.sites, "n_sites": n_sites, "n_calls": n_calls,
        "snv_del_ins_calls": kinds}
a_rows = rows(["(a) map_reads_pileup_device", "(a) map_reads_calls_device"],
              timed([lambda: a.map_reads_pileup_device(*head, **stages), lambda: a.map_reads_calls_device(*head, **calling, **stages)]), **info)

select = ((lines[:, 0] >= 0) & ((lines[:, 1] & 0x100) == 0)).to(torch.int32)
tensors = (index.ref, window[0], window[1], jobs[9], jobs[3], jobs[4], aln[0], aln[4], stride, aln[5])
one = table.clone()
sites_out = a.pileup_sites_device(table, index.ref, 0, *SITES, args.sites, call=False, flags=False)
ins_table = torch.zeros_like(ins[0])
new_stages = [lambda: a.pileup_sites_device(table, index.ref, 0, *SITES, args.sites, call=False, flags=False, out=sites_out),
              lambda: a.pileup_insertions_device(*tensors, found[2], found[3], aln[6], select, 0, args.max_ins, ins_table),
              lambda: a.genotype_sites_device(table, index.ref, found[2], found[3], ins[0], 0, args.max_ins, args.max_del, out=called)]
s_rows = rows(["(a) pileup_sites_device alone, %d slots" % args.sites, "(a) pileup_insertions_device alone", "(a) genotype_sites_device alone"], timed(new_stages))
print(json.dumps({"line": "(a) the calls behind the pileup", "ms_calls_minus_pileup": round(a_rows[1]["ms_per_pass_median"] - a_rows[0]["ms_per_pass_median"], 4),
                  "ms_sum_of_the_three_stages_alone": round(sum(r["ms_per_pass_median"] for r in s_rows), 4)}), flush=True)

# ---- (b) the pileup alone against the insertions alone, on the same tensors
spare = torch.zeros_like(table)
rows(["(b) pileup_device alone", "(b) pileup_insertions_device alone"],
     timed([lambda: a.pileup_device(*tensors, aln[6], select, (0, ref_len), spare), new_stages[1]]))

# ---- (c) the genotype alone
rows(["(c) genotype_sites_device alone, %d sites in %d slots" % (n_sites, args.sites)], timed([new_stages[2]]))

# ---- (d) the same calls with numpy on the host, from the device's own alignments, table and sites read back
if not args.no_host:
    cap = 4 * n
    keep = np.flatnonzero((res[8][1].cpu().numpy() == 0) & (select.cpu().numpy() != 0))
    rec, cg, cl = aln[0].cpu().numpy(), aln[4].cpu().numpy().reshape(cap, stride), aln[5].cpu().numpy()
    ts, qs, ori = window[0].cpu().numpy(), jobs[3].cpu().numpy(), jobs[9].cpu().numpy()
    counts = one.cpu().numpy().view(np.uint32)
    site = found[2].cpu().numpy()[:n_sites].astype(np.int64)
    refb = index.ref.cpu().numpy()
    lut = np.full(256, 4, np.int64)
    for k, pair in enumerate((b"Aa", b"Cc", b"Gg", b"Tt")):
        lut[list(pair)] = k
    M, cm, ch, ce = args.max_ins, *(lambda c: (c.cost_match, c.cost_het, c.cost_error))(genotype_costs(20))
    t0 = time.perf_counter()
    pos, flags, alt = site[:, 0], site[:, 1], site[:, 6]
    tab = np.zeros((n_sites, 6 * M + 1), np.int64)
    for j in keep:
        at, qat = int(ts[j]) + int(rec[j, 1]), int(qs[j]) + int(rec[j, 3])
        for num, op in re.findall(r"(\d+)([MID])", cg[j, :cl[j]].tobytes().decode()):
            m = int(num)
            if op == "I":
                k = int(np.searchsorted(pos, at - 1))
                if k < n_sites and pos[k] == at - 1:
                    if m > M:
                        tab[k, 0] += 1
                    else:
                        tab[k, m] += 1
                        np.add.at(tab[k], M + 1 + 5 * np.arange(m) + lut[ori[qat:qat + m]], 1)
                qat += m
            else:
                at, qat = at + m, qat + (m if op == "M" else 0)
    c = counts[:, pos].astype(np.int64)
    depth = c[:6].sum(axis=0)
    rch = lut[refb[pos]]
    cref = c[rch, np.arange(n_sites)]
    out = []
    snv = ((flags & 2) != 0) & (rch <= 3) & (alt >= 0) & (alt <= 3)
    s = np.flatnonzero(snv)
    out.append((s, np.full(len(s), 1), np.ones(len(s), np.int64), alt[s], cref[s], c[np.clip(alt[s], 0, 3), s], np.zeros(len(s), np.int64)))
    isdel = (flags & 4) != 0
    cont = np.zeros(n_sites, bool)
    cont[1:] = isdel[1:] & isdel[:-1] & (pos[1:] == pos[:-1] + 1)
    s = np.flatnonzero(isdel & ~cont)
    ends = np.append(np.flatnonzero(~cont), n_sites)
    run = ends[np.searchsorted(ends, s, side="right")] - s
    out.append((s, np.full(len(s), 2), np.minimum(run, args.max_del), np.full(len(s), -1), cref[s], c[5, s], (run > args.max_del).astype(np.int64)))
    words = tab[:, 1:M + 1]
    s = np.flatnonzero(((flags & 8) != 0) & (words.max(axis=1) > 0))
    out.append((s, np.full(len(s), 3), words[s].argmax(axis=1) + 1, np.full(len(s), -1), np.maximum(depth[s] - c[6, s], 0), words[s].max(axis=1), np.zeros(len(s), np.int64)))
    s, kind, length, al, r, av, fl = (np.concatenate([o[k] for o in out]) for k in range(7))
    order = np.lexsort((kind, s))
    s, kind, length, al, r, av, fl = (x[order] for x in (s, kind, length, al, r, av, fl))
    lik = np.stack([r * cm + av * ce, (r + av) * ch, av * cm + r * ce])
    pl = np.minimum((lik - lik.min(axis=0) + 128) >> 8, 2 ** 31 - 1)
    gt = lik.argmin(axis=0)
    gq = np.minimum(99, np.where(gt == 0, np.minimum(pl[1], pl[2]), np.where(gt == 1, np.minimum(pl[0], pl[2]), np.minimum(pl[0], pl[1]))))
    clip = lambda x: np.minimum(x, 2 ** 31 - 1)  # noqa: E731
    host = np.stack([pos[s], kind, length, rch[s], al, clip(depth[s]), clip(r), clip(av), gt, gq, pl[0], pl[0], pl[1], pl[2], fl, np.zeros(len(s), np.int64)], axis=1)
    seq = np.zeros((len(s), M), np.uint8)
    best = np.frombuffer(b"ACGTN", np.uint8)[tab[:, M + 1:].reshape(n_sites, M, 5).argmax(axis=2)]
    isins = kind == 3
    seq[isins] = np.where(np.arange(M)[None, :] < length[isins, None], best[s[isins]], 0)
    sec = time.perf_counter() - t0
    same = bool(len(host) == n_calls and (host == called[0].cpu().numpy()[:n_calls]).all() and (seq == called[2].cpu().numpy()[:n_calls]).all() and
                (tab == ins[0].cpu().numpy().view(np.uint32)[:n_sites]).all())
    print(json.dumps({"line": "(d) the same calls with numpy on the host, one pass", "ms": round(sec * 1e3, 1), "equal_to_the_device_calls": same}), flush=True)
    assert same
index.close()
