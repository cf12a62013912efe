"""mgl_sw_describe_alignments_batch_device against the textbook (tests/describe_textbook.py) on random batches: 1 .. 200 alignments of
0 .. 40 elements (now and then 600 .. 1 500: more than one LDS chunk) of 1 .. 3, 40 or 300 bases (rarely one M of up to 20 000), at a
mismatch rate of 0, 0.05 or 0.5 over ACGT or a nine-letter alphabet, embedded at random offsets in longer sequences with random gaps
between the pairs; in text or binary; strides at the need, below it or far below it; now and then without MD, the extended CIGAR, the
status in or the status out; and bad alignments -- a sum one off, a span outside its sequence, a foreign byte or word in the slot, a
zero length, a length above the stride, a status going in over a poisoned slot: every output of every alignment and the canaries behind
the arrays and the texts.  Not a test: prints the alignments run, their columns, the refused and the overflowing ones, the calls and the
mismatches (expected 0).

  python scripts/describe_fuzz.py --seconds 60 --seed 1
"""
import argparse, os, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import torch
import describe_cases as dc
import describe_textbook as dtb
from mgl_amd.smithwaterman import MicrosoftSmithWaterman

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=60)
ap.add_argument("--seed", type=int, default=1)
args = ap.parse_args()
rng = np.random.default_rng(args.seed)
a = MicrosoftSmithWaterman(0)
dev = torch.device("cuda", 0)
NAMES = ("stats", "md", "xcigar", "status")


def alignment(binary):
    r = rng.random()
    alphabet = b"ACGT" if rng.random() < 0.8 else b"ACGTNacgt"
    if r < 0.02:
        t = dc.seq(rng, int(rng.integers(5000, 20001)), alphabet)
        t, q, cg = t, dc.mutate(rng, t, float(rng.choice((0.0, 0.01, 0.3))), alphabet), [(len(t), "M")]
    else:
        els = int(rng.integers(600, 1501)) if r < 0.05 else int(rng.integers(0, 41))
        t, q, cg = dc.random_alignment(rng, els, alphabet, float(rng.choice((0.0, 0.05, 0.5))), int(rng.choice((3, 40, 300))) if els <= 40 else 3)
    c = dc.embedded(rng, t, q, cg, *(int(x) for x in rng.integers(0, 40, 4)))
    if rng.random() < 0.1:  # a bad one
        kind = int(rng.integers(7))
        slot = dtb.cigar_bytes(cg, binary)
        if kind == 0:
            c = c._replace(cigar=cg + [(1, "MID"[int(rng.integers(3))])], want=dc.BAD_ARG)
        elif kind == 1 and cg:
            n, op = cg[-1]
            c = c._replace(cigar=cg[:-1] + [(n + 1, op)], want=dc.BAD_ARG)
        elif kind == 2:
            rec = list(c.rec)
            rec[int(rng.integers(4))] += int(rng.choice((-1, 1))) * (len(c.t) + len(c.q) + 1)
            c = c._replace(rec=tuple(rec), want=dc.BAD_ARG)
        elif kind == 3 and slot:
            k = int(rng.integers(len(slot)))
            bad = bytes([int(rng.choice((0x0f, 0xff, 0x53, 0x04)))]) if binary and k % 4 == 0 else bytes([int(rng.choice((ord("S"), ord("="), 0, 0x80, ord(" "))))])
            if not binary or k % 4 == 0:
                c = c._replace(cigar=None, slot=slot[:k] + bad + slot[k + 1:], want=dc.BAD_ARG)
        elif kind == 4 and cg:
            k = int(rng.integers(len(cg)))
            zero = dtb.cigar_bytes(cg[:k], binary) + (b"\0\0\0\0" if binary else b"0M") + dtb.cigar_bytes(cg[k:], binary)
            c = c._replace(cigar=None, slot=zero, want=dc.BAD_ARG)
        elif kind == 5:
            c = c._replace(cigar=None, slot=slot, cigar_len=int(rng.choice((-1, -4, 1 << 24, 1 << 30))), want=dc.BAD_ARG)
        elif kind == 6:
            c = c._replace(cigar=None, slot=b"\xff" * (len(slot) // 4 * 4), rec=(-5, 1 << 29, 9, -1), cigar_len=1 << 29, status_in=int(rng.choice((1, 3, 5))))
    return c


count = cols = refused = over = calls = bad = 0
t0 = time.time()
while time.time() - t0 < args.seconds:
    binary = bool(rng.random() < 0.5)
    cases = [alignment(binary) for _ in range(int(rng.integers(1, 201)))]
    no_status_in = rng.random() < 0.15
    if no_status_in:
        cases = [c for c in cases if not c.status_in] or [dc.case(b"A", b"A", [(1, "M")])]
    n = len(cases)
    gaps = [tuple(int(x) for x in rng.integers(0, 17, 2)) for _ in cases]
    gaps[0] = (0, 0)
    p = dc.pack(cases, binary, None, gaps)
    ds = [dc.described(c) for c in cases if not c.status_in and not c.want]
    need_md, need_xc = max([len(d.md) for d in ds] + [1]), (max([len(dtb.xcigar_bytes(d.xcigar, binary)) for d in ds] + [4]) + 3) // 4 * 4
    r = rng.random()
    md_stride = need_md if r < 0.6 else max(1, need_md - 1) if r < 0.8 else int(rng.integers(1, need_md + 1))
    unit = 4 if binary else 1
    r = rng.random()
    xc_stride = need_xc if r < 0.6 else max(unit, need_xc - unit) if r < 0.8 else int(rng.integers(1, need_xc // unit + 1)) * unit
    md, xc, status = rng.random() < 0.85, rng.random() < 0.85, rng.random() < 0.85
    g = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    i32 = lambda m: torch.full((m + dc.PAD,), dc.CANARY, dtype=torch.int32, device=dev)  # noqa: E731
    u8 = lambda m: torch.full((m + dc.PAD,), dc.CANARY_BYTE, dtype=torch.uint8, device=dev)  # noqa: E731
    out = (i32(8 * n), u8(n * md_stride) if md else None, u8(n * xc_stride) if xc else None, i32(n) if status else None)
    a.describe_device(g(p["targets"]), g(p["t_start"]), g(p["t_len"]), g(p["queries"]), g(p["q_start"]), g(p["q_len"]), g(p["aln"]), g(p["cigar"]),
                      p["cigar_stride"], g(p["cigar_len"]), None if no_status_in else g(p["status_in"]), md_stride, xc_stride, binary, out=out)
    torch.cuda.synchronize()
    want = dc.expected(cases, binary, md_stride, xc_stride, md, xc)
    calls += 1
    count += n
    cols += sum(dtb.block_len(d) for d in ds)
    refused += int((want[3][:n] == dc.BAD_ARG).sum())
    over += int((want[3][:n] == dc.OVERFLOW).sum())
    for name, x, y in zip(NAMES, out, want):
        if x is None:
            continue
        x = x.cpu().numpy()
        if (x != y).any():
            bad += 1
            if bad <= 5:
                k = np.flatnonzero(x != y)[:6]
                print("MISMATCH", name, "binary" if binary else "text", n, md_stride, xc_stride, k, x[k], y[k], flush=True)
print(f"describe_fuzz seed {args.seed}: {count} alignments, {cols} columns ({refused} refused, {over} overflowing) in {calls} calls, {bad} mismatches", flush=True)
sys.exit(1 if bad else 0)
