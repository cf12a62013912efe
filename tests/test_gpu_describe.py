"""mgl_sw_describe_alignments_batch_device on the GPU against tests/describe_textbook.py, bit for bit, in text and in binary: every
output array starts as canaries, is 16 entries longer than its size, and must come back as describe_cases.expected builds it -- the
canaries behind every array and behind each text's length included.  The cases are tests/describe_cases.py's: the seams of the 64-column
step, the digit borders of a run, deletions, insertions, more elements than one LDS chunk, every byte offset of the spans, every
refusal between two good alignments, strides at, below and far below the need, null outputs, a batch larger than the grid's waves,
and the entry directly behind the two alignment entries on a side stream."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import describe_cases as dc  # noqa: E402
import describe_textbook as dtb  # noqa: E402
from mgl_amd import _lib, formats  # noqa: E402

pytestmark = pytest.mark.gpu

GATK = (200, -150, 260, 11)
BINARY = pytest.mark.parametrize("binary", [False, True], ids=["text", "binary"])


@pytest.fixture(scope="module")
def aligner():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mgl_amd import smithwaterman as sw

    a = sw.MicrosoftSmithWaterman(0)
    assert a.load()
    yield a
    a.close()


def _need(cases, binary):
    """the longest MD and extended CIGAR among the good cases"""
    ds = [dc.described(c) for c in cases if not c.status_in and not c.want]
    return max([len(d.md) for d in ds] + [1]), max([len(dtb.xcigar_bytes(d.xcigar, binary)) for d in ds] + [4])


def run(aligner, cases, binary, gaps=None, md_stride=None, xcigar_stride=None, md=True, xcigar=True, status=True, status_in=True, cigar_stride=None):
    dev = torch.device("cuda", 0)
    n = len(cases)
    p = dc.pack(cases, binary, cigar_stride, gaps)
    need_md, need_xc = _need(cases, binary)
    md_stride = need_md if md_stride is None else md_stride
    xcigar_stride = (need_xc + 3) // 4 * 4 if xcigar_stride is None else xcigar_stride
    assert status_in or not any(c.status_in for c in cases)
    g = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    i32 = lambda m: torch.full((m + dc.PAD,), dc.CANARY, dtype=torch.int32, device=dev)  # noqa: E731
    u8 = lambda m: torch.full((m + dc.PAD,), dc.CANARY_BYTE, dtype=torch.uint8, device=dev)  # noqa: E731
    out = (i32(8 * n), u8(n * md_stride) if md else None, u8(n * xcigar_stride) if xcigar else None, i32(n) if status else None)
    got = aligner.describe_device(g(p["targets"]), g(p["t_start"]), g(p["t_len"]), g(p["queries"]), g(p["q_start"]), g(p["q_len"]), g(p["aln"]),
                                  g(p["cigar"]), p["cigar_stride"], g(p["cigar_len"]), g(p["status_in"]) if status_in else None, md_stride, xcigar_stride,
                                  binary, out=out)
    torch.cuda.synchronize()
    assert got is out
    want = dc.expected(cases, binary, md_stride, xcigar_stride, md, xcigar)
    names = ("stats", "md", "xcigar", "status")
    for name, x, y in zip(names, out, want):
        if x is None:
            continue
        x = x.cpu().numpy()
        if not (x == y).all():
            k = int(np.flatnonzero(x != y)[0])
            per = {"stats": 8, "md": md_stride, "xcigar": xcigar_stride, "status": 1}[name]
            c = cases[min(k // per, n - 1)]
            raise AssertionError("%s differs first at entry %d (case %d, entry %d of it): got %r, want %r; cigar %r" % (
                name, k, k // per, k % per, x[k:k + 12].tolist(), y[k:k + 12].tolist(), dc.slot_of(c, binary)[:60]))
    return want


@BINARY
def test_step_seams_and_digit_borders(aligner, binary):
    run(aligner, dc.seam_cases(np.random.default_rng(1)), binary)


@BINARY
def test_indels_chunks_and_bytes(aligner, binary):
    cases = dc.indel_cases(np.random.default_rng(2))
    assert max(len(c.cigar) for c in cases) == 6000 > 512  # more than one LDS chunk
    run(aligner, cases, binary)


@BINARY
def test_every_byte_offset(aligner, binary):
    cases, gaps = dc.offset_cases(np.random.default_rng(3))
    p = dc.pack(cases, binary, None, gaps)
    assert {int((s + c.rec[0]) % 16) for s, c in zip(p["t_start"][1:17], cases[1:17])} == set(range(16))
    assert {int((s + c.rec[2]) % 16) for s, c in zip(p["q_start"][1:17], cases[1:17])} == set(range(16))
    assert p["t_start"][0] + cases[0].rec[0] == 0 and p["t_start"][-1] + cases[-1].rec[1] == len(p["targets"])  # the very start, the very end
    assert p["q_start"][0] + cases[0].rec[2] == 0 and p["q_start"][-1] + cases[-1].rec[3] == len(p["queries"])
    run(aligner, cases, binary, gaps)


def test_refusals_in_text(aligner):
    cases = dc.refusals(np.random.default_rng(4))
    want = run(aligner, cases, False)
    assert sorted(set(want[3][:len(cases)].tolist())) == [0, dc.BAD_ARG, 5]


def test_refusals_in_binary(aligner):
    cases = dc.binary_refusals(np.random.default_rng(5))
    want = run(aligner, cases, True)
    assert sorted(set(want[3][:len(cases)].tolist())) == [0, dc.BAD_ARG, 5]


def test_a_cigar_longer_than_the_stride_is_refused(aligner):
    rng = np.random.default_rng(6)
    t = dc.seq(rng, 30)
    good = lambda: dc.case(t, dc.mutate(rng, t, 0.2), [(12, "M"), (18, "M")])  # noqa: E731  (six bytes: it fits)
    cases = [good(), dc.case(t, t, [(10, "M"), (10, "M"), (10, "M")], cigar_len=9, want=dc.BAD_ARG), good()]
    run(aligner, cases, False, cigar_stride=8)


@BINARY
def test_strides_at_below_and_far_below_the_need(aligner, binary):
    rng = np.random.default_rng(7)
    cases = [dc.case(*dc.random_alignment(rng, 12, p_mismatch=0.3)) for _ in range(6)]
    need_md, need_xc = _need(cases, binary)
    unit = 4 if binary else 1
    for md_stride, xc_stride in ((need_md, need_xc), (need_md - 1, need_xc), (need_md, need_xc - unit), (need_md - 1, need_xc - unit), (3, 4), (1, unit)):
        want = run(aligner, cases, binary, md_stride=md_stride, xcigar_stride=xc_stride)
        assert (dc.OVERFLOW in want[3][:6]) == (md_stride < need_md or xc_stride < need_xc)


@BINARY
def test_null_outputs_and_an_empty_batch(aligner, binary):
    rng = np.random.default_rng(8)
    cases = [dc.case(*dc.random_alignment(rng, 8, p_mismatch=0.2)) for _ in range(5)]
    run(aligner, cases, binary, md=False, xcigar=False)  # a sizing pass: the lengths still right, no overflow
    run(aligner, cases, binary, md=False)
    run(aligner, cases, binary, xcigar=False, status=False, status_in=False)
    run(aligner, [], binary)


@BINARY
def test_a_batch_larger_than_the_grid(aligner, binary):
    cases = dc.mixed_batch(np.random.default_rng(9), 300)
    assert len(cases) == 300
    run(aligner, cases, binary)
    big = cases * 24  # 7 200 alignments: more than the waves of the largest grid, so the persistent loop turns
    run(aligner, big, binary)


@BINARY
def test_directly_behind_the_alignment_entries(aligner, binary):
    from mgl_amd.smithwaterman import _pack_pairs

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(10)
    ts, qs, seeds = [], [], []
    for _ in range(12):
        core = dc.seq(rng, 400)
        q = dc.mutate(rng, core, 0.03)
        q = q[:150] + dc.seq(rng, 3) + q[150:260] + q[270:]  # an insertion and a deletion
        ts.append(dc.seq(rng, 30) + core + dc.seq(rng, 25))
        qs.append(q)
        seeds.append((30 + 40, 40, 20))
    n, packed, stride = _pack_pairs(ts, qs, dev, None, binary)
    g = lambda x: torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.int32))).to(dev)  # noqa: E731
    sd = np.asarray(seeds, np.int32)
    start = torch.arange(n + 1, dtype=torch.int64, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain = aligner.align_chain_device(*packed[:6], start, g(sd[:, 0]), g(sd[:, 1]), g(sd[:, 2]), *packed[6:], 0, 0, 32, -1, GATK, True, stride, binary)
        d_chain = aligner.describe_device(*packed[:6], chain[0], chain[4], stride, chain[5], chain[6], binary_cigar=binary)
        seed = aligner.extend_seed_device(*packed[:6], g(sd[:, 0]), g(sd[:, 1]), g(sd[:, 2]), *packed[6:], 32, -1, GATK, False, stride, binary)
        d_seed = aligner.describe_device(*packed[:6], seed[0], seed[3], stride, seed[4], seed[5], binary_cigar=binary)
    torch.cuda.synchronize()  # the one synchronisation
    for aln, cg, ln, st, desc in ((chain[0], chain[4], chain[5], chain[6], d_chain), (seed[0], seed[3], seed[4], seed[5], d_seed)):
        rec, cg, ln, st = aln.cpu().numpy(), cg.cpu().numpy().reshape(n, stride), ln.cpu().numpy(), st.cpu().numpy()
        stats, md, xc, dst = (x.cpu().numpy() for x in desc)
        assert not st.any() and not dst.any()
        md, xc = md.reshape(n, stride), xc.reshape(n, stride)
        kinds = set()
        for p in range(n):
            raw = cg[p, :ln[p]].tobytes()
            els = [(int(w) >> 4, "MID"[int(w) & 15]) for w in np.frombuffer(raw, "<u4")] if binary else formats.cigar_text_to_elements(raw.decode())
            d = dtb.describe(ts[p][rec[p, 1]:rec[p, 2]], qs[p][rec[p, 3]:rec[p, 4]], els)
            assert stats[p].tolist() == dtb.stats(d, binary), p
            assert md[p, :stats[p, 6]].tobytes() == d.md and xc[p, :stats[p, 7]].tobytes() == dtb.xcigar_bytes(d.xcigar, binary), p
            kinds |= {op for _, op in d.xcigar}
        assert {"=", "X"} <= kinds <= set("=XID")


def test_over_lists(aligner):
    rng = np.random.default_rng(11)
    als = [dc.random_alignment(rng, 7, p_mismatch=0.2) for _ in range(9)]
    for binary in (False, True):
        stats, mds, xcs = aligner.describe([a[0] for a in als], [a[1] for a in als], [dtb.xcigar_text(a[2]) for a in als], binary_cigar=binary)
        for (t, q, cg), s, m, x in zip(als, stats, mds, xcs):
            d = dtb.describe(t, q, cg)
            assert list(s)[:7] == dtb.stats(d)[:7] and m == d.md and x == dtb.xcigar_text(d.xcigar)
    with pytest.raises(_lib.MglSwError):
        aligner.describe([b"ACGT"], [b"ACGT"], ["3M"])
    assert aligner.describe([b"ACGT"], [b"ACGT"], ["3M"], return_status=True)[3].tolist() == [dc.BAD_ARG]
