"""The one-wave pair kernel (small_pair() of sw_small_pair.h, behind sw_small_kernel and the mailbox waves of sw_service_kernel) on the
batches of tests/small_cases.py, whose lengths, paths, ties and bytes lie on the kernel's own seams -- the rows a lane owns, the
masked, unmasked and clamped blocks of the fill, the rounds of 64 of the walk, the two passes that pick the last column's and the
last row's cell, the base codes, the 16-bit span, the largest geometry LDS holds, the CIGAR slot's width -- bit for bit against the
oracle: offset, CIGAR text, all six score fields, status and cigar_len.  The kernel is forced (set_small_kernel(2)) and asserted
from the timing record after every batch; tests/test_small_cases.py checks on the CPU that the cases mean what they say."""
import functools
import os

import numpy as np
import pytest
import torch

import oracle_lib as ol
import small_cases as sc
from mgl_amd import device_batch, smithwaterman as sw

pytestmark = pytest.mark.gpu

SMALL = 8


@functools.lru_cache(maxsize=None)
def oracle(name, k, strategy):
    """the oracle's (offsets, scores, cigars) of batch k of a set: computed once, shared by the tests below"""
    c = sc.cases(name)[k]
    return ol.oracle_align_batch(list(c.targets), list(c.queries), c.params, strategy, nthreads=16)


@pytest.fixture(scope="module")
def forced():
    a = sw.MicrosoftSmithWaterman(0)
    a.set_small_kernel(2)
    yield a
    a.close()


def _on_kernel(c):
    return sc.built()[1]["on_kernel"].get(c.name, True)


def _compare(c, strategy, want, offsets, scores, cigars, cigar_len, how):
    off, score, cg = want
    for n in range(len(cg)):
        got = (int(offsets[n]), cigars[n], tuple(int(x) for x in scores[n]), int(cigar_len[n]))
        assert got == (int(off[n]), cg[n], tuple(int(x) for x in score[n]), len(cg[n])), (how, c.name, strategy, n, c.intent[n], len(c.targets[n]), len(c.queries[n]))


@pytest.mark.parametrize("name", ["rows", "ramps", "runs", "round_ties", "last_cell_ties", "bytes", "span", "fits"])
def test_set(forced, name):
    """every batch of the set under every strategy it names, through the host entry (which raises on any status but 0)"""
    cs = sc.cases(name)
    assert cs
    for k, c in enumerate(cs):
        for strategy in c.strategies:
            res = forced.align_batch(list(c.targets), list(c.queries), c.params, strategy, cigar_stride=c.cigar_stride)
            assert (forced.timing().fill_kernel == SMALL) == _on_kernel(c), (c.name, strategy, forced.timing().fill_kernel)
            _compare(c, strategy, oracle(name, k, strategy), res.offsets, res.scores, res.cigars, res.cigar_len, "host")
    if name in ("fits", "span"):      # one past an edge the planner routes elsewhere -- and still agrees
        assert {_on_kernel(c) for c in cs} == {True, False}


def _ascii_batch(c, cigar_stride, guard=0xAA):
    """the batch on the device, its CIGAR slots inside a larger buffer filled with `guard`: a slot's width on either side"""
    td, toff = sw.concat(list(c.targets))
    qd, qoff = sw.concat(list(c.queries))
    b = device_batch.from_host(td, toff, qd, qoff, "cuda:0", cigar_stride=cigar_stride)
    whole = torch.full(((b.n + 2) * cigar_stride,), guard, dtype=torch.uint8, device="cuda:0")
    b.cigars = whole[cigar_stride:(b.n + 1) * cigar_stride].view(b.n, cigar_stride)
    return b, whole


def test_slots(forced):
    """CIGAR slots one byte short, exact, one and three bytes long, and 7, 9 and 513 bytes wide (no multiple of four: the byte-wise
    copy-out) through the device entry: the status of every pair, cigar_len the length needed whether it fits or not, zeros behind
    the text (a slot that overflowed is all zeros), the bytes in front of the first slot and behind the last one untouched"""
    cs = sc.cases("slots")
    seen = set()
    for k, c in enumerate(cs):
        off, score, cg = oracle("slots", k, sc.SOFTCLIP)
        stride = c.cigar_stride
        b, whole = _ascii_batch(c, stride)
        b.run(forced, c.params, sc.SOFTCLIP)
        torch.cuda.synchronize()
        assert forced.timing().fill_kernel == SMALL, c.name
        raw, ln, st = b.cigars.cpu().numpy(), b.cigar_len.cpu().numpy(), b.status.cpu().numpy()
        edge = whole.cpu().numpy()
        assert (edge[:stride] == 0xAA).all() and (edge[-stride:] == 0xAA).all(), c.name
        for n in range(b.n):
            fits = len(cg[n]) <= stride
            text = cg[n].encode() if fits else b""
            assert int(st[n]) == (0 if fits else sc.ERR_CIGAR_OVERFLOW) and int(ln[n]) == len(cg[n]), (c.name, n, int(st[n]), int(ln[n]), cg[n])
            assert raw[n].tobytes() == text + bytes(stride - len(text)), (c.name, n, cg[n], raw[n].tobytes())
            assert tuple(int(x) for x in b.scores[n].cpu()) == tuple(int(x) for x in score[n]) and int(b.offsets[n]) == int(off[n]), (c.name, n)
            seen.add((stride - len(cg[n]), fits))
    assert {(-1, False), (0, True), (1, True), (3, True)} <= seen


def _device_subset():
    """the four full-wave ends, bytes, span: (set, batch index, case)"""
    out = [("ramps", k, c) for k, c in enumerate(sc.cases("ramps")) if int(c.name.rsplit("tl", 1)[1].split("/")[0]) in (128, 256, 384, 512)]
    out += [(name, k, c) for name in ("bytes", "span") for k, c in enumerate(sc.cases(name)) if _on_kernel(c)]
    return out


def test_device_entries(forced):
    """the same batches through the ASCII device entry and -- where every byte is one of ACGT -- as 2-bit packed bases
    (device_batch.PackedBatch): the same kernel, the same results"""
    packed = 0
    for name, k, c in _device_subset():
        acgt = all(set(s) <= set(b"ACGT") for s in c.targets + c.queries)
        td, toff = sw.concat(list(c.targets))
        qd, qoff = sw.concat(list(c.queries))
        dev = torch.device("cuda", 0)
        i32 = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.int32)).to(dev)  # noqa: E731
        batches = [("ascii", device_batch.from_host(td, toff, qd, qoff, "cuda:0", cigar_stride=c.cigar_stride))]
        if acgt:
            batches.append(("2bit", device_batch.PackedBatch(torch.from_numpy(device_batch.pack2bit(td)).to(dev), torch.from_numpy(toff[:-1].copy()).to(dev),
                                                             i32(np.diff(toff)), torch.from_numpy(device_batch.pack2bit(qd)).to(dev),
                                                             torch.from_numpy(qoff[:-1].copy()).to(dev), i32(np.diff(qoff)),
                                                             len(c.targets[0]), len(c.queries[0]), cigar_stride=c.cigar_stride)))
            packed += 1
        for strategy in c.strategies:
            for how, b in batches:
                b.run(forced, c.params, strategy)
                torch.cuda.synchronize()
                assert forced.timing().fill_kernel == SMALL, (how, c.name, strategy)
                assert not b.status.cpu().numpy().any(), (how, c.name, strategy)
                _compare(c, strategy, oracle(name, k, strategy), b.offsets.cpu().numpy(), b.scores.cpu().numpy(), b.cigar_strings(), b.cigar_len.cpu().numpy(), how)
    assert packed >= 8


def _restore_front_ends():
    """back to what the library starts with (sw_service.cpp: ServicePool(), sw_batcher.cpp: EnvInit)"""
    sw.set_service(int(os.environ.get("MGL_SW_SERVICE_SLOTS", 64)))
    us, batch = int(os.environ.get("MGL_SW_COALESCE_US", 50)), int(os.environ.get("MGL_SW_COALESCE_BATCH", 4096))
    if us >= 0 and batch > 0:
        sw.set_coalescing(batch, us)


@pytest.mark.parametrize("service", [64, 0], ids=["mailboxes", "coalescer"])
def test_one_pair_entry(service):
    """mgl_sw_align on a subset of every set: through the mailbox waves (small_pair<false>; the last pair needs more than 64 KiB of
    LDS and makes the service launch its larger grid), then with the service off, through the coalescer"""
    sub = sc.service_subset()
    sw.set_service(service)
    sw.set_coalescing(256, 200)
    before = sw.service_stats()[0]
    try:
        for t, q, params, strategy, where in sub:
            o = ol.oracle_align(t, q, params, strategy)
            cigar, off, ez = sw.align(t, q, params, strategy)
            assert (off, cigar, tuple(ez)) == (o["offset"], o["cigar"], tuple(o["score"])), (where, params, strategy, len(t), len(q))
        served = sw.service_stats()[0] - before
        print("test_one_pair_entry", service, "pairs", len(sub), "served through mailboxes", served)
        assert (served >= len(sub) // 2) if service else served == 0
    finally:
        _restore_front_ends()
