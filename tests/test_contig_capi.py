"""The contig entries at the C ABI without a GPU -- mgl_sw_index_build_contigs_device, mgl_sw_index_get_contigs,
mgl_sw_index_contig_of_batch_device, mgl_sw_chain_anchors_grouped_batch_device and mgl_sw_locate_window_contigs_batch_device: declared,
exported, mirrored; every call-level refusal before any device work, on both sides of its edge; without a GPU a well-formed call fails
loudly and the build hands back a null handle; no kernel id and no flag was added, the ABI version stands."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from mgl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mgl_sw.h")).read()
CHAIN_TAIL = ["int64_t total_cand", "int max_cand", "int max_pred", "int max_dist_t", "int max_dist_q", "int bw", "int pen_gap", "int pen_skip",
              "int64_t *d_chain_start_out", "int32_t *d_chain_t_out", "int32_t *d_chain_q_out", "int32_t *d_chain_len_out", "int32_t *d_chain_score_out",
              "int32_t *d_f_out", "int32_t *d_pred_out", "int32_t *d_status_out"]
DECLARED = {
    "mgl_sw_index_build_contigs_device": ["mgl_sw_ctx *ctx", "void *stream", "const uint8_t *d_ref", "int64_t ref_len", "const int64_t *contig_start",
                                          "const int64_t *contig_len", "int64_t n_contigs", "int k", "int w", "mgl_sw_index **out"],
    "mgl_sw_index_get_contigs": ["const mgl_sw_index *idx", "int64_t capacity", "int64_t *start_out", "int64_t *len_out", "int64_t *n_out"],
    "mgl_sw_index_contig_of_batch_device": ["mgl_sw_ctx *ctx", "void *stream", "const mgl_sw_index *idx", "int64_t total", "const int32_t *d_t",
                                            "const int32_t *d_len", "int32_t *d_group_out"],
    "mgl_sw_chain_anchors_grouped_batch_device": [
        "mgl_sw_ctx *ctx", "void *stream", "int64_t n", "const int32_t *d_t_len", "const int32_t *d_q_len", "const int64_t *d_cand_start",
        "const int32_t *d_cand_t", "const int32_t *d_cand_q", "const int32_t *d_cand_len", "const int32_t *d_cand_group"] + CHAIN_TAIL,
    "mgl_sw_locate_window_contigs_batch_device": [
        "mgl_sw_ctx *ctx", "void *stream", "int64_t n", "const mgl_sw_index *idx", "const int32_t *d_q_len", "const int64_t *d_anchor_start",
        "const int32_t *d_anchor_t", "const int32_t *d_anchor_q", "const int32_t *d_anchor_len", "int64_t total_anchors", "int slack", "int max_tl",
        "int64_t *d_t_start_out", "int32_t *d_t_len_out", "int32_t *d_anchor_t_out", "int32_t *d_rid_out", "int32_t *d_status_out"],
}

D = C.c_void_p(0x1000)  # never dereferenced: every case below fails before any device access
BAD, DEV = _lib.ERR_BAD_ARG, _lib.ERR_DEVICE
MAX = 1 << 20


def _p(on):
    return D if on else None


def _table(n, gap=1):
    """n contigs of 3 bases with ``gap`` bytes between two -> (start, len, ref_len)"""
    start = np.arange(n, dtype=np.int64) * (3 + gap)
    return start, np.full(n, 3, np.int64), int(start[-1]) + 3 if n else 0


def _build(start, length, ref_len, n=None, ref=True, k=15, w=10, out=True, arrays=(True, True)):
    handle = C.c_void_p(0x7777)
    start, length = np.ascontiguousarray(start, np.int64), np.ascontiguousarray(length, np.int64)
    ptr = lambda a, on: (a.ctypes.data if a.size else D) if on else None  # noqa: E731
    rc = _lib.lib().mgl_sw_index_build_contigs_device(None, None, _p(ref), ref_len, ptr(start, arrays[0]), ptr(length, arrays[1]),
                                                      len(start) if n is None else n, k, w, C.byref(handle) if out else None)
    return rc, handle.value


def _contig_of(idx=True, total=10, arrays=(True,) * 3):
    return _lib.lib().mgl_sw_index_contig_of_batch_device(None, None, _p(idx), total, *[_p(x) for x in arrays])


def _chain(n=3, lens=(True, True), cands=(True,) * 4, group=True, total=100, max_cand=50, max_pred=64, dist=(5000, 5000), bw=500, pen=(38, 0), outs=(True,) * 5,
           optional=(True,) * 3):
    return _lib.lib().mgl_sw_chain_anchors_grouped_batch_device(None, None, n, *[_p(x) for x in lens], *[_p(x) for x in cands], _p(group), total, max_cand, max_pred,
                                                                *dist, bw, *pen, *[_p(x) for x in outs], *[_p(x) for x in optional])


def _locate(n=3, idx=True, ins=(True,) * 5, total=100, slack=200, max_tl=5000, outs=(True,) * 4, status=True):
    return _lib.lib().mgl_sw_locate_window_contigs_batch_device(None, None, n, _p(idx), *[_p(x) for x in ins], total, slack, max_tl, *[_p(x) for x in outs],
                                                                _p(status))


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    decl = re.search(r"\b(?:int|void) %s\s*\((.*?)\);" % name, text, re.S).group(1)
    return [re.sub(r"\s+", " ", a).strip() for a in decl.split(",")]


def test_entries_declared_exported_and_mirrored():
    for name, args in DECLARED.items():
        assert _declared(name) == args, name
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
        assert len(getattr(_lib.lib(), name).argtypes) == len(args)
    # the grouped entry is the chain entry with ONE more argument, behind the candidates
    plain = _declared("mgl_sw_chain_anchors_batch_device")
    grouped = DECLARED["mgl_sw_chain_anchors_grouped_batch_device"]
    assert grouped[:9] + grouped[10:] == plain and grouped[9] == "const int32_t *d_cand_group"
    # the window entry is the plain one with the index for ref_len and d_rid_out in front of the status
    window = _declared("mgl_sw_locate_window_batch_device")
    mine = DECLARED["mgl_sw_locate_window_contigs_batch_device"]
    assert mine[:3] + ["int64_t ref_len"] + mine[4:15] + mine[16:] == window
    info = re.search(r"typedef struct mgl_sw_index_info \{(.*?)\} mgl_sw_index_info;", HEADER, re.S).group(1)
    assert re.sub(r"\s+", " ", info).strip() == "int64_t ref_len, entries, bytes; int32_t k, w;" and C.sizeof(_lib.IndexInfo) == 32
    assert HEADER.count("tests/contig_textbook.py") >= 3 and "ONE reference sequence (contigs concatenated by the caller" not in HEADER
    assert "straddles a gap" in HEADER


def test_version_kernel_ids_and_flags_stand():
    assert re.search(r"#define MGL_SW_VERSION 104\b", HEADER)
    assert _lib.ABI_VERSION == 104 and _lib.lib().mgl_sw_version() == 104
    assert len(re.findall(r"^#define MGL_SW_KERNEL_\w+ \d+\b", HEADER, re.M)) == 13 == len(_lib.FILL_KERNEL_NAMES)
    assert len(re.findall(r"^#define MGL_SW_KERNEL_\w+ ", HEADER, re.M)) == 15
    flags = {k: int(v, 0) for k, v in re.findall(r"#define (MGL_SW_FLAG_\w+) (0x[0-9a-fA-F]+|\d+)\b", HEADER)}
    assert len(flags) == 7 and max(flags.values()) == 0x40 == _lib.FLAG_EXTEND_ADAPTIVE_BAND
    assert not any("flags" in a for args in DECLARED.values() for a in args)


def test_python_methods_and_their_defaults():
    from mgl_amd import formats, smithwaterman as sw, synth

    M = sw.MicrosoftSmithWaterman
    for f in ("build_index_contigs", "build_index_contigs_device", "locate_window_contigs_device"):
        assert hasattr(M, f), f
    sig = lambda f: {k: v.default for k, v in inspect.signature(f).parameters.items() if v.default is not inspect.Parameter.empty}  # noqa: E731
    assert sig(M.build_index_contigs) == dict(k=15, w=10, gap=1) and sig(M.build_index_contigs_device) == dict(names=None, k=15, w=10)
    assert sig(M.chain_anchors_device)["group"] is None and sig(M.chain_anchors)["groups"] is None
    assert list(inspect.signature(M.chain_anchors_device).parameters)[-1] == "group"  # behind the existing ones: positional callers stand
    assert all(hasattr(sw.Index, f) for f in ("contig_of_device", "get_contigs", "info", "export", "close"))
    assert sig(sw.Index.__init__) == dict(contigs=None, owner=None)
    assert sw.MapResult._fields == ("ref_beg", "ref_end", "strand", "score", "cigars", "status")
    for plain, contig in ((sw.MapResult, sw.ContigMapResult), (sw.RankedMapResult, sw.ContigRankedMapResult), (sw.DescribedMapResult, sw.ContigDescribedMapResult)):
        assert contig._fields == plain._fields + ("rid", "rname")
    assert sw.ContigTable._fields == ("names", "starts", "lens")
    assert list(inspect.signature(formats.write_sam).parameters)[:3] == ["path", "ref_name", "ref_len"]
    # the synthetic set: mapping_set's reference, cut inside its spacers
    ref, reads, truth = synth.mapping_set(11, 8, length=2000, spacer=3000)
    contigs, creads, ctruth = synth.contig_mapping_set(11, 8, length=2000, spacer=3000, contigs=4)
    assert creads == reads and [n for n, _ in contigs] == ["contig%d" % c for c in range(4)] and len(ctruth) == 8
    laid = b"N".join(s for _, s in contigs)
    cuts = [i for i, b in enumerate(laid) if b == ord("N")]
    assert len(laid) == len(ref) and len(cuts) == 3 and all(laid[i] == ref[i] for i in range(len(ref)) if i not in cuts)
    starts = [0] + [c + 1 for c in cuts]
    for (rid, pos, n, strand), (at, m, s) in zip(ctruth, truth):
        assert (starts[rid] + pos, n, strand) == (at, m, s) and contigs[rid][1][pos:pos + n] == ref[at:at + m]
    assert all(not any(at <= c < at + m for at, m, _ in truth) for c in cuts) and {t[0] for t in ctruth} == {0, 1, 2, 3}
    one = synth.contig_mapping_set(11, 8, length=2000, spacer=3000, contigs=1)
    assert one[0] == [("contig0", ref)] and one[2] == [(0, at, m, s) for at, m, s in truth]
    many = synth.contig_mapping_set(5, 3, length=600, spacer=100, contigs=40)  # more cuts than spacers between reads
    assert len(many[0]) == 40 and all(len(s) >= 1 for _, s in many[0]) and len(b"N".join(s for _, s in many[0])) == len(synth.mapping_set(5, 3, 600, 100)[0])


def test_build_contigs_refusals_on_both_sides_of_their_edges():
    s, n, ref_len = _table(5)
    ok = DEV if _lib.lib().mgl_sw_device_count() <= 0 else None
    # n_contigs 0, 1, 2^20, 2^20 + 1
    assert _build(s[:0], n[:0], 10) == (BAD, None) and _build(s, n, ref_len, n=0) == (BAD, None) and _build(s, n, ref_len, n=-1) == (BAD, None)
    big_s, big_n, big_len = _table(MAX + 1)
    assert _build(big_s, big_n, big_len) == (BAD, None)
    if ok is not None:
        assert _build(s[:1], n[:1], 3) == (ok, None) and _build(big_s[:MAX], big_n[:MAX], int(big_s[MAX - 1]) + 3) == (ok, None)
        assert _build(s, n, ref_len) == (ok, None) and _build(*_table(5, gap=7)) == (ok, None)
    # start[0] = 1
    assert _build(s + 1, n, ref_len + 1) == (BAD, None)
    # a gap of 0, of 1
    tight = s.copy()
    tight[3:] -= 1
    assert _build(tight, n, ref_len - 1) == (BAD, None)
    # the last end off by one, either way
    assert _build(s, n, ref_len + 1) == (BAD, None) and _build(s, n, ref_len - 1) == (BAD, None)
    # len = 0, and a negative one
    for bad_len in (0, -1):
        z = n.copy()
        z[2] = bad_len
        assert _build(s, z, ref_len) == (BAD, None)
    z = n.copy()
    z[4] = 0
    assert _build(s, z, ref_len - 3) == (BAD, None)
    # starts that descend; a contig beyond the buffer
    assert _build(s[::-1].copy(), n, ref_len) == (BAD, None) and _build(s, n * 1000, ref_len) == (BAD, None)
    # the plain build's arguments
    for kw in (dict(ref=False), dict(k=3), dict(k=17), dict(w=0), dict(w=33), dict(arrays=(False, True)), dict(arrays=(True, False))):
        assert _build(s, n, ref_len, **kw) == (BAD, None), kw
    assert _build(s, n, 0) == (BAD, None) and _build(s, n, 1 << 31) == (BAD, None) and _build(s, n, ref_len, out=False)[0] == BAD
    # get_contigs
    cnt = C.c_int64(-5)
    assert _lib.lib().mgl_sw_index_get_contigs(None, 0, None, None, C.byref(cnt)) == BAD and _lib.lib().mgl_sw_index_get_contigs(D, 0, None, None, None) == BAD


def test_stage_refusals_before_any_device_work():
    assert _contig_of(idx=False) == BAD and _contig_of(total=-1) == BAD and _contig_of(total=(1 << 30) + 1) == BAD
    for i in range(3):
        assert _contig_of(arrays=tuple(x != i for x in range(3))) == BAD
    # the grouped chain entry: the plain entry's refusals, and a null group array
    assert _chain(group=False) == BAD
    for i in range(2):
        assert _chain(lens=tuple(x != i for x in range(2))) == BAD
    for i in range(4):
        assert _chain(cands=tuple(x != i for x in range(4))) == BAD
    for i in range(5):
        assert _chain(outs=tuple(x != i for x in range(5))) == BAD
    assert _chain(n=-1) == BAD and _chain(n=(1 << 30) + 1) == BAD and _chain(total=-1) == BAD and _chain(total=(1 << 30) + 1) == BAD
    assert _chain(max_cand=-1) == BAD and _chain(max_pred=0) == BAD and _chain(max_pred=65) == BAD
    assert _chain(dist=(-1, 5)) == BAD and _chain(dist=(5, -1)) == BAD and _chain(bw=-1) == BAD and _chain(pen=(-1, 0)) == BAD and _chain(pen=(0, -1)) == BAD
    assert _chain(dist=(1 << 30, 1 << 30), bw=1 << 30, pen=(2, 0)) == BAD  # the int32 guard of pen
    # the window entry
    assert _locate(idx=False) == BAD
    for i in range(5):
        assert _locate(ins=tuple(x != i for x in range(5))) == BAD
    for i in range(4):
        assert _locate(outs=tuple(x != i for x in range(4))) == BAD
    assert _locate(n=-1) == BAD and _locate(n=(1 << 30) + 1) == BAD and _locate(total=-1) == BAD and _locate(total=(1 << 30) + 1) == BAD
    assert _locate(slack=-1) == BAD and _locate(max_tl=0) == BAD


def test_without_a_gpu_a_well_formed_call_is_a_device_error():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    assert _contig_of() == DEV and _contig_of(total=0) == DEV and _contig_of(total=1 << 30) == DEV
    assert _chain() == DEV and _chain(n=0) == DEV and _chain(n=1 << 30) == DEV and _chain(total=0) == DEV and _chain(total=1 << 30) == DEV
    assert _chain(max_cand=0) == DEV and _chain(max_pred=1) == DEV and _chain(optional=(False,) * 3) == DEV
    assert _chain(dist=(1 << 30, 1 << 30), bw=1 << 30, pen=(1, 0)) == DEV
    assert _locate() == DEV and _locate(n=0) == DEV and _locate(n=1 << 30) == DEV and _locate(total=0) == DEV and _locate(total=1 << 30) == DEV
    assert _locate(slack=0) == DEV and _locate(max_tl=1) == DEV and _locate(status=False) == DEV
    s, n, ref_len = _table(5)
    assert _build(s, n, ref_len) == (DEV, None) and _build(s[:1], n[:1], 3) == (DEV, None)
    big_s, big_n, _ = _table(MAX)
    assert _build(big_s, big_n, int(big_s[-1]) + 3) == (DEV, None)
