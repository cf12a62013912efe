"""The index family at the C ABI without a GPU -- mgl_sw_index_build_device, _destroy, _get_info, _export_device,
mgl_sw_seed_index_batch_device and mgl_sw_locate_window_batch_device: declared, exported, mirrored; every call-level bad argument is
refused before any device work, on both sides of its edge; without a GPU a well-formed call fails loudly and the build hands back a
null handle; no kernel id and no flag was added, the ABI version stands."""
import ctypes as C
import os
import re

import pytest

from mgl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mgl_sw.h")).read()
DECLARED = {
    "mgl_sw_index_build_device": ["mgl_sw_ctx *ctx", "void *stream", "const uint8_t *d_ref", "int64_t ref_len", "int k", "int w", "mgl_sw_index **out"],
    "mgl_sw_index_destroy": ["mgl_sw_index *idx"],
    "mgl_sw_index_get_info": ["const mgl_sw_index *idx", "mgl_sw_index_info *out"],
    "mgl_sw_index_export_device": ["const mgl_sw_index *idx", "void *stream", "uint32_t *d_keys_out", "int32_t *d_pos_out", "int64_t capacity"],
    "mgl_sw_seed_index_batch_device": [
        "mgl_sw_ctx *ctx", "void *stream", "const mgl_sw_index *idx", "int64_t n", "const uint8_t *d_queries", "const int64_t *d_q_start",
        "const int32_t *d_q_len", "int strands", "int max_occ", "int max_occ_ref", "int merge", "int max_cand", "int64_t cand_capacity",
        "int64_t *d_cand_start_out", "int32_t *d_cand_t_out", "int32_t *d_cand_q_out", "int32_t *d_cand_len_out", "int32_t *d_row_t_len_out",
        "int32_t *d_row_q_len_out", "int32_t *d_status_out"],
    "mgl_sw_locate_window_batch_device": [
        "mgl_sw_ctx *ctx", "void *stream", "int64_t n", "int64_t ref_len", "const int32_t *d_q_len", "const int64_t *d_anchor_start",
        "const int32_t *d_anchor_t", "const int32_t *d_anchor_q", "const int32_t *d_anchor_len", "int64_t total_anchors", "int slack", "int max_tl",
        "int64_t *d_t_start_out", "int32_t *d_t_len_out", "int32_t *d_anchor_t_out", "int32_t *d_status_out"],
}

D = C.c_void_p(0x1000)  # never dereferenced: every case below fails before any device access


def _p(on):
    return D if on else None


def _build(ref=True, ref_len=1000, k=15, w=10, out=True):
    handle = C.c_void_p(0x7777)
    rc = _lib.lib().mgl_sw_index_build_device(None, None, _p(ref), ref_len, k, w, C.byref(handle) if out else None)
    return rc, handle.value


def _seed(idx=True, n=3, reads=(True,) * 3, strands=2, max_occ=8, max_occ_ref=64, merge=1, max_cand=4096, capacity=100, cands=(True,) * 4, rows=(True, True),
          status=True):
    return _lib.lib().mgl_sw_seed_index_batch_device(None, None, _p(idx), n, *[_p(x) for x in reads], strands, max_occ, max_occ_ref, merge, max_cand, capacity,
                                                     *[_p(x) for x in cands], *[_p(x) for x in rows], _p(status))


def _locate(n=3, ref_len=1000, ins=(True,) * 5, total=100, slack=200, max_tl=5000, outs=(True,) * 3, status=True):
    return _lib.lib().mgl_sw_locate_window_batch_device(None, None, n, ref_len, *[_p(x) for x in ins], total, slack, max_tl, *[_p(x) for x in outs], _p(status))


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    decl = re.search(r"\b(?:int|void) %s\s*\((.*?)\);" % name, text, re.S).group(1)
    return [re.sub(r"\s+", " ", a).strip() for a in decl.split(",")]


def test_entries_declared_exported_and_mirrored():
    for name, args in DECLARED.items():
        assert _declared(name) == args, name
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
        assert len(getattr(_lib.lib(), name).argtypes) == len(args)
    # the outputs of the seed stage are mgl_sw_seed_strands_batch_device's, by name, type and order
    strands = re.search(r"\bint mgl_sw_seed_strands_batch_device\s*\((.*?)\);", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S), re.S).group(1)
    assert DECLARED["mgl_sw_seed_index_batch_device"][-8:] == [re.sub(r"\s+", " ", a).strip() for a in strands.split(",")][-8:]
    assert re.search(r"typedef struct mgl_sw_index mgl_sw_index;", HEADER)
    info = re.search(r"typedef struct mgl_sw_index_info \{(.*?)\} mgl_sw_index_info;", HEADER, re.S).group(1)
    assert re.sub(r"\s+", " ", info).strip() == "int64_t ref_len, entries, bytes; int32_t k, w;"
    assert C.sizeof(_lib.IndexInfo) == 32 and [f for f, _ in _lib.IndexInfo._fields_] == ["ref_len", "entries", "bytes", "k", "w"]
    assert HEADER.count("tests/index_textbook.py") >= 3


def test_python_methods_and_the_mapping_set():
    from mgl_amd import smithwaterman as sw, synth

    for f in ("build_index", "seed_index", "seed_index_device", "locate_window_device", "map_reads_device", "map_reads"):
        assert hasattr(sw.MicrosoftSmithWaterman, f), f
    assert all(hasattr(sw.Index, f) for f in ("info", "export", "close"))
    assert sw.MapResult._fields == ("ref_beg", "ref_end", "strand", "score", "cigars", "status")
    ref, reads, truth = synth.mapping_set(5, 4, length=600, spacer=100)
    pairs = synth.chain_pairs(5, 4, 600)
    assert len(reads) == len(truth) == 4 and len(ref) == 5 * 100 + sum(len(p[0]) for p in pairs)
    at = 0
    for p, ((pos, n, strand), (T, Q, _)) in enumerate(zip(truth, pairs)):
        assert pos == at + 100 and n == len(T) and ref[pos:pos + n] == T and strand == p % 2
        assert reads[p] == (synth.revcomp(Q) if strand else Q)
        at = pos + n
    assert synth.mapping_set(5, 4, length=600, spacer=100) == (ref, reads, truth) and set(ref) <= set(b"ACGT")
    assert synth.mapping_set(5, 2, length=600, spacer=0)[0] == pairs[0][0] + synth.chain_pairs(5, 2, 600)[1][0]


def test_version_kernel_ids_and_flags_stand():
    assert re.search(r"#define MGL_SW_VERSION 104\b", HEADER)
    assert _lib.ABI_VERSION == 104 and _lib.lib().mgl_sw_version() == 104
    assert len(re.findall(r"^#define MGL_SW_KERNEL_\w+ \d+\b", HEADER, re.M)) == 13 == len(_lib.FILL_KERNEL_NAMES)
    assert len(re.findall(r"^#define MGL_SW_KERNEL_\w+ ", HEADER, re.M)) == 15
    flags = {k: int(v, 0) for k, v in re.findall(r"#define (MGL_SW_FLAG_\w+) (0x[0-9a-fA-F]+|\d+)\b", HEADER)}
    assert len(flags) == 7 and max(flags.values()) == 0x40 == _lib.FLAG_EXTEND_ADAPTIVE_BAND


def test_index_build_bad_arguments_hand_back_a_null_handle():
    bad = _lib.ERR_BAD_ARG
    for kw in (dict(ref=False), dict(ref_len=0), dict(ref_len=-1), dict(ref_len=1 << 31), dict(k=3), dict(k=17), dict(w=0), dict(w=33)):
        assert _build(**kw) == (bad, None), kw
    assert _build(out=False)[0] == bad
    L = _lib.lib()
    L.mgl_sw_index_destroy(None)  # harmless
    info = _lib.IndexInfo()
    assert L.mgl_sw_index_get_info(None, C.byref(info)) == bad
    assert L.mgl_sw_index_export_device(None, None, D, D, 10) == bad


def test_seed_index_bad_arguments_before_any_device_work():
    bad = _lib.ERR_BAD_ARG
    assert _seed(idx=False) == bad
    for i in range(3):
        assert _seed(reads=tuple(x != i for x in range(3))) == bad
    for i in range(4):
        assert _seed(cands=tuple(x != i for x in range(4))) == bad
    assert _seed(strands=0) == bad and _seed(strands=3) == bad and _seed(strands=-1) == bad
    assert _seed(n=-1) == bad and _seed(n=(1 << 29) + 1) == bad and _seed(strands=1, n=(1 << 30) + 1) == bad
    assert _seed(max_occ=0) == bad and _seed(max_occ=65) == bad
    assert _seed(max_occ_ref=0) == bad and _seed(max_occ_ref=8193) == bad
    assert _seed(merge=-1) == bad and _seed(merge=2) == bad
    assert _seed(max_cand=0) == bad and _seed(max_cand=8193) == bad
    assert _seed(capacity=-1) == bad and _seed(capacity=(1 << 30) + 1) == bad


def test_locate_window_bad_arguments_before_any_device_work():
    bad = _lib.ERR_BAD_ARG
    for i in range(5):
        assert _locate(ins=tuple(x != i for x in range(5))) == bad
    for i in range(3):
        assert _locate(outs=tuple(x != i for x in range(3))) == bad
    assert _locate(n=-1) == bad and _locate(n=(1 << 30) + 1) == bad
    assert _locate(ref_len=0) == bad and _locate(ref_len=1 << 31) == bad
    assert _locate(total=-1) == bad and _locate(total=(1 << 30) + 1) == bad
    assert _locate(slack=-1) == bad and _locate(max_tl=0) == bad


def test_without_a_gpu_a_well_formed_call_is_a_device_error():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    dev = _lib.ERR_DEVICE
    for kw in (dict(), dict(ref_len=1), dict(ref_len=(1 << 31) - 1), dict(k=4), dict(k=16), dict(w=1), dict(w=32)):
        assert _build(**kw) == (dev, None), kw
    assert _seed() == dev
    assert _seed(n=0) == dev and _seed(n=1 << 29) == dev and _seed(strands=1, n=1 << 30) == dev
    assert _seed(max_occ=1) == dev and _seed(max_occ=64) == dev
    assert _seed(max_occ_ref=1) == dev and _seed(max_occ_ref=8192) == dev
    assert _seed(merge=0) == dev and _seed(max_cand=1) == dev and _seed(max_cand=8192) == dev
    assert _seed(capacity=0) == dev and _seed(capacity=1 << 30) == dev
    assert _seed(status=False) == dev and _seed(rows=(False, True)) == dev and _seed(rows=(True, False)) == dev and _seed(rows=(False, False), status=False) == dev
    assert _locate() == dev
    assert _locate(n=0) == dev and _locate(n=1 << 30) == dev
    assert _locate(ref_len=1) == dev and _locate(ref_len=(1 << 31) - 1) == dev
    assert _locate(total=0) == dev and _locate(total=1 << 30) == dev
    assert _locate(slack=0) == dev and _locate(max_tl=1) == dev and _locate(status=False) == dev
