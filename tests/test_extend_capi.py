"""mgl_sw_extend_batch_device at the C ABI without a GPU: declared, exported, mirrored; bad arguments are refused before any device work;
without a GPU a well-formed call fails loudly; the ABI version stands."""
import ctypes as C
import os
import re

import pytest

from mgl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mgl_sw_extend_batch_device"


def _call(ctx=None, n=1, seqs=True, index=True, ext=True, max_tl=10, max_ql=10, band=4, zdrop=100, stride=64, flags=0, cigar=True, cigar_len=True):
    L = _lib.lib()
    d = C.c_void_p(0x1000)  # never dereferenced: every case below fails before any device access
    return L.mgl_sw_extend_batch_device(ctx, None, n, d if seqs else None, d if index else None, d, d, d, d, max_tl, max_ql, 200, -150, -260, -11,
                                        band, zdrop, d if ext else None, d if cigar else None, stride, d if cigar_len else None, None, flags)


def test_entry_declared_exported_and_mirrored():
    header = open(os.path.join(ROOT, "include", "mgl_sw.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint %s\s*\(" % NAME, text)
    assert NAME in _lib.SYMBOLS
    assert hasattr(_lib.lib(), NAME)
    assert len(_lib.lib().mgl_sw_extend_batch_device.argtypes) == 23
    assert re.search(r"#define MGL_SW_VERSION 104\b", header)
    assert _lib.ABI_VERSION == 104 and _lib.lib().mgl_sw_version() == 104


def test_extension_record_layout():
    names = ["score", "t_end", "q_end", "score_qend", "t_end_qend", "rows_done", "dropped", "cigar_from"]
    assert C.sizeof(_lib.Extension) == 32 and [f for f, _ in _lib.Extension._fields_] == names
    text = open(os.path.join(ROOT, "include", "mgl_sw.h")).read()
    body = re.search(r"typedef struct mgl_sw_extension \{(.*?)\} mgl_sw_extension;", text, re.S).group(1)
    assert re.sub(r"\s+", " ", body).strip() == "int32_t " + ", ".join(names) + ";"


def test_kernel_id_follows_the_banded_kernel():
    header = open(os.path.join(ROOT, "include", "mgl_sw.h")).read()
    m = re.search(r"#define MGL_SW_KERNEL_BANDED (\d+)[^\n]*\n#define MGL_SW_KERNEL_EXTEND \(MGL_SW_KERNEL_BANDED \+ 1\)\s+/\* 13, sw_extend_kernel\b", header)
    assert m and int(m.group(1)) + 1 == 13 == _lib.KERNEL_EXTEND
    assert _lib.fill_kernel_name(13) == "sw_extend_kernel" and _lib.fill_kernel_name(12) == "sw_banded_kernel"


def test_the_new_flag_is_a_free_bit():
    header = open(os.path.join(ROOT, "include", "mgl_sw.h")).read()
    flags = {k: int(v, 0) for k, v in re.findall(r"#define (MGL_SW_FLAG_\w+) (0x[0-9a-fA-F]+|\d+)\b", header)}
    new = flags.pop("MGL_SW_FLAG_EXTEND_TO_QUERY_END")
    assert new == _lib.FLAG_EXTEND_TO_QUERY_END and new & (new - 1) == 0 and new not in flags.values() and len(flags) >= 5


def test_bad_arguments_before_any_device_work():
    bad = _lib.ERR_BAD_ARG
    assert _call(n=-1) == bad
    assert _call(seqs=False) == bad
    assert _call(index=False) == bad
    assert _call(ext=False) == bad
    assert _call(ext=False, cigar=False, flags=_lib.FLAG_SCORE_ONLY) == bad
    assert _call(band=-1) == bad
    assert _call(max_tl=0) == bad and _call(max_ql=0) == bad
    assert _call(stride=1) == bad                                   # text: "1M" needs 2 bytes
    assert _call(stride=3, flags=_lib.FLAG_BINARY_CIGAR) == bad     # binary: one element is 4
    assert _call(cigar=False) == bad
    assert _call(cigar_len=False) == bad


def test_without_a_gpu_a_well_formed_call_is_a_device_error():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    assert _call() == _lib.ERR_DEVICE
    assert _call(band=0) == _lib.ERR_DEVICE
    assert _call(zdrop=-1) == _lib.ERR_DEVICE
    assert _call(n=0) == _lib.ERR_DEVICE
    assert _call(flags=_lib.FLAG_EXTEND_TO_QUERY_END) == _lib.ERR_DEVICE
    assert _call(stride=0, cigar=False, cigar_len=False, flags=_lib.FLAG_SCORE_ONLY) == _lib.ERR_DEVICE


def test_kernel_sources_hold_no_scalar_memory_store():
    for f in ("sw_extend.hip", "sw_extend.h", "sw_extend.cpp", "sw_band_wave.h", "sw_band_host.h", "sw_ctx_access.h"):
        src = open(os.path.join(ROOT, "mgl_amd", "csrc", f)).read().lower()
        for word in ("s_" + "store", "s_" + "buffer_", "s_" + "scratch_", "s_" + "atomic", "s_" + "dcache"):
            assert word not in src, (f, word)
