"""mgl_sw_align_batch_device_banded at the C ABI without a GPU: declared, exported, mirrored; bad arguments are refused before any device
work; without a GPU a well-formed call fails loudly; the ABI version stands."""
import ctypes as C
import os
import re

import pytest

from mgl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mgl_sw_align_batch_device_banded"
SOFTCLIP = 1


def _call(ctx=None, n=1, seqs=True, index=True, offset=True, max_tl=10, max_ql=10, strategy=SOFTCLIP, band=4, stride=64, flags=0, cigar=True,
          score=True):
    L = _lib.lib()
    d = C.c_void_p(0x1000)  # never dereferenced: every case below fails before any device access
    return L.mgl_sw_align_batch_device_banded(ctx, None, n, d if seqs else None, d if index else None, d, d, d, d, max_tl, max_ql,
                                              200, -150, -260, -11, strategy, band, d if offset else None, d if score else None,
                                              d if cigar else None, stride, d if cigar else None, None, flags)


def test_entry_declared_exported_and_mirrored():
    header = open(os.path.join(ROOT, "include", "mgl_sw.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint %s\s*\(" % NAME, text)
    assert NAME in _lib.SYMBOLS
    assert hasattr(_lib.lib(), NAME)
    assert len(_lib.lib().mgl_sw_align_batch_device_banded.argtypes) == 24
    assert re.search(r"#define MGL_SW_VERSION 104\b", header)
    assert _lib.ABI_VERSION == 104 and _lib.lib().mgl_sw_version() == 104


def test_kernel_id_follows_the_local_kernels():
    header = open(os.path.join(ROOT, "include", "mgl_sw.h")).read()
    m = re.search(r"#define MGL_SW_KERNEL_LOCAL (\d+)[^\n]*\n#define MGL_SW_KERNEL_BANDED (\d+)\s+/\* sw_banded_kernel\b", header)
    assert m and int(m.group(2)) == int(m.group(1)) + 1 == 12
    assert _lib.FILL_KERNEL_NAMES[12] == "sw_banded_kernel" and len(_lib.FILL_KERNEL_NAMES) == 13


def test_bad_arguments_before_any_device_work():
    bad = _lib.ERR_BAD_ARG
    assert _call(n=-1) == bad
    assert _call(seqs=False) == bad
    assert _call(index=False) == bad
    assert _call(offset=False) == bad
    assert _call(band=-1) == bad
    for s in (0, 3, 16, -1):
        assert _call(strategy=s) == bad
    assert _call(max_tl=0) == bad and _call(max_ql=0) == bad
    assert _call(stride=1) == bad                                   # text: "1M" needs 2 bytes
    assert _call(stride=3, flags=_lib.FLAG_BINARY_CIGAR) == bad     # binary: one element is 4
    assert _call(cigar=False) == bad
    assert _call(cigar=False, score=False, flags=_lib.FLAG_SCORE_ONLY) == bad


def test_without_a_gpu_a_well_formed_call_is_a_device_error():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    assert _call() == _lib.ERR_DEVICE
    assert _call(band=0) == _lib.ERR_DEVICE
    assert _call(n=0) == _lib.ERR_DEVICE
    assert _call(stride=0, cigar=False, flags=_lib.FLAG_SCORE_ONLY) == _lib.ERR_DEVICE
    for s in (1, 2, 4, 8):
        assert _call(strategy=s) == _lib.ERR_DEVICE


def test_kernel_sources_hold_no_scalar_memory_store():
    for f in ("sw_banded.hip", "sw_banded.h", "sw_banded.cpp", "sw_band_wave.h", "sw_band_host.h", "sw_ctx_access.h"):
        src = open(os.path.join(ROOT, "mgl_amd", "csrc", f)).read().lower()
        for word in ("s_" + "store", "s_" + "buffer_", "s_" + "scratch_", "s_" + "atomic", "s_" + "dcache"):
            assert word not in src, (f, word)
