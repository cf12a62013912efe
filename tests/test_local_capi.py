"""mgl_sw_local_batch_device_matrix at the C ABI without a GPU: declared, exported, mirrored; bad arguments are refused before any device
work; without a GPU the call fails loudly; mgl_sw_local_hit's layout."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from mgl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mgl_sw_local_batch_device_matrix"


def _call(ctx=None, n=1, matrix=True, code=True, stride=64, flags=0, cigar=True, hit=True):
    L = _lib.lib()
    m = np.zeros((32, 32), np.int8)
    c = np.zeros(256, np.uint8)
    dummy = C.c_void_p(0x1000)  # never dereferenced: every case below fails before any device access
    return L.mgl_sw_local_batch_device_matrix(ctx, None, n, dummy, dummy, dummy, dummy, dummy, dummy, 10, 10,
                                              m.ctypes.data if matrix else None, c.ctypes.data if code else None, 11, 1,
                                              dummy if hit else None, dummy if cigar else None, stride, dummy if cigar else None, None, flags)


def test_entry_declared_exported_and_mirrored():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mgl_sw.h")).read(), flags=re.S)
    assert re.search(r"\bint %s\s*\(" % NAME, text)
    assert "typedef struct mgl_sw_local_hit" in text
    assert NAME in _lib.SYMBOLS
    assert hasattr(_lib.lib(), NAME)
    assert re.search(r"#define MGL_SW_VERSION 104\b", open(os.path.join(ROOT, "include", "mgl_sw.h")).read())
    assert _lib.ABI_VERSION == 104 and _lib.lib().mgl_sw_version() == 104


def test_bad_arguments_before_any_device_work():
    assert _call(n=-1) == _lib.ERR_BAD_ARG
    assert _call(matrix=False) == _lib.ERR_BAD_ARG
    assert _call(code=False) == _lib.ERR_BAD_ARG
    assert _call(stride=1) == _lib.ERR_BAD_ARG                                    # text: "1M" needs 2 bytes
    assert _call(stride=3, flags=_lib.FLAG_BINARY_CIGAR) == _lib.ERR_BAD_ARG      # binary: one element is 4
    assert _call(cigar=False) == _lib.ERR_BAD_ARG
    assert _call(hit=False) == _lib.ERR_BAD_ARG
    # a code >= 32
    L = _lib.lib()
    m = np.zeros((32, 32), np.int8)
    c = np.zeros(256, np.uint8)
    c[65] = 32
    d = C.c_void_p(0x1000)
    assert L.mgl_sw_local_batch_device_matrix(None, None, 1, d, d, d, d, d, d, 10, 10, m.ctypes.data, c.ctypes.data, 11, 1, d, d, 64, d, None, 0) == _lib.ERR_BAD_ARG


def test_score_only_needs_no_cigar_arrays_and_no_gpu_means_device_error():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    assert _call(stride=0, cigar=False, flags=_lib.FLAG_SCORE_ONLY) == _lib.ERR_DEVICE
    assert _call() == _lib.ERR_DEVICE
    assert _call(n=0) == _lib.ERR_DEVICE


def test_local_hit_layout():
    assert C.sizeof(_lib.LocalHit) == 20
    assert [f for f, _ in _lib.LocalHit._fields_] == ["score", "t_begin", "t_end", "q_begin", "q_end"]
    text = open(os.path.join(ROOT, "include", "mgl_sw.h")).read()
    body = re.search(r"typedef struct mgl_sw_local_hit \{(.*?)\} mgl_sw_local_hit;", text, re.S).group(1)
    assert re.sub(r"\s+", " ", body).strip() == "int32_t score, t_begin, t_end, q_begin, q_end;"


def test_kernel_ids_mirrored():
    text = open(os.path.join(ROOT, "include", "mgl_sw.h")).read()
    assert re.search(r"#define MGL_SW_KERNEL_LOCAL_LANE (\d+)\s+/\* sw_local_lane_kernel\b", text)
    ids = {k: int(v) for k, v in re.findall(r"#define (MGL_SW_KERNEL_LOCAL\w*) (\d+)", text)}
    assert _lib.FILL_KERNEL_NAMES[ids["MGL_SW_KERNEL_LOCAL_LANE"]] == "sw_local_lane_kernel"
    assert _lib.FILL_KERNEL_NAMES[ids["MGL_SW_KERNEL_LOCAL"]] == "sw_local_pair_kernel"


def test_new_kernel_sources_hold_no_scalar_memory_store():
    for f in ("sw_local.hip", "sw_local_lane.hip", "sw_local.h", "sw_local.cpp", "sw_ctx_access.h"):
        src = open(os.path.join(ROOT, "mgl_amd", "csrc", f)).read().lower()
        for word in ("s_" + "store", "s_" + "buffer_", "s_" + "scratch_", "s_" + "atomic", "s_" + "dcache"):
            assert word not in src, (f, word)
