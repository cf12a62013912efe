"""mgl_sw_chain_anchors_batch_device at the C ABI without a GPU: declared, exported, mirrored; bad arguments are refused before any device
work; without a GPU a well-formed call fails loudly; no kernel id and no flag was added, the ABI version stands."""
import ctypes as C
import os
import re

import pytest

from mgl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mgl_sw_chain_anchors_batch_device"
HEADER = open(os.path.join(ROOT, "include", "mgl_sw.h")).read()
ARGS = ["mgl_sw_ctx *ctx", "void *stream", "int64_t n", "const int32_t *d_t_len", "const int32_t *d_q_len", "const int64_t *d_cand_start",
        "const int32_t *d_cand_t", "const int32_t *d_cand_q", "const int32_t *d_cand_len", "int64_t total_cand", "int max_cand", "int max_pred",
        "int max_dist_t", "int max_dist_q", "int bw", "int pen_gap", "int pen_skip", "int64_t *d_chain_start_out", "int32_t *d_chain_t_out",
        "int32_t *d_chain_q_out", "int32_t *d_chain_len_out", "int32_t *d_chain_score_out", "int32_t *d_f_out", "int32_t *d_pred_out", "int32_t *d_status_out"]


def _call(ctx=None, n=3, lens=(True, True), cands=(True, True, True, True), total=10, max_cand=8, max_pred=64, dist=(100, 100), bw=50, pen=(38, 0),
          chain=(True, True, True, True, True), dp=(True, True), status=True):
    L = _lib.lib()
    d = C.c_void_p(0x1000)  # never dereferenced: every case below fails before any device access
    p = lambda on: d if on else None  # noqa: E731
    return L.mgl_sw_chain_anchors_batch_device(ctx, None, n, p(lens[0]), p(lens[1]), *[p(x) for x in cands], total, max_cand, max_pred, dist[0], dist[1], bw,
                                               pen[0], pen[1], *[p(x) for x in chain], p(dp[0]), p(dp[1]), p(status))


def test_entry_declared_exported_and_mirrored():
    text = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    decl = re.search(r"\bint %s\s*\((.*?)\);" % NAME, text, re.S).group(1)
    assert [re.sub(r"\s+", " ", a).strip() for a in decl.split(",")] == ARGS and len(ARGS) == 25
    assert NAME in _lib.SYMBOLS and hasattr(_lib.lib(), NAME)
    assert len(_lib.lib().mgl_sw_chain_anchors_batch_device.argtypes) == 25
    assert "tests/chain_dp_textbook.py" in HEADER


def test_version_kernel_ids_and_flags_stand():
    assert re.search(r"#define MGL_SW_VERSION 104\b", HEADER)
    assert _lib.ABI_VERSION == 104 and _lib.lib().mgl_sw_version() == 104
    assert len(re.findall(r"^#define MGL_SW_KERNEL_\w+ \d+\b", HEADER, re.M)) == 13 == len(_lib.FILL_KERNEL_NAMES)
    assert len(re.findall(r"^#define MGL_SW_KERNEL_\w+ ", HEADER, re.M)) == 15
    flags = {k: int(v, 0) for k, v in re.findall(r"#define (MGL_SW_FLAG_\w+) (0x[0-9a-fA-F]+|\d+)\b", HEADER)}
    assert max(flags.values()) == 0x40 == _lib.FLAG_EXTEND_ADAPTIVE_BAND


def test_bad_arguments_before_any_device_work():
    bad = _lib.ERR_BAD_ARG
    for k in range(2):
        assert _call(lens=tuple(x != k for x in range(2))) == bad
    for k in range(4):
        assert _call(cands=tuple(x != k for x in range(4))) == bad
    for k in range(5):
        assert _call(chain=tuple(x != k for x in range(5))) == bad
    assert _call(n=-1) == bad and _call(n=(1 << 30) + 1) == bad
    assert _call(total=-1) == bad and _call(total=(1 << 30) + 1) == bad
    assert _call(max_pred=0) == bad and _call(max_pred=65) == bad and _call(max_pred=-1) == bad
    assert _call(dist=(-1, 100)) == bad and _call(dist=(100, -1)) == bad
    assert _call(bw=-1) == bad
    assert _call(pen=(-1, 0)) == bad and _call(pen=(0, -1)) == bad
    assert _call(max_cand=-1) == bad
    # the int32 guard of pen: pen_gap * bw + pen_skip * min(max_dist_t, max_dist_q) >= 2^31
    assert _call(bw=1, pen=((1 << 31) - 1, 1), dist=(1, 7)) == bad          # 2^31 - 1 + 1
    assert _call(bw=1 << 16, pen=(1 << 15, 0)) == bad                       # 2^31
    assert _call(bw=0, pen=(0, 2147484), dist=(2000, 1000)) == bad          # 2147484000
    assert _call(bw=(1 << 31) - 1, pen=((1 << 31) - 1, (1 << 31) - 1), dist=((1 << 31) - 1, (1 << 31) - 1)) == bad  # (no wrap in the guard itself)


def test_without_a_gpu_a_well_formed_call_is_a_device_error():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    dev = _lib.ERR_DEVICE
    assert _call() == dev
    assert _call(n=0) == dev and _call(total=0) == dev and _call(max_cand=0) == dev
    assert _call(n=1 << 30, total=1 << 30) == dev
    assert _call(max_pred=1) == dev and _call(max_pred=64) == dev
    assert _call(dist=(0, 0), bw=0, pen=(0, 0)) == dev
    assert _call(dp=(False, False), status=False) == dev                    # f, pred and the status are optional
    assert _call(dp=(True, False)) == dev
    assert _call(bw=1, pen=((1 << 31) - 1, 0)) == dev                       # the guard's edge: 2^31 - 1
    assert _call(bw=0, pen=(0, 2147483), dist=(2000, 1000)) == dev          # 2147483000
