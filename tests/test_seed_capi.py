"""mgl_sw_seed_batch_device at the C ABI without a GPU: declared, exported, mirrored; every call-level bad argument is refused before any
device work, on both sides of its edge; without a GPU a well-formed call fails loudly; no kernel id and no flag was added, the ABI version
stands."""
import ctypes as C
import os
import re

import pytest

from mgl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mgl_sw_seed_batch_device"
HEADER = open(os.path.join(ROOT, "include", "mgl_sw.h")).read()
ARGS = ["mgl_sw_ctx *ctx", "void *stream", "int64_t n", "const uint8_t *d_targets", "const int64_t *d_t_start", "const int32_t *d_t_len",
        "const uint8_t *d_queries", "const int64_t *d_q_start", "const int32_t *d_q_len", "int k", "int w", "int max_occ", "int merge", "int max_cand",
        "int64_t cand_capacity", "int64_t *d_cand_start_out", "int32_t *d_cand_t_out", "int32_t *d_cand_q_out", "int32_t *d_cand_len_out",
        "int32_t *d_status_out"]


def _call(ctx=None, n=3, seqs=(True,) * 6, k=15, w=10, max_occ=8, merge=1, max_cand=4096, capacity=100, cands=(True,) * 4, status=True):
    L = _lib.lib()
    d = C.c_void_p(0x1000)  # never dereferenced: every case below fails before any device access
    p = lambda on: d if on else None  # noqa: E731
    return L.mgl_sw_seed_batch_device(ctx, None, n, *[p(x) for x in seqs], k, w, max_occ, merge, max_cand, capacity, *[p(x) for x in cands], p(status))


def test_entry_declared_exported_and_mirrored():
    text = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    decl = re.search(r"\bint %s\s*\((.*?)\);" % NAME, text, re.S).group(1)
    assert [re.sub(r"\s+", " ", a).strip() for a in decl.split(",")] == ARGS and len(ARGS) == 20
    assert NAME in _lib.SYMBOLS and hasattr(_lib.lib(), NAME)
    assert len(_lib.lib().mgl_sw_seed_batch_device.argtypes) == 20
    assert "tests/seed_textbook.py" in HEADER
    from mgl_amd import smithwaterman as sw

    assert all(hasattr(sw.MicrosoftSmithWaterman, f) for f in ("seed", "seed_device", "align_reads_device"))


def test_version_kernel_ids_and_flags_stand():
    assert re.search(r"#define MGL_SW_VERSION 104\b", HEADER)
    assert _lib.ABI_VERSION == 104 and _lib.lib().mgl_sw_version() == 104
    assert len(re.findall(r"^#define MGL_SW_KERNEL_\w+ \d+\b", HEADER, re.M)) == 13 == len(_lib.FILL_KERNEL_NAMES)
    assert len(re.findall(r"^#define MGL_SW_KERNEL_\w+ ", HEADER, re.M)) == 15
    flags = {k: int(v, 0) for k, v in re.findall(r"#define (MGL_SW_FLAG_\w+) (0x[0-9a-fA-F]+|\d+)\b", HEADER)}
    assert len(flags) == 7 and max(flags.values()) == 0x40 == _lib.FLAG_EXTEND_ADAPTIVE_BAND


def test_bad_arguments_before_any_device_work():
    bad = _lib.ERR_BAD_ARG
    for i in range(6):
        assert _call(seqs=tuple(x != i for x in range(6))) == bad
    for i in range(4):
        assert _call(cands=tuple(x != i for x in range(4))) == bad
    assert _call(n=-1) == bad and _call(n=(1 << 30) + 1) == bad
    assert _call(k=3) == bad and _call(k=17) == bad and _call(k=-1) == bad
    assert _call(w=0) == bad and _call(w=33) == bad
    assert _call(max_occ=0) == bad and _call(max_occ=65) == bad
    assert _call(merge=-1) == bad and _call(merge=2) == bad
    assert _call(max_cand=0) == bad and _call(max_cand=8193) == bad
    assert _call(capacity=-1) == bad and _call(capacity=(1 << 30) + 1) == bad


def test_without_a_gpu_a_well_formed_call_is_a_device_error():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    dev = _lib.ERR_DEVICE
    assert _call() == dev
    assert _call(n=0) == dev and _call(n=1 << 30) == dev
    assert _call(k=4) == dev and _call(k=16) == dev
    assert _call(w=1) == dev and _call(w=32) == dev
    assert _call(max_occ=1) == dev and _call(max_occ=64) == dev
    assert _call(merge=0) == dev and _call(merge=1) == dev
    assert _call(max_cand=1) == dev and _call(max_cand=8192) == dev
    assert _call(capacity=0) == dev and _call(capacity=1 << 30) == dev
    assert _call(status=False) == dev  # the status is optional
