"""mgl_sw_seed_strands_batch_device and mgl_sw_select_strand_batch_device at the C ABI without a GPU: declared, exported, mirrored; every
call-level bad argument is refused before any device work, on both sides of its edge; without a GPU a well-formed call fails loudly; no
kernel id and no flag was added, the ABI version stands."""
import ctypes as C
import os
import re

import pytest

from mgl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mgl_sw.h")).read()
SEED = "mgl_sw_seed_strands_batch_device"
SELECT = "mgl_sw_select_strand_batch_device"
SEED_ARGS = ["mgl_sw_ctx *ctx", "void *stream", "int64_t n", "const uint8_t *d_targets", "const int64_t *d_t_start", "const int32_t *d_t_len",
             "const uint8_t *d_queries", "const int64_t *d_q_start", "const int32_t *d_q_len", "int k", "int w", "int max_occ", "int merge", "int max_cand",
             "int64_t cand_capacity", "int64_t *d_cand_start_out", "int32_t *d_cand_t_out", "int32_t *d_cand_q_out", "int32_t *d_cand_len_out",
             "int32_t *d_row_t_len_out", "int32_t *d_row_q_len_out", "int32_t *d_status_out"]
SELECT_ARGS = ["mgl_sw_ctx *ctx", "void *stream", "int64_t n", "const uint8_t *d_queries", "const int64_t *d_q_start", "const int32_t *d_q_len",
               "const int64_t *d_chain_start", "const int32_t *d_chain_t", "const int32_t *d_chain_q", "const int32_t *d_chain_len",
               "const int32_t *d_chain_score", "int64_t total_chain", "int64_t query_bytes", "int32_t *d_strand_out", "uint8_t *d_queries_out",
               "int64_t *d_anchor_start_out", "int32_t *d_anchor_t_out", "int32_t *d_anchor_q_out", "int32_t *d_anchor_len_out", "int32_t *d_score_out",
               "int32_t *d_status_out"]

D = C.c_void_p(0x1000)  # never dereferenced: every case below fails before any device access


def _p(on):
    return D if on else None


def _seed(ctx=None, n=3, seqs=(True,) * 6, k=15, w=10, max_occ=8, merge=1, max_cand=4096, capacity=100, cands=(True,) * 4, rows=(True, True), status=True):
    return _lib.lib().mgl_sw_seed_strands_batch_device(ctx, None, n, *[_p(x) for x in seqs], k, w, max_occ, merge, max_cand, capacity,
                                                       *[_p(x) for x in cands], *[_p(x) for x in rows], _p(status))


def _select(ctx=None, n=3, ins=(True,) * 8, total=100, query_bytes=1000, outs=(True,) * 6, score=True, status=True):
    return _lib.lib().mgl_sw_select_strand_batch_device(ctx, None, n, *[_p(x) for x in ins], total, query_bytes, *[_p(x) for x in outs], _p(score),
                                                        _p(status))


def _declared(name):
    text = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    decl = re.search(r"\bint %s\s*\((.*?)\);" % name, text, re.S).group(1)
    return [re.sub(r"\s+", " ", a).strip() for a in decl.split(",")]


def test_entries_declared_exported_and_mirrored():
    assert _declared(SEED) == SEED_ARGS and len(SEED_ARGS) == 22
    assert _declared(SELECT) == SELECT_ARGS and len(SELECT_ARGS) == 21
    # the first 19 arguments are mgl_sw_seed_batch_device's, by name, type and order
    assert SEED_ARGS[:19] == _declared("mgl_sw_seed_batch_device")[:19]
    for name, count in ((SEED, 22), (SELECT, 21)):
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
        assert len(getattr(_lib.lib(), name).argtypes) == count
    assert HEADER.count("tests/strand_textbook.py") >= 2
    from mgl_amd import smithwaterman as sw, synth

    assert all(hasattr(sw.MicrosoftSmithWaterman, f) for f in ("seed_strands", "seed_strands_device", "select_strand_device", "align_reads_strands_device"))
    assert synth.revcomp(b"AACGNt") == b"tNCGTT"
    assert "[ql - q_end, ql - q_beg)" in sw.MicrosoftSmithWaterman.align_reads_strands_device.__doc__


def test_version_kernel_ids_and_flags_stand():
    assert re.search(r"#define MGL_SW_VERSION 104\b", HEADER)
    assert _lib.ABI_VERSION == 104 and _lib.lib().mgl_sw_version() == 104
    assert len(re.findall(r"^#define MGL_SW_KERNEL_\w+ \d+\b", HEADER, re.M)) == 13 == len(_lib.FILL_KERNEL_NAMES)
    assert len(re.findall(r"^#define MGL_SW_KERNEL_\w+ ", HEADER, re.M)) == 15
    flags = {k: int(v, 0) for k, v in re.findall(r"#define (MGL_SW_FLAG_\w+) (0x[0-9a-fA-F]+|\d+)\b", HEADER)}
    assert len(flags) == 7 and max(flags.values()) == 0x40 == _lib.FLAG_EXTEND_ADAPTIVE_BAND


def test_seed_strands_bad_arguments_before_any_device_work():
    bad = _lib.ERR_BAD_ARG
    for i in range(6):
        assert _seed(seqs=tuple(x != i for x in range(6))) == bad
    for i in range(4):
        assert _seed(cands=tuple(x != i for x in range(4))) == bad
    assert _seed(n=-1) == bad and _seed(n=(1 << 29) + 1) == bad and _seed(n=1 << 30) == bad
    assert _seed(k=3) == bad and _seed(k=17) == bad and _seed(k=-1) == bad
    assert _seed(w=0) == bad and _seed(w=33) == bad
    assert _seed(max_occ=0) == bad and _seed(max_occ=65) == bad
    assert _seed(merge=-1) == bad and _seed(merge=2) == bad
    assert _seed(max_cand=0) == bad and _seed(max_cand=8193) == bad
    assert _seed(capacity=-1) == bad and _seed(capacity=(1 << 30) + 1) == bad


def test_select_strand_bad_arguments_before_any_device_work():
    bad = _lib.ERR_BAD_ARG
    for i in range(8):
        assert _select(ins=tuple(x != i for x in range(8))) == bad
    for i in range(6):
        assert _select(outs=tuple(x != i for x in range(6))) == bad
    assert _select(n=-1) == bad and _select(n=(1 << 29) + 1) == bad
    assert _select(total=-1) == bad and _select(total=(1 << 30) + 1) == bad
    assert _select(query_bytes=-1) == bad


def test_without_a_gpu_a_well_formed_call_is_a_device_error():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    dev = _lib.ERR_DEVICE
    assert _seed() == dev
    assert _seed(n=0) == dev and _seed(n=1 << 29) == dev
    assert _seed(k=4) == dev and _seed(k=16) == dev
    assert _seed(w=1) == dev and _seed(w=32) == dev
    assert _seed(max_occ=1) == dev and _seed(max_occ=64) == dev
    assert _seed(merge=0) == dev and _seed(merge=1) == dev
    assert _seed(max_cand=1) == dev and _seed(max_cand=8192) == dev
    assert _seed(capacity=0) == dev and _seed(capacity=1 << 30) == dev
    assert _seed(status=False) == dev and _seed(rows=(False, True)) == dev and _seed(rows=(True, False)) == dev and _seed(rows=(False, False)) == dev
    assert _select() == dev
    assert _select(n=0) == dev and _select(n=1 << 29) == dev
    assert _select(total=0) == dev and _select(total=1 << 30) == dev
    assert _select(query_bytes=0) == dev
    assert _select(score=False) == dev and _select(status=False) == dev and _select(score=False, status=False) == dev
