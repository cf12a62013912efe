"""mgl_sw_rank_chains_batch_device at the C ABI without a GPU: declared, exported, mirrored, its record's twelve fields; every call-level
bad argument is refused before any device work, on both sides of its edge; without a GPU a well-formed call fails loudly; no kernel id
and no flag was added, the ABI version stands."""
import ctypes as C
import os
import re

from mgl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mgl_sw.h")).read()
NAME = "mgl_sw_rank_chains_batch_device"
DECLARED = [
    "mgl_sw_ctx *ctx", "void *stream", "int64_t n", "int strands", "const int32_t *d_row_q_len", "const int64_t *d_cand_start", "const int32_t *d_cand_t",
    "const int32_t *d_cand_q", "const int32_t *d_cand_len", "int64_t total_cand", "const int32_t *d_f", "const int32_t *d_pred", "const int32_t *d_row_status",
    "int max_cand", "int max_chains", "int min_score", "int min_cnt", "int mask_level", "int32_t *d_n_chains_out", "mgl_sw_ranked_chain *d_records_out",
    "int64_t *d_ranked_start_out", "int32_t *d_ranked_t_out", "int32_t *d_ranked_q_out", "int32_t *d_ranked_len_out", "int32_t *d_status_out"]
FIELDS = ["score", "strand", "n_anchors", "t_beg", "t_end", "q_beg", "q_end", "parent", "n_sub", "subsc", "mapq", "end_index"]

D = C.c_void_p(0x1000)  # never dereferenced: every case below fails before any device access


def _p(on):
    return D if on else None


def _rank(n=3, strands=2, ins=(True,) * 5, total=100, dp=(True, True), row_status=True, max_cand=4096, max_chains=4, min_score=40, min_cnt=3, mask_level=128,
          outs=(True, True), anchors=(True,) * 4, status=True):
    return _lib.lib().mgl_sw_rank_chains_batch_device(None, None, n, strands, *[_p(x) for x in ins], total, *[_p(x) for x in dp], _p(row_status), max_cand,
                                                      max_chains, min_score, min_cnt, mask_level, *[_p(x) for x in outs], *[_p(x) for x in anchors], _p(status))


def test_the_entry_is_declared_exported_and_mirrored():
    text = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    decl = re.search(r"\bint %s\s*\((.*?)\);" % NAME, text, re.S).group(1)
    assert [re.sub(r"\s+", " ", a).strip() for a in decl.split(",")] == DECLARED
    assert NAME in _lib.SYMBOLS and hasattr(_lib.lib(), NAME)
    argtypes = _lib.lib().mgl_sw_rank_chains_batch_device.argtypes
    assert len(argtypes) == len(DECLARED)
    for a, t in zip(DECLARED, argtypes):
        assert t is (C.c_void_p if "*" in a else C.c_int64 if a.startswith("int64_t") else C.c_int), a
    rec = re.search(r"typedef struct mgl_sw_ranked_chain \{(.*?)\} mgl_sw_ranked_chain;", HEADER, re.S).group(1)
    assert re.sub(r"\s+", " ", rec).strip() == "int32_t " + ", ".join(FIELDS) + ";"
    assert C.sizeof(_lib.RankedChain) == 48 and [f for f, _ in _lib.RankedChain._fields_] == FIELDS
    assert all(t is C.c_int32 for _, t in _lib.RankedChain._fields_)
    assert HEADER.count("tests/rank_textbook.py") >= 1


def test_python_methods_and_the_repeat_mapping_set():
    import inspect

    from mgl_amd import smithwaterman as sw, synth

    for f in ("rank_chains", "rank_chains_device", "map_reads_ranked_device", "map_reads_ranked"):
        assert hasattr(sw.MicrosoftSmithWaterman, f), f
    assert sw.RankedMapResult._fields == sw.MapResult._fields + ("mapq", "n_chains", "secondary")
    assert list(sw.RankedChain._fields) == FIELDS
    for f in ("rank_chains", "rank_chains_device", "map_reads_ranked_device"):
        d = {k: v.default for k, v in inspect.signature(getattr(sw.MicrosoftSmithWaterman, f)).parameters.items()}
        assert (d["max_chains"], d["min_score"], d["min_cnt"], d["mask_level"]) == (4, 40, 3, 128), f
    ref, reads, truth = synth.mapping_set(5, 4, length=600, spacer=100)
    assert synth.repeat_mapping_set(5, 4, length=600, spacer=100) == (ref, reads, truth, [])
    ref2, reads2, truth2, copy = synth.repeat_mapping_set(5, 4, length=600, spacer=100, copies=3, divergence=0.0)
    assert (reads2, truth2) == (reads, truth) and ref2[:len(ref)] == ref and len(copy) == 3
    at = len(ref)
    for (pos, n, _), (cpos, cn) in zip(truth, copy):
        assert (cpos, cn) == (at, n) and ref2[cpos:cpos + n] == ref[pos:pos + n]
        at += n + 100
    assert at == len(ref2) and set(ref2) <= set(b"ACGT")
    ref3, _, _, copy3 = synth.repeat_mapping_set(5, 4, length=600, spacer=100, copies=3, divergence=0.1)
    assert copy3 == copy and len(ref3) == len(ref2) and ref3[:len(ref)] == ref and set(ref3) <= set(b"ACGT")
    for (pos, n, _), (cpos, _) in zip(truth, copy):
        differ = sum(a != b for a, b in zip(ref3[cpos:cpos + n], ref[pos:pos + n]))
        assert 0.04 * n < differ < 0.2 * n  # substitutions by ANOTHER base at rate 0.1
    assert synth.repeat_mapping_set(5, 4, length=600, spacer=100, copies=3, divergence=0.1)[0] == ref3


def test_version_kernel_ids_and_flags_stand():
    assert re.search(r"#define MGL_SW_VERSION 104\b", HEADER)
    assert _lib.ABI_VERSION == 104 and _lib.lib().mgl_sw_version() == 104
    assert len(re.findall(r"^#define MGL_SW_KERNEL_\w+ \d+\b", HEADER, re.M)) == 13 == len(_lib.FILL_KERNEL_NAMES)
    assert len(re.findall(r"^#define MGL_SW_KERNEL_\w+ ", HEADER, re.M)) == 15
    flags = {k: int(v, 0) for k, v in re.findall(r"#define (MGL_SW_FLAG_\w+) (0x[0-9a-fA-F]+|\d+)\b", HEADER)}
    assert len(flags) == 7 and max(flags.values()) == 0x40 == _lib.FLAG_EXTEND_ADAPTIVE_BAND


def test_bad_arguments_before_any_device_work():
    bad = _lib.ERR_BAD_ARG
    for i in range(5):
        assert _rank(ins=tuple(x != i for x in range(5))) == bad
    assert _rank(dp=(False, True)) == bad and _rank(dp=(True, False)) == bad
    assert _rank(outs=(False, True)) == bad and _rank(outs=(True, False)) == bad
    for i in range(4):  # the anchor outputs: all four or none
        assert _rank(anchors=tuple(x != i for x in range(4))) == bad and _rank(anchors=tuple(x == i for x in range(4))) == bad
    assert _rank(strands=0) == bad and _rank(strands=3) == bad and _rank(strands=-1) == bad
    assert _rank(n=-1) == bad and _rank(n=(1 << 29) + 1) == bad and _rank(strands=1, n=(1 << 30) + 1) == bad
    assert _rank(total=-1) == bad and _rank(total=(1 << 30) + 1) == bad
    assert _rank(max_chains=0) == bad and _rank(max_chains=17) == bad
    assert _rank(mask_level=0) == bad and _rank(mask_level=257) == bad
    assert _rank(max_cand=-1) == bad and _rank(max_cand=8193) == bad
    assert _rank(min_score=0) == bad and _rank(min_cnt=0) == bad


def test_a_well_formed_call_without_a_context_is_a_device_error_without_a_gpu():
    # (with a GPU the null context is the one thing left to refuse: MGL_SW_ERR_BAD_ARG, as the siblings do)
    dev = _lib.ERR_DEVICE if _lib.lib().mgl_sw_device_count() <= 0 else _lib.ERR_BAD_ARG
    assert _rank() == dev
    assert _rank(strands=1) == dev and _rank(n=0) == dev and _rank(n=1 << 29) == dev and _rank(strands=1, n=1 << 30) == dev
    assert _rank(total=0) == dev and _rank(total=1 << 30) == dev
    assert _rank(max_chains=1) == dev and _rank(max_chains=16) == dev
    assert _rank(mask_level=1) == dev and _rank(mask_level=256) == dev
    assert _rank(max_cand=0) == dev and _rank(max_cand=8192) == dev
    assert _rank(min_score=1) == dev and _rank(min_cnt=1) == dev
    assert _rank(row_status=False) == dev and _rank(status=False) == dev and _rank(anchors=(False,) * 4) == dev
    assert _rank(row_status=False, status=False, anchors=(False,) * 4) == dev
