"""mgl_sw_describe_alignments_batch_device at the C ABI without a GPU: declared, exported, mirrored, its record's eight fields; the two
alignment records it reads have one layout; every call-level bad argument is refused before any device work, on both sides of its
edge; without a GPU a well-formed call fails loudly; no kernel id and no flag was added, the ABI version stands."""
import ctypes as C
import inspect
import os
import re

from mgl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mgl_sw.h")).read()
NAME = "mgl_sw_describe_alignments_batch_device"
DECLARED = [
    "mgl_sw_ctx *ctx", "void *stream", "int64_t n", "const uint8_t *d_targets", "const int64_t *d_t_start", "const int32_t *d_t_len",
    "const uint8_t *d_queries", "const int64_t *d_q_start", "const int32_t *d_q_len", "const mgl_sw_chain_alignment *d_aln", "const char *d_cigar",
    "int cigar_stride", "const int32_t *d_cigar_len", "const int32_t *d_status_in", "mgl_sw_alignment_stats *d_stats_out", "char *d_md_out", "int md_stride",
    "char *d_xcigar_out", "int xcigar_stride", "int32_t *d_status_out", "int flags"]
FIELDS = ["n_match", "n_mismatch", "n_ins", "n_del", "n_ins_runs", "n_del_runs", "md_len", "xcigar_len"]

D = C.c_void_p(0x1000)  # never dereferenced: every case below fails before any device access


def _p(on):
    return D if on else None


def _describe(n=3, seqs=(True,) * 6, aln=True, cigar=True, cigar_stride=64, cigar_len=True, status_in=True, stats=True, md=True, md_stride=64, xcigar=True,
              xcigar_stride=64, status=True, flags=0):
    return _lib.lib().mgl_sw_describe_alignments_batch_device(None, None, n, *[_p(x) for x in seqs], _p(aln), _p(cigar), cigar_stride, _p(cigar_len),
                                                              _p(status_in), _p(stats), _p(md), md_stride, _p(xcigar), xcigar_stride, _p(status), flags)


def test_the_entry_is_declared_exported_and_mirrored():
    text = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    decl = re.search(r"\bint %s\s*\((.*?)\);" % NAME, text, re.S).group(1)
    assert [re.sub(r"\s+", " ", a).strip() for a in decl.split(",")] == DECLARED and len(DECLARED) == 21
    assert NAME in _lib.SYMBOLS and hasattr(_lib.lib(), NAME)
    argtypes = _lib.lib().mgl_sw_describe_alignments_batch_device.argtypes
    assert len(argtypes) == 21
    for a, t in zip(DECLARED, argtypes):
        assert t is (C.c_void_p if "*" in a else C.c_int64 if a.startswith("int64_t") else C.c_int), a
    rec = re.search(r"typedef struct mgl_sw_alignment_stats \{(.*?)\} mgl_sw_alignment_stats;", HEADER, re.S).group(1)
    assert re.sub(r"\s+", " ", rec).strip() == "int32_t " + ", ".join(FIELDS) + ";"
    assert C.sizeof(_lib.AlignmentStats) == 32 and [f for f, _ in _lib.AlignmentStats._fields_] == FIELDS
    assert all(t is C.c_int32 for _, t in _lib.AlignmentStats._fields_)
    assert HEADER.count("tests/describe_textbook.py") >= 1 and "aligned 16-byte blocks" in HEADER


def test_the_two_alignment_records_have_one_layout():
    body = lambda name: re.sub(r"\s+", " ", re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), HEADER, re.S).group(1)).strip()  # noqa: E731
    seed, chain = body("mgl_sw_seed_alignment"), body("mgl_sw_chain_alignment")
    assert seed.replace("seed_score", "anchor_score") == chain == "int32_t score, t_beg, t_end, q_beg, q_end, anchor_score, dropped, cigar_from;"
    assert C.sizeof(_lib.SeedAlignment) == C.sizeof(_lib.ChainAlignment) == 32
    for f in ("t_beg", "t_end", "q_beg", "q_end"):
        assert getattr(_lib.SeedAlignment, f).offset == getattr(_lib.ChainAlignment, f).offset == 4 * (1 + ["t_beg", "t_end", "q_beg", "q_end"].index(f))
    src = open(os.path.join(ROOT, "mgl_amd", "csrc", "sw_describe.cpp")).read()
    assert "static_assert(sizeof(mgl_sw_seed_alignment) == sizeof(mgl_sw_chain_alignment)" in src and "offsetof(mgl_sw_seed_alignment, q_end)" in src


def test_python_methods_formats_and_defaults():
    from mgl_amd import formats, smithwaterman as sw

    for f in ("describe_device", "describe", "map_reads_described_device", "map_reads_described"):
        assert hasattr(sw.MicrosoftSmithWaterman, f), f
    assert sw.DescribedMapResult._fields == sw.RankedMapResult._fields + ("q_beg", "q_end", "nm", "n_match", "block_len", "md", "xcigars")
    assert list(sw.AlignmentStats._fields) == FIELDS
    d = {k: v.default for k, v in inspect.signature(sw.MicrosoftSmithWaterman.describe_device).parameters.items()}
    assert (d["status_in"], d["md_stride"], d["xcigar_stride"], d["binary_cigar"], d["md"], d["xcigar"], d["out"]) == (None, None, None, False, True, True, None)
    d = {k: v.default for k, v in inspect.signature(sw.MicrosoftSmithWaterman.describe).parameters.items()}
    assert (d["spans"], d["binary_cigar"]) == (None, False)
    d = {k: v.default for k, v in inspect.signature(sw.MicrosoftSmithWaterman.map_reads_described).parameters.items()}
    assert (d["band"], d["zdrop"], d["slack"], d["strands"], d["max_tl"], d["extended"]) == (64, -1, 200, 2, None, False)
    for f in ("sam_header", "write_sam", "write_paf", "read_sam"):
        assert hasattr(formats, f), f
    assert inspect.signature(formats.write_sam).parameters["extended"].default is False
    for f in ("describe_bench.py", "describe_fuzz.py"):
        assert os.path.exists(os.path.join(ROOT, "scripts", f)), f
    mk = open(os.path.join(ROOT, "mgl_amd", "csrc", "Makefile")).read()
    assert all(("$(HERE)sw_describe" + ext) in mk for ext in (".hip", ".cpp", ".h"))


def test_version_kernel_ids_and_flags_stand():
    assert re.search(r"#define MGL_SW_VERSION 104\b", HEADER)
    assert _lib.ABI_VERSION == 104 and _lib.lib().mgl_sw_version() == 104
    assert len(re.findall(r"^#define MGL_SW_KERNEL_\w+ \d+\b", HEADER, re.M)) == 13 == len(_lib.FILL_KERNEL_NAMES)
    assert len(re.findall(r"^#define MGL_SW_KERNEL_\w+ ", HEADER, re.M)) == 15
    flags = {k: int(v, 0) for k, v in re.findall(r"#define (MGL_SW_FLAG_\w+) (0x[0-9a-fA-F]+|\d+)\b", HEADER)}
    assert len(flags) == 7 and max(flags.values()) == 0x40 == _lib.FLAG_EXTEND_ADAPTIVE_BAND and flags["MGL_SW_FLAG_BINARY_CIGAR"] == _lib.FLAG_BINARY_CIGAR


def test_bad_arguments_before_any_device_work():
    bad, binary = _lib.ERR_BAD_ARG, _lib.FLAG_BINARY_CIGAR
    assert _describe(n=-1) == bad and _describe(n=(1 << 30) + 1) == bad
    for i in range(6):
        assert _describe(seqs=tuple(x != i for x in range(6))) == bad
    assert _describe(aln=False) == bad and _describe(cigar=False) == bad and _describe(cigar_len=False) == bad and _describe(stats=False) == bad
    assert _describe(cigar_stride=0) == bad and _describe(cigar_stride=-4) == bad
    assert _describe(md_stride=0) == bad and _describe(xcigar_stride=0) == bad and _describe(md_stride=-1) == bad and _describe(xcigar_stride=-1) == bad
    for stride in (5, 6, 7, 63):  # binary: whole words
        assert _describe(cigar_stride=stride, flags=binary) == bad and _describe(xcigar_stride=stride, flags=binary) == bad


def test_a_well_formed_call_without_a_context_is_a_device_error_without_a_gpu():
    # (with a GPU the null context is the one thing left to refuse: MGL_SW_ERR_BAD_ARG, as the siblings do)
    dev, binary = _lib.ERR_DEVICE if _lib.lib().mgl_sw_device_count() <= 0 else _lib.ERR_BAD_ARG, _lib.FLAG_BINARY_CIGAR
    assert _describe() == dev and _describe(n=0) == dev and _describe(n=1 << 30) == dev
    assert _describe(status_in=False) == dev and _describe(status=False) == dev and _describe(md=False) == dev and _describe(xcigar=False) == dev
    assert _describe(status_in=False, status=False, md=False, xcigar=False) == dev
    assert _describe(cigar_stride=1) == dev and _describe(md_stride=1) == dev and _describe(xcigar_stride=1) == dev
    assert _describe(md=False, md_stride=0) == dev and _describe(xcigar=False, xcigar_stride=0) == dev  # a stride matters where the output is wanted
    assert _describe(xcigar=False, xcigar_stride=7, flags=binary) == dev and _describe(md_stride=7, flags=binary) == dev  # MD is text either way
    for stride in (4, 8, 64):
        assert _describe(cigar_stride=stride, xcigar_stride=stride, flags=binary) == dev
    assert _describe(cigar_stride=5, xcigar_stride=7) == dev  # text: any stride
    assert _describe(flags=0x7fffffff & ~binary) == dev  # no other flag is read
