"""mgl_sw_pileup_alignments_batch_device and mgl_sw_pileup_sites_device at the C ABI without a GPU: declared, exported, mirrored, the
site record of eight int32; every call-level bad argument is refused before any device work, on both sides of its edge; without a GPU
a well-formed call fails loudly; no kernel id and no flag was added, the ABI version stands; the Python methods and their defaults."""
import ctypes as C
import os
import re

from mgl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mgl_sw.h")).read()
PILEUP, SITES, DESCRIBE = "mgl_sw_pileup_alignments_batch_device", "mgl_sw_pileup_sites_device", "mgl_sw_describe_alignments_batch_device"
DECLARED = {
    PILEUP: [
        "mgl_sw_ctx *ctx", "void *stream", "int64_t n", "const uint8_t *d_targets", "const int64_t *d_t_start", "const int32_t *d_t_len",
        "const uint8_t *d_queries", "const int64_t *d_q_start", "const int32_t *d_q_len", "const mgl_sw_chain_alignment *d_aln", "const char *d_cigar",
        "int cigar_stride", "const int32_t *d_cigar_len", "const int32_t *d_status_in", "const int32_t *d_select", "int64_t region_beg", "int64_t region_len",
        "uint32_t *d_counts", "int32_t *d_status_out", "int flags"],
    SITES: [
        "mgl_sw_ctx *ctx", "void *stream", "const uint32_t *d_counts", "int64_t region_len", "const uint8_t *d_targets", "int64_t region_beg", "int min_depth",
        "int min_alt", "int min_frac", "uint8_t *d_call_out", "uint8_t *d_flags_out", "mgl_sw_site *d_sites_out", "int64_t site_capacity",
        "int64_t *d_n_sites_out"],
}
SITE = ["pos", "flags", "depth", "ref", "call", "call_count", "alt", "alt_count"]

D = 0x100000  # never dereferenced: every case below fails before any device access
MAX_REGION = (1 << 31) - 1


def _p(on, at=D):
    return C.c_void_p(at) if on else None


def _pileup(n=3, seqs=(True,) * 6, aln=(True,) * 3, stride=64, status_in=True, select=True, beg=0, length=1000, counts=True, status=True, flags=0):
    s = [_p(x) for x in seqs]
    return _lib.lib().mgl_sw_pileup_alignments_batch_device(None, None, n, *s, _p(aln[0]), _p(aln[1]), stride, _p(aln[2]), _p(status_in), _p(select), beg, length,
                                                            _p(counts), _p(status), flags)


def _sites(counts=True, length=1000, targets=True, beg=0, min_depth=4, min_alt=2, min_frac=64, call=True, flags=True, sites=True, cap=10, n_sites=True):
    return _lib.lib().mgl_sw_pileup_sites_device(None, None, _p(counts), length, _p(targets), beg, min_depth, min_alt, min_frac, _p(call), _p(flags), _p(sites), cap,
                                                 _p(n_sites))


def _args(name):
    text = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    decl = re.search(r"\bint %s\s*\((.*?)\);" % name, text, re.S).group(1)
    return [re.sub(r"\s+", " ", a).strip() for a in decl.split(",")]


def test_the_entries_are_declared_exported_and_mirrored():
    for name, declared in DECLARED.items():
        assert _args(name) == declared
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
        argtypes = getattr(_lib.lib(), name).argtypes
        assert len(argtypes) == len(declared)
        for a, t in zip(declared, argtypes):
            assert t is (C.c_void_p if "*" in a else C.c_int64 if a.startswith("int64_t") else C.c_int), a
    # the first thirteen arguments are exactly describe's
    assert _args(PILEUP)[:13] == _args(DESCRIBE)[:13]
    rec = re.search(r"typedef struct mgl_sw_site \{(.*?)\} mgl_sw_site;", HEADER, re.S).group(1)
    assert re.sub(r"\s+", " ", rec).strip() == "int32_t " + ", ".join(SITE) + ";"
    assert C.sizeof(_lib.Site) == 32 and [f for f, _ in _lib.Site._fields_] == SITE and all(t is C.c_int32 for _, t in _lib.Site._fields_)
    assert HEADER.count("tests/pileup_textbook.py") >= 2


def test_the_textbook_names_the_records_fields():
    import sys

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import pileup_textbook as ptb

    assert list(ptb.Site._fields) == SITE and ptb.PLANES == 8 and ptb.CALLS == b"ACGTN*"


def test_python_methods_and_their_defaults():
    import inspect

    from mgl_amd import formats, smithwaterman as sw, synth

    for f in ("pileup_device", "pileup_sites_device", "pileup", "map_reads_pileup_device", "map_reads_pileup"):
        assert hasattr(sw.MicrosoftSmithWaterman, f), f
    assert callable(formats.write_sites) and callable(synth.variant_mapping_set)
    d = {k: v.default for k, v in inspect.signature(sw.MicrosoftSmithWaterman.pileup_device).parameters.items()}
    assert (d["status_in"], d["select"], d["region"], d["counts"]) == (None, None, None, None)
    d = {k: v.default for k, v in inspect.signature(sw.MicrosoftSmithWaterman.pileup_sites_device).parameters.items()}
    assert (d["region_beg"], d["min_depth"], d["min_alt"], d["min_frac"], d["site_capacity"], d["call"], d["flags"]) == (0, 4, 2, 64, None, True, True)
    d = {k: v.default for k, v in inspect.signature(sw.MicrosoftSmithWaterman.pileup).parameters.items()}
    assert (d["spans"], d["positions"], d["region"]) == (None, None, None)
    d = {k: v.default for k, v in inspect.signature(sw.MicrosoftSmithWaterman.map_reads_pileup_device).parameters.items()}
    assert (d["counts"], d["min_mapq"]) == (None, 0)
    d = {k: v.default for k, v in inspect.signature(synth.variant_mapping_set).parameters.items()}
    assert (d["ref_len"], d["read_len"], d["step"], d["snvs"], d["dele"], d["ins"]) == (8000, 1000, 125, 10, 3, 2)


def test_version_kernel_ids_and_flags_stand():
    assert re.search(r"#define MGL_SW_VERSION 104\b", HEADER)
    assert _lib.ABI_VERSION == 104 and _lib.lib().mgl_sw_version() == 104
    assert len(re.findall(r"^#define MGL_SW_KERNEL_\w+ \d+\b", HEADER, re.M)) == 13 == len(_lib.FILL_KERNEL_NAMES)
    assert len(re.findall(r"^#define MGL_SW_KERNEL_\w+ ", HEADER, re.M)) == 15
    flags = {k: int(v, 0) for k, v in re.findall(r"#define (MGL_SW_FLAG_\w+) (0x[0-9a-fA-F]+|\d+)\b", HEADER)}
    assert len(flags) == 7 and max(flags.values()) == 0x40 == _lib.FLAG_EXTEND_ADAPTIVE_BAND


def test_pileup_bad_arguments_before_any_device_work():
    bad = _lib.ERR_BAD_ARG
    for i in range(6):
        assert _pileup(seqs=tuple(x != i for x in range(6))) == bad
    for i in range(3):
        assert _pileup(aln=tuple(x != i for x in range(3))) == bad
    assert _pileup(n=-1) == bad and _pileup(n=(1 << 30) + 1) == bad
    assert _pileup(stride=0) == bad and _pileup(stride=-4) == bad
    for stride in (1, 2, 3, 5, 62):
        assert _pileup(stride=stride, flags=_lib.FLAG_BINARY_CIGAR) == bad
    assert _pileup(beg=-1) == bad
    assert _pileup(length=0) == bad and _pileup(length=-1) == bad and _pileup(length=MAX_REGION + 1) == bad
    assert _pileup(counts=False) == bad


def test_sites_bad_arguments_before_any_device_work():
    bad = _lib.ERR_BAD_ARG
    assert _sites(counts=False) == bad and _sites(targets=False) == bad and _sites(n_sites=False) == bad
    assert _sites(sites=False, cap=1) == bad
    assert _sites(length=0) == bad and _sites(length=-1) == bad and _sites(length=MAX_REGION + 1) == bad
    assert _sites(beg=-1) == bad
    assert _sites(min_depth=0) == bad and _sites(min_alt=0) == bad and _sites(min_depth=-1) == bad and _sites(min_alt=-1) == bad
    assert _sites(min_frac=0) == bad and _sites(min_frac=257) == bad
    assert _sites(cap=-1) == bad and _sites(cap=(1 << 30) + 1) == bad


def test_well_formed_calls_without_a_context_are_device_errors_without_a_gpu():
    # (with a GPU the null context is the one thing left to refuse: MGL_SW_ERR_BAD_ARG, as the siblings do)
    dev = _lib.ERR_DEVICE if _lib.lib().mgl_sw_device_count() <= 0 else _lib.ERR_BAD_ARG
    assert _pileup() == dev and _pileup(n=0) == dev and _pileup(n=1 << 30) == dev
    assert _pileup(stride=1) == dev and _pileup(stride=4, flags=_lib.FLAG_BINARY_CIGAR) == dev and _pileup(stride=63, flags=~_lib.FLAG_BINARY_CIGAR) == dev
    assert _pileup(status_in=False) == dev and _pileup(select=False) == dev and _pileup(status=False) == dev
    assert _pileup(beg=0) == dev and _pileup(beg=1 << 40) == dev and _pileup(length=1) == dev and _pileup(length=MAX_REGION) == dev
    assert _sites() == dev and _sites(length=1) == dev and _sites(length=MAX_REGION) == dev and _sites(beg=1 << 40) == dev
    assert _sites(min_depth=1) == dev and _sites(min_alt=1) == dev and _sites(min_frac=1) == dev and _sites(min_frac=256) == dev
    assert _sites(cap=0) == dev and _sites(cap=0, sites=False) == dev and _sites(cap=1 << 30) == dev
    assert _sites(call=False) == dev and _sites(flags=False) == dev


def test_variant_mapping_set_and_its_truth():
    from mgl_amd import synth

    ref, reads, planted = synth.variant_mapping_set(5)
    assert synth.variant_mapping_set(5) == (ref, reads, planted) and synth.variant_mapping_set(6)[0] != ref
    assert len(ref) == 8000 and set(ref) <= set(b"ACGT")
    kinds = sorted(v[0] for v in planted)
    assert kinds == ["D", "I"] + ["X"] * 10
    at = sorted(v[1] for v in planted)
    assert at[0] >= 1000 and at[-1] < 7000 and min(b - a for a, b in zip(at, at[1:])) >= 300
    # the donor, rebuilt from the truth, is what the reads tile
    donor, shift = bytearray(ref), 0
    for kind, pos, what in sorted(planted, key=lambda v: v[1]):
        if kind == "X":
            assert ref[pos] != what[0] and len(what) == 1
            donor[pos + shift] = what[0]
        elif kind == "D":
            assert what == ref[pos:pos + 3] and all(b not in (ref[pos - 1], ref[pos + 3]) for b in what)
            del donor[pos + shift:pos + shift + 3]
            shift -= 3
        else:  # the inserted bases stand behind reference position pos
            assert len(what) == 2 and all(b not in (ref[pos], ref[pos + 1]) for b in what)
            donor[pos + shift + 1:pos + shift + 1] = what
            shift += 2
    donor = bytes(donor)
    assert len(donor) == 8000 - 3 + 2
    starts = list(range(0, len(donor) - 1000 + 1, 125))
    assert len(reads) == len(starts)
    for k, (s, r) in enumerate(zip(starts, reads)):
        assert (synth.revcomp(r) if k % 2 else r) == donor[s:s + 1000]
