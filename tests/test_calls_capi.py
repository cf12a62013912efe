"""mgl_sw_pileup_insertions_batch_device and mgl_sw_genotype_sites_device at the C ABI without a GPU: declared, exported, mirrored, the
call record of sixteen int32; every call-level bad argument is refused before any device work, on both sides of its edge; without a GPU
a well-formed call fails loudly; no kernel id and no flag was added, the ABI version stands; the Python methods and their defaults."""
import ctypes as C
import os
import re

from mgl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mgl_sw.h")).read()
INSERTIONS, GENOTYPE, PILEUP = "mgl_sw_pileup_insertions_batch_device", "mgl_sw_genotype_sites_device", "mgl_sw_pileup_alignments_batch_device"
DECLARED = {
    INSERTIONS: [
        "mgl_sw_ctx *ctx", "void *stream", "int64_t n", "const uint8_t *d_targets", "const int64_t *d_t_start", "const int32_t *d_t_len",
        "const uint8_t *d_queries", "const int64_t *d_q_start", "const int32_t *d_q_len", "const mgl_sw_chain_alignment *d_aln", "const char *d_cigar",
        "int cigar_stride", "const int32_t *d_cigar_len", "const int32_t *d_status_in", "const int32_t *d_select", "int64_t region_beg",
        "const mgl_sw_site *d_sites", "const int64_t *d_n_sites", "int64_t site_capacity", "int max_ins", "uint32_t *d_ins", "int32_t *d_status_out", "int flags"],
    GENOTYPE: [
        "mgl_sw_ctx *ctx", "void *stream", "const uint32_t *d_counts", "int64_t region_len", "const uint8_t *d_targets", "int64_t region_beg",
        "const mgl_sw_site *d_sites", "const int64_t *d_n_sites", "int64_t site_capacity", "const uint32_t *d_ins", "int max_ins", "int max_del", "int cost_match",
        "int cost_het", "int cost_error", "mgl_sw_call *d_calls_out", "int64_t call_capacity", "int64_t *d_n_calls_out", "uint8_t *d_ins_seq_out"],
}
CALL = ["pos", "kind", "len", "ref", "alt", "depth", "ref_count", "alt_count", "gt", "gq", "qual", "pl0", "pl1", "pl2", "flags", "reserved"]

D = 0x100000  # never dereferenced: every case below fails before any device access
MAX_REGION = (1 << 31) - 1


def _p(on, at=D):
    return C.c_void_p(at) if on else None


def _insertions(n=3, seqs=(True,) * 6, aln=(True,) * 3, stride=64, status_in=True, select=True, beg=0, sites=True, n_sites=True, cap=10, max_ins=16, ins=True,
                status=True, flags=0):
    s = [_p(x) for x in seqs]
    return _lib.lib().mgl_sw_pileup_insertions_batch_device(None, None, n, *s, _p(aln[0]), _p(aln[1]), stride, _p(aln[2]), _p(status_in), _p(select), beg,
                                                            _p(sites), _p(n_sites), cap, max_ins, _p(ins), _p(status), flags)


def _genotype(counts=True, length=1000, targets=True, beg=0, sites=True, n_sites=True, cap=10, ins=True, max_ins=16, max_del=64, costs=(11, 778, 6341),
              calls=True, call_cap=30, n_calls=True, seq=True):
    return _lib.lib().mgl_sw_genotype_sites_device(None, None, _p(counts), length, _p(targets), beg, _p(sites), _p(n_sites), cap, _p(ins), max_ins, max_del,
                                                   *costs, _p(calls), call_cap, _p(n_calls), _p(seq))


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
    # the first fifteen arguments, and region_beg behind them, are exactly the pileup's
    assert _args(INSERTIONS)[:16] == _args(PILEUP)[:16]
    rec = re.search(r"typedef struct mgl_sw_call \{(.*?)\} mgl_sw_call;", HEADER, re.S).group(1)
    assert re.sub(r"\s+", " ", rec).strip() == "int32_t " + ", ".join(CALL) + ";"
    assert C.sizeof(_lib.Call) == 64 and [f for f, _ in _lib.Call._fields_] == CALL and all(t is C.c_int32 for _, t in _lib.Call._fields_)
    assert HEADER.count("tests/calls_textbook.py") >= 2


def test_the_textbook_names_the_records_fields():
    import sys

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import calls_textbook as ctb

    assert list(ctb.Call._fields) == CALL and (ctb.SNV, ctb.DELETION, ctb.INSERTION, ctb.LONG_DEL) == (1, 2, 3, 1) and ctb.width(64) == 385


def test_python_methods_and_their_defaults():
    import inspect

    from mgl_amd import formats, smithwaterman as sw, synth

    for f in ("pileup_insertions_device", "genotype_sites_device", "map_reads_calls_device", "map_reads_calls"):
        assert hasattr(sw.MicrosoftSmithWaterman, f), f
    assert callable(formats.write_vcf) and callable(formats.read_vcf) and callable(synth.diploid_variant_set) and callable(sw.genotype_costs)
    d = {k: v.default for k, v in inspect.signature(sw.MicrosoftSmithWaterman.pileup_insertions_device).parameters.items()}
    assert (d["status_in"], d["select"], d["region_beg"], d["max_ins"], d["ins"], d["binary_cigar"], d["out"]) == (None, None, 0, 16, None, False, None)
    d = {k: v.default for k, v in inspect.signature(sw.MicrosoftSmithWaterman.genotype_sites_device).parameters.items()}
    assert (d["ins"], d["region_beg"], d["max_ins"], d["max_del"], d["error_phred"], d["costs"], d["call_capacity"], d["out"]) == (None, 0, 16, 64, 20, None, None, None)
    d = {k: v.default for k, v in inspect.signature(sw.MicrosoftSmithWaterman.map_reads_calls).parameters.items()}
    assert (d["min_mapq"], d["min_depth"], d["min_alt"], d["min_frac"], d["max_ins"], d["max_del"], d["error_phred"]) == (0, 4, 2, 64, 16, 64, 20)
    d = {k: v.default for k, v in inspect.signature(formats.write_vcf).parameters.items()}
    assert (d["starts"], d["min_qual"], d["sample"]) == (None, 0, "sample")
    assert list(inspect.signature(formats.write_vcf).parameters)[:5] == ["path", "ref_name", "ref_len", "ref", "calls"]
    assert inspect.signature(synth.diploid_variant_set).parameters["het"].default == "even"
    assert sw.genotype_costs(20) == (11, 6341, 778)
    assert sw.Call._fields == ("pos", "kind", "len", "ref", "alt", "depth", "ref_count", "alt_count", "gt", "gq", "qual", "pl", "flags")


def test_version_kernel_ids_and_flags_stand():
    assert re.search(r"#define MGL_SW_VERSION 104\b", HEADER)
    assert _lib.ABI_VERSION == 104 and _lib.lib().mgl_sw_version() == 104
    assert len(re.findall(r"^#define MGL_SW_KERNEL_\w+ \d+\b", HEADER, re.M)) == 13 == len(_lib.FILL_KERNEL_NAMES)
    assert len(re.findall(r"^#define MGL_SW_KERNEL_\w+ ", HEADER, re.M)) == 15
    flags = {k: int(v, 0) for k, v in re.findall(r"#define (MGL_SW_FLAG_\w+) (0x[0-9a-fA-F]+|\d+)\b", HEADER)}
    assert len(flags) == 7 and max(flags.values()) == 0x40 == _lib.FLAG_EXTEND_ADAPTIVE_BAND


def test_insertions_bad_arguments_before_any_device_work():
    bad = _lib.ERR_BAD_ARG
    for i in range(6):
        assert _insertions(seqs=tuple(x != i for x in range(6))) == bad
    for i in range(3):
        assert _insertions(aln=tuple(x != i for x in range(3))) == bad
    assert _insertions(n=-1) == bad and _insertions(n=(1 << 30) + 1) == bad
    assert _insertions(stride=0) == bad and _insertions(stride=-4) == bad
    for stride in (1, 2, 3, 5, 62):
        assert _insertions(stride=stride, flags=_lib.FLAG_BINARY_CIGAR) == bad
    assert _insertions(beg=-1) == bad
    assert _insertions(sites=False) == bad and _insertions(n_sites=False) == bad and _insertions(ins=False) == bad
    assert _insertions(cap=0) == bad and _insertions(cap=-1) == bad and _insertions(cap=(1 << 30) + 1) == bad
    assert _insertions(max_ins=0) == bad and _insertions(max_ins=-1) == bad and _insertions(max_ins=65) == bad
    assert _insertions(n=0, max_ins=65) == bad                   # an empty batch is checked all the same


def test_genotype_bad_arguments_before_any_device_work():
    bad = _lib.ERR_BAD_ARG
    for name in ("counts", "targets", "sites", "n_sites", "n_calls"):
        assert _genotype(**{name: False}) == bad, name
    assert _genotype(calls=False, call_cap=1) == bad and _genotype(seq=False, call_cap=1) == bad
    assert _genotype(length=0) == bad and _genotype(length=-1) == bad and _genotype(length=MAX_REGION + 1) == bad
    assert _genotype(beg=-1) == bad
    assert _genotype(cap=0) == bad and _genotype(cap=-1) == bad and _genotype(cap=(1 << 30) + 1) == bad
    assert _genotype(max_ins=0) == bad and _genotype(max_ins=65) == bad and _genotype(max_ins=0, ins=False) == bad
    assert _genotype(max_del=0) == bad and _genotype(max_del=-1) == bad and _genotype(max_del=4097) == bad
    for costs in ((0, 2, 3), (-1, 2, 3), (1, 2, (1 << 20) + 1), (1, 1, 3), (2, 1, 3), (1, 3, 3), (1, 3, 2), (3, 2, 1), (1 << 20, (1 << 20) + 1, (1 << 20) + 2)):
        assert _genotype(costs=costs) == bad, costs
    assert _genotype(call_cap=-1) == bad and _genotype(call_cap=(1 << 30) + 1) == bad


def test_well_formed_calls_without_a_context_are_device_errors_without_a_gpu():
    # (with a GPU the null context is the one thing left to refuse: MGL_SW_ERR_BAD_ARG, as the siblings do)
    dev = _lib.ERR_DEVICE if _lib.lib().mgl_sw_device_count() <= 0 else _lib.ERR_BAD_ARG
    assert _insertions() == dev and _insertions(n=0) == dev and _insertions(n=1 << 30) == dev
    assert _insertions(stride=1) == dev and _insertions(stride=4, flags=_lib.FLAG_BINARY_CIGAR) == dev and _insertions(stride=63, flags=~_lib.FLAG_BINARY_CIGAR) == dev
    assert _insertions(status_in=False) == dev and _insertions(select=False) == dev and _insertions(status=False) == dev
    assert _insertions(beg=0) == dev and _insertions(beg=1 << 40) == dev
    assert _insertions(cap=1) == dev and _insertions(cap=1 << 30) == dev and _insertions(max_ins=1) == dev and _insertions(max_ins=64) == dev
    assert _genotype() == dev and _genotype(length=1) == dev and _genotype(length=MAX_REGION) == dev and _genotype(beg=1 << 40) == dev
    assert _genotype(cap=1) == dev and _genotype(cap=1 << 30) == dev and _genotype(ins=False) == dev and _genotype(ins=False, seq=False) == dev
    assert _genotype(max_ins=1) == dev and _genotype(max_ins=64) == dev and _genotype(max_del=1) == dev and _genotype(max_del=4096) == dev
    assert _genotype(costs=(1, 2, 3)) == dev and _genotype(costs=((1 << 20) - 2, (1 << 20) - 1, 1 << 20)) == dev
    assert _genotype(call_cap=0) == dev and _genotype(call_cap=0, calls=False, seq=False) == dev and _genotype(call_cap=1 << 30) == dev
