"""mgl_sw_expand_chains_batch_device and mgl_sw_classify_alignments_batch_device at the C ABI without a GPU: declared, exported,
mirrored, their two records of eight int32; every call-level bad argument is refused before any device work, on both sides of its
edge; without a GPU a well-formed call fails loudly; no kernel id and no flag was added, the ABI version stands; the Python methods
and their defaults."""
import ctypes as C
import os
import re

from mgl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mgl_sw.h")).read()
EXPAND, CLASSIFY = "mgl_sw_expand_chains_batch_device", "mgl_sw_classify_alignments_batch_device"
DECLARED = {
    EXPAND: [
        "mgl_sw_ctx *ctx", "void *stream", "int64_t n", "const uint8_t *d_queries", "const int64_t *d_q_start", "const int32_t *d_q_len",
        "int64_t query_bytes", "const int32_t *d_rank_status", "const int32_t *d_n_chains", "const mgl_sw_ranked_chain *d_records", "int max_chains",
        "const int64_t *d_ranked_start", "const int32_t *d_ranked_t", "const int32_t *d_ranked_q", "const int32_t *d_ranked_len", "int64_t total_anchors",
        "int keep_secondary", "int64_t job_capacity", "int64_t *d_n_jobs_out", "int64_t *d_job_start_out", "mgl_sw_job *d_jobs_out",
        "int64_t *d_job_q_start_out", "int32_t *d_job_q_len_out", "int64_t *d_job_anchor_start_out", "int32_t *d_job_anchor_t_out",
        "int32_t *d_job_anchor_q_out", "int32_t *d_job_anchor_len_out", "uint8_t *d_oriented_out", "int32_t *d_status_out"],
    CLASSIFY: [
        "mgl_sw_ctx *ctx", "void *stream", "int64_t n", "const int64_t *d_job_start", "const mgl_sw_job *d_jobs", "int64_t job_capacity",
        "const mgl_sw_chain_alignment *d_aln", "const int32_t *d_aln_status", "int match", "int min_score", "int mask_level", "mgl_sw_line *d_lines_out",
        "int32_t *d_n_lines_out", "int32_t *d_primary_job_out", "int32_t *d_status_out"],
}
JOB = ["read", "rank", "strand", "n_anchors", "chain_score", "chain_parent", "q_len", "reserved"]
LINE = ["order", "flag", "mapq", "parent", "n_sub", "subsc", "fwd_q_beg", "fwd_q_end"]

D = 0x100000  # never dereferenced: every case below fails before any device access


def _p(on, at=D):
    return C.c_void_p(at) if on else None


def _expand(n=3, reads=(True,) * 3, query_bytes=1000, rank_status=True, chains=(True,) * 2, max_chains=4, ranked=(True,) * 4, total=100, keep=1, cap=12,
            outs=(True,) * 9, oriented=D + 0x10000, status=True, queries=D):
    r = [_p(x) for x in ranked]
    return _lib.lib().mgl_sw_expand_chains_batch_device(
        None, None, n, _p(reads[0], queries), _p(reads[1]), _p(reads[2]), query_bytes, _p(rank_status), _p(chains[0]), _p(chains[1]), max_chains, *r, total,
        keep, cap, *[_p(x) for x in outs], _p(oriented is not None, oriented or 0), _p(status))


def _classify(n=3, ins=(True,) * 4, cap=12, match=200, min_score=40, mask_level=128, outs=(True,) * 3, status=True):
    return _lib.lib().mgl_sw_classify_alignments_batch_device(None, None, n, _p(ins[0]), _p(ins[1]), cap, _p(ins[2]), _p(ins[3]), match, min_score, mask_level,
                                                              *[_p(x) for x in outs], _p(status))


def test_the_entries_are_declared_exported_and_mirrored():
    text = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name, declared in DECLARED.items():
        decl = re.search(r"\bint %s\s*\((.*?)\);" % name, text, re.S).group(1)
        assert [re.sub(r"\s+", " ", a).strip() for a in decl.split(",")] == declared
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
        argtypes = getattr(_lib.lib(), name).argtypes
        assert len(argtypes) == len(declared)
        for a, t in zip(declared, argtypes):
            assert t is (C.c_void_p if "*" in a else C.c_int64 if a.startswith("int64_t") else C.c_int), a
    for struct, mirror, fields in (("mgl_sw_job", _lib.Job, JOB), ("mgl_sw_line", _lib.Line, LINE)):
        rec = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), HEADER, re.S).group(1)
        assert re.sub(r"\s+", " ", rec).strip() == "int32_t " + ", ".join(fields) + ";"
        assert C.sizeof(mirror) == 32 and [f for f, _ in mirror._fields_] == fields and all(t is C.c_int32 for _, t in mirror._fields_)
    assert HEADER.count("tests/lines_textbook.py") >= 2


def test_the_textbook_names_the_records_fields():
    import sys

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import lines_textbook as ltb

    assert list(ltb.Job._fields) == JOB and list(ltb.Line._fields) == LINE and ltb.MAX_JOBS == 16


def test_python_methods_and_their_defaults():
    import inspect

    from mgl_amd import smithwaterman as sw

    from mgl_amd import formats

    for f in ("expand_chains_device", "classify_alignments_device", "map_reads_all_device", "map_reads_all"):
        assert hasattr(sw.MicrosoftSmithWaterman, f), f
    assert callable(formats.write_sam_all) and callable(formats.write_paf_all)
    assert sw.AllMapResult._fields == ("n_lines", "lines")
    assert sw.Line._fields == ("ref_beg", "ref_end", "strand", "score", "cigar", "q_beg", "q_end", "flag", "mapq", "parent", "nm", "n_match", "block_len", "md",
                               "xcigar", "rid", "rname", "status")
    d = {k: v.default for k, v in inspect.signature(sw.MicrosoftSmithWaterman.map_reads_all).parameters.items()}
    assert (d["band"], d["zdrop"], d["slack"], d["strands"], d["max_tl"], d["extended"]) == (64, -1, 200, 2, None, False)
    d = {k: v.default for k, v in inspect.signature(sw.MicrosoftSmithWaterman.expand_chains_device).parameters.items()}
    assert (d["max_chains"], d["keep_secondary"], d["job_capacity"], d["out"]) == (4, True, None, None)
    d = {k: v.default for k, v in inspect.signature(sw.MicrosoftSmithWaterman.classify_alignments_device).parameters.items()}
    assert (d["min_score"], d["mask_level"], d["out"]) == (40, 128, None)
    d = {k: v.default for k, v in inspect.signature(sw.MicrosoftSmithWaterman.map_reads_all_device).parameters.items()}
    assert (d["max_chains"], d["min_score"], d["min_cnt"], d["mask_level"], d["keep_secondary"], d["job_capacity"]) == (4, 40, 3, 128, True, None)
    r = {k: v.default for k, v in inspect.signature(sw.MicrosoftSmithWaterman.map_reads_ranked_device).parameters.items()}
    assert all(d[k] == r[k] for k in ("strands", "max_cand", "max_chains", "min_score", "min_cnt", "mask_level"))


def test_version_kernel_ids_and_flags_stand():
    assert re.search(r"#define MGL_SW_VERSION 104\b", HEADER)
    assert _lib.ABI_VERSION == 104 and _lib.lib().mgl_sw_version() == 104
    assert len(re.findall(r"^#define MGL_SW_KERNEL_\w+ \d+\b", HEADER, re.M)) == 13 == len(_lib.FILL_KERNEL_NAMES)
    assert len(re.findall(r"^#define MGL_SW_KERNEL_\w+ ", HEADER, re.M)) == 15
    flags = {k: int(v, 0) for k, v in re.findall(r"#define (MGL_SW_FLAG_\w+) (0x[0-9a-fA-F]+|\d+)\b", HEADER)}
    assert len(flags) == 7 and max(flags.values()) == 0x40 == _lib.FLAG_EXTEND_ADAPTIVE_BAND


def test_expand_bad_arguments_before_any_device_work():
    bad = _lib.ERR_BAD_ARG
    for i in range(3):
        assert _expand(reads=tuple(x != i for x in range(3))) == bad
    for i in range(2):
        assert _expand(chains=tuple(x != i for x in range(2))) == bad
    for i in range(4):
        assert _expand(ranked=tuple(x != i for x in range(4))) == bad
    for i in range(9):
        assert _expand(outs=tuple(x != i for x in range(9))) == bad
    assert _expand(oriented=None) == bad
    assert _expand(n=-1) == bad and _expand(n=(1 << 29) + 1) == bad
    assert _expand(max_chains=0) == bad and _expand(max_chains=17) == bad and _expand(max_chains=-1) == bad
    assert _expand(cap=-1) == bad and _expand(cap=(1 << 30) + 1) == bad
    assert _expand(total=-1) == bad and _expand(total=(1 << 30) + 1) == bad
    assert _expand(query_bytes=-1) == bad and _expand(query_bytes=(1 << 40) + 1) == bad
    assert _expand(keep=2) == bad and _expand(keep=-1) == bad
    # the oriented buffer (2 * query_bytes) against the reads' (query_bytes): a byte of overlap at either end, and inside
    assert _expand(oriented=D) == bad and _expand(oriented=D + 999) == bad and _expand(oriented=D - 1999) == bad and _expand(oriented=D - 500) == bad


def test_classify_bad_arguments_before_any_device_work():
    bad = _lib.ERR_BAD_ARG
    for i in range(4):
        assert _classify(ins=tuple(x != i for x in range(4))) == bad
    for i in range(3):
        assert _classify(outs=tuple(x != i for x in range(3))) == bad
    assert _classify(n=-1) == bad and _classify(n=(1 << 29) + 1) == bad
    assert _classify(cap=-1) == bad and _classify(cap=(1 << 30) + 1) == bad
    assert _classify(mask_level=0) == bad and _classify(mask_level=257) == bad
    assert _classify(match=0) == bad and _classify(min_score=0) == bad


def test_well_formed_calls_without_a_context_are_device_errors_without_a_gpu():
    # (with a GPU the null context is the one thing left to refuse: MGL_SW_ERR_BAD_ARG, as the siblings do)
    dev = _lib.ERR_DEVICE if _lib.lib().mgl_sw_device_count() <= 0 else _lib.ERR_BAD_ARG
    assert _expand() == dev and _expand(n=0) == dev and _expand(n=1 << 29) == dev
    assert _expand(max_chains=1) == dev and _expand(max_chains=16) == dev
    assert _expand(cap=0) == dev and _expand(cap=1 << 30) == dev and _expand(total=0) == dev and _expand(total=1 << 30) == dev
    assert _expand(query_bytes=0) == dev and _expand(query_bytes=1 << 40, oriented=D + (1 << 40)) == dev
    assert _expand(keep=0) == dev and _expand(rank_status=False) == dev and _expand(status=False) == dev
    assert _expand(oriented=D + 1000) == dev and _expand(oriented=D - 2000) == dev  # the buffers touch and do not overlap
    assert _classify() == dev and _classify(n=0) == dev and _classify(n=1 << 29) == dev
    assert _classify(cap=0) == dev and _classify(cap=1 << 30) == dev
    assert _classify(mask_level=1) == dev and _classify(mask_level=256) == dev
    assert _classify(match=1) == dev and _classify(min_score=1) == dev and _classify(status=False) == dev


def test_split_mapping_set_and_its_truth():
    from mgl_amd import synth

    ref, reads, truth = synth.split_mapping_set(11, 8, length=2000, spacer=3000)
    base, plain, placed = synth.mapping_set(11, 8, length=2000, spacer=3000)
    pairs = synth.chain_pairs(11, 8, 2000)
    assert ref == base and len(reads) == len(truth) == 8 and synth.split_mapping_set(11, 8, length=2000, spacer=3000) == (ref, reads, truth)
    for p, (read, parts) in enumerate(zip(reads, truth)):
        (pos0, n0, s0, b0, e0), (pos1, n1, s1, b1, e1) = parts
        a, b = pairs[p][1], pairs[(p + 1) % 8][1]
        assert (pos0, n0) == placed[p][:2] and (pos1, n1) == placed[(p + 1) % 8][:2] and (b0, e0, b1, e1) == (0, len(a) // 2, len(a) // 2, len(read))
        assert (s0, s1) == (0, 1 if p % 3 == 2 else 0) and read[b0:e0] == a[:len(a) // 2]
        assert (synth.revcomp(read[b1:e1]) if s1 else read[b1:e1]) == b[len(b) // 2:]
        # each part is its window's read: the window T of the pair the part was cut from
        assert ref[pos0:pos0 + n0] == pairs[p][0] and ref[pos1:pos1 + n1] == pairs[(p + 1) % 8][0]
    assert [t[1][2] for t in truth] == [0, 0, 1, 0, 0, 1, 0, 0]
