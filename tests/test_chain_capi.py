"""mgl_sw_align_chain_batch_device at the C ABI without a GPU: declared, exported, mirrored; bad arguments are refused before any device
work; without a GPU a well-formed call fails loudly; no kernel id and no flag was added, the ABI version stands."""
import ctypes as C
import os
import re

import pytest

from mgl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mgl_sw_align_chain_batch_device"
HEADER = open(os.path.join(ROOT, "include", "mgl_sw.h")).read()


def _call(ctx=None, n=1, seqs=True, index=True, anchors=(True, True, True, True), total=3, aln=True, left=True, right=True, gaps=True, max_tl=10, max_ql=10,
          max_gap=(5, 5), band=4, zdrop=100, stride=64, flags=0, cigar=True, cigar_len=True):
    L = _lib.lib()
    d = C.c_void_p(0x1000)  # never dereferenced: every case below fails before any device access
    p = lambda on: d if on else None  # noqa: E731
    return L.mgl_sw_align_chain_batch_device(ctx, None, n, p(seqs), p(index), d, d, d, d, p(anchors[0]), p(anchors[1]), p(anchors[2]), p(anchors[3]), total,
                                             max_tl, max_ql, max_gap[0], max_gap[1], 200, -150, -260, -11, band, zdrop, p(aln), p(left), p(right), p(gaps),
                                             p(cigar), stride, p(cigar_len), None, flags)


def test_entry_declared_exported_and_mirrored():
    text = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    assert re.search(r"\bint %s\s*\(" % NAME, text)
    assert NAME in _lib.SYMBOLS
    assert hasattr(_lib.lib(), NAME)
    assert len(_lib.lib().mgl_sw_align_chain_batch_device.argtypes) == 33
    decl = re.search(r"\bint %s\s*\((.*?)\);" % NAME, text, re.S).group(1)
    args = [a.strip() for a in decl.split(",")]
    assert len(args) == 33
    # the seed entry's arguments with the three seed arrays replaced and d_gap_score_out added
    seed = [a.strip() for a in re.search(r"\bint mgl_sw_extend_seed_batch_device\s*\((.*?)\);", text, re.S).group(1).split(",")]
    mine = [a for a in args if not re.search(r"anchor|max_gap|d_gap_score_out", a)]
    assert mine == [a.replace("mgl_sw_seed_alignment", "mgl_sw_chain_alignment") for a in seed if "d_seed_" not in a]
    assert [a for a in args if re.search(r"anchor|max_gap", a)] == ["const int64_t *d_anchor_start", "const int32_t *d_anchor_t", "const int32_t *d_anchor_q",
                                                                    "const int32_t *d_anchor_len", "int64_t total_anchors", "int max_gap_tl", "int max_gap_ql"]
    assert re.search(r"#define MGL_SW_VERSION 104\b", HEADER)
    assert _lib.ABI_VERSION == 104 and _lib.lib().mgl_sw_version() == 104


def test_alignment_record_layout():
    names = ["score", "t_beg", "t_end", "q_beg", "q_end", "anchor_score", "dropped", "cigar_from"]
    assert C.sizeof(_lib.ChainAlignment) == 32 and [f for f, _ in _lib.ChainAlignment._fields_] == names
    assert all(t is C.c_int32 for _, t in _lib.ChainAlignment._fields_)
    body = re.search(r"typedef struct mgl_sw_chain_alignment \{(.*?)\} mgl_sw_chain_alignment;", HEADER, re.S).group(1)
    assert re.sub(r"\s+", " ", body).strip() == "int32_t " + ", ".join(names) + ";"
    # the seed record's order, anchor_score in seed_score's place
    assert [n.replace("anchor_score", "seed_score") for n in names] == [f for f, _ in _lib.SeedAlignment._fields_]


def test_no_kernel_id_and_no_flag_was_added():
    numeric = re.findall(r"^#define MGL_SW_KERNEL_\w+ \d+\b", HEADER, re.M)
    assert len(numeric) == 13 == len(_lib.FILL_KERNEL_NAMES)
    assert len(re.findall(r"^#define MGL_SW_KERNEL_\w+ ", HEADER, re.M)) == 15
    assert (_lib.KERNEL_EXTEND, _lib.KERNEL_EXTEND_ADAPTIVE) == (13, 14)
    flags = {k: int(v, 0) for k, v in re.findall(r"#define (MGL_SW_FLAG_\w+) (0x[0-9a-fA-F]+|\d+)\b", HEADER)}
    assert max(flags.values()) == 0x40 == _lib.FLAG_EXTEND_ADAPTIVE_BAND


def test_bad_arguments_before_any_device_work():
    bad = _lib.ERR_BAD_ARG
    assert _call(n=-1) == bad
    assert _call(n=(1 << 30) + 1) == bad
    assert _call(seqs=False) == bad
    assert _call(index=False) == bad
    for k in range(4):
        assert _call(anchors=tuple(x != k for x in range(4))) == bad
    assert _call(total=-1) == bad
    assert _call(total=(1 << 30) + 1) == bad
    assert _call(aln=False) == bad
    assert _call(aln=False, cigar=False, flags=_lib.FLAG_SCORE_ONLY) == bad
    assert _call(band=-1) == bad
    assert _call(max_tl=0) == bad and _call(max_ql=0) == bad
    assert _call(max_gap=(-1, 5)) == bad and _call(max_gap=(5, -1)) == bad
    assert _call(stride=1) == bad                                   # text: "1M" needs 2 bytes
    assert _call(stride=3, flags=_lib.FLAG_BINARY_CIGAR) == bad     # binary: one element is 4
    assert _call(cigar=False) == bad
    assert _call(cigar_len=False) == bad
    assert _call(band=-1, flags=_lib.FLAG_EXTEND_ADAPTIVE_BAND) == bad


def test_without_a_gpu_a_well_formed_call_is_a_device_error():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    assert _call() == _lib.ERR_DEVICE
    assert _call(band=0) == _lib.ERR_DEVICE
    assert _call(zdrop=-1) == _lib.ERR_DEVICE
    assert _call(n=0) == _lib.ERR_DEVICE
    assert _call(total=0) == _lib.ERR_DEVICE                        # (every pair then has K < 1: a pair's status, not the call's)
    assert _call(max_gap=(0, 0)) == _lib.ERR_DEVICE
    assert _call(left=False, right=False, gaps=False) == _lib.ERR_DEVICE  # the side records and the gap scores are optional
    assert _call(flags=_lib.FLAG_EXTEND_TO_QUERY_END | _lib.FLAG_EXTEND_ADAPTIVE_BAND) == _lib.ERR_DEVICE
    assert _call(stride=0, cigar=False, cigar_len=False, flags=_lib.FLAG_SCORE_ONLY) == _lib.ERR_DEVICE
