"""tests/describe_textbook.py, the definition of mgl_sw_describe_alignments_batch_device, pinned without a GPU:
by the MD and NM tags of the reference's own BAM fixture, by an independent restatement on random alignments, by hand cases worked
out by hand, and by the round trip through formats.reference_under_read."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import describe_cases as dc  # noqa: E402
import describe_textbook as dtb  # noqa: E402
from mgl_amd import formats  # noqa: E402

BAM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "HiSeq.1mb.1RG.2k_lines.bam")


def _core(rec, cigar):
    """the read without its clips and the CIGAR without them"""
    seq, k, core = rec.seq, 0, []
    lead = sum(n for n, op in cigar[:1] if op == "S")
    for n, op in cigar:
        if op in "SH":
            continue
        core.append((n, "M" if op in "M=X" else op))
        k += n if op in "MI" else 0
    return seq[lead:lead + k], core


def test_the_bam_fixtures_md_and_nm_tags():
    _, _, records = formats.read_bam(BAM)
    assert len(records) == 1677
    used = own = indels = 0
    longest = 0
    for rec in records:
        if rec.flag & 4:
            continue
        rebuilt = formats.reference_under_read(rec)
        if rebuilt is None:
            continue
        try:  # the CIGAR that rebuilt it: the record's own, or OC's (reference_under_read tries them in this order)
            formats._rebuild(rec)
            cigar, is_own = rec.cigar, True
        except (AssertionError, IndexError):
            cigar, is_own = formats.cigar_text_to_elements(rec.tags["OC"]), False
        if any(op not in "MIDS" for _, op in cigar):
            continue
        query, core = _core(rec, cigar)
        d = dtb.describe(rebuilt[0], query, core)
        assert d.md.decode() == rec.tags["MD"], rec.name
        if is_own:
            assert dtb.nm(d) == rec.tags["NM"] == rebuilt[1], rec.name
            own += 1
        used += 1
        indels += bool(d.n_ins or d.n_del)
        longest = max(longest, len(d.md))
    assert used >= 1652 and own >= 1648 and indels >= 25 and longest == 31, (used, own, indels, longest)


def test_the_restatement_by_columns_on_random_alignments():
    rng = np.random.default_rng(5)
    for k in range(400):
        t, q, cigar = dc.random_alignment(rng, int(rng.integers(0, 12)), alphabet=b"ACGTNacgt" if k % 3 == 0 else b"ACGT", p_mismatch=float(rng.choice((0.0, 0.1, 0.6))))
        assert dtb.describe(t, q, cigar) == dtb.describe_by_columns(t, q, cigar), (t, q, cigar)


HAND = [
    # (target, query, cigar, counts (match, mismatch, ins, del, ins runs, del runs), MD, extended CIGAR)
    (b"", b"", "", (0, 0, 0, 0, 0, 0), "0", ""),
    (b"", b"ACG", "3I", (0, 0, 3, 0, 1, 0), "0", "3I"),
    (b"ACG", b"", "3D", (0, 0, 0, 3, 0, 1), "0^ACG0", "3D"),
    (b"ACGT", b"ACTTGT", "2M2I2M", (4, 0, 2, 0, 1, 0), "4", "2=2I2="),                 # I inside a match run: the run goes on
    (b"ACGGTA", b"ACCA", "2M2D2M", (3, 1, 0, 2, 0, 1), "2^GG0T1", "2=2D1X1="),          # D then mismatch
    (b"ACGGTA", b"ATTA", "2M2D2M", (3, 1, 0, 2, 0, 1), "1C0^GG2", "1=1X2D2="),          # mismatch then D
    (b"ACGT", b"ATTT", "4M", (2, 2, 0, 0, 0, 0), "1C0G1", "1=2X1="),                    # two mismatches in a row
    (b"ACGT", b"CCGA", "4M", (2, 2, 0, 0, 0, 0), "0A2T0", "1X2=1X"),                    # first and last column
    (b"AC", b"AC", "1M1M", (2, 0, 0, 0, 0, 0), "2", "2="),                              # merged across an element border
    (b"ACGT", b"AT", "1M1D1D1M", (2, 0, 0, 2, 0, 2), "1^C0^G1", "1=2D1="),              # two D elements: two MD tokens, one merged element
    (b"acgt", b"ACGT", "4M", (0, 4, 0, 0, 0, 0), "0a0c0g0t0", "4X"),                    # bytes: no case folding
    (b"ANGT", b"ANGN", "4M", (3, 1, 0, 0, 0, 0), "3T0", "3=1X"),                        # N equals N and nothing else
]


@pytest.mark.parametrize("case", HAND, ids=[c[2] or "empty" for c in HAND])
def test_hand_cases(case):
    t, q, cigar, counts, md, xc = case
    d = dtb.describe(t, q, formats.cigar_text_to_elements(cigar))
    assert tuple(d[:6]) == counts and d.md == md.encode() and dtb.xcigar_text(d.xcigar) == xc
    assert dtb.nm(d) == counts[1] + counts[2] + counts[3] and dtb.block_len(d) == sum(counts[:4])


@pytest.mark.parametrize("run", [9, 10, 99, 100, 9999, 10000])
def test_runs_at_the_digit_borders(run):
    t = b"A" * run + b"C" + b"G" * run
    q = b"A" * run + b"T" + b"G" * run
    d = dtb.describe(t, q, [(2 * run + 1, "M")])
    assert d.md == b"%dC%d" % (run, run) and dtb.xcigar_text(d.xcigar) == "%d=1X%d=" % (run, run) and d.n_match == 2 * run
    assert dtb.xcigar_bytes(d.xcigar, True) == np.asarray([run << 4 | 7, 1 << 4 | 8, run << 4 | 7], "<u4").tobytes()
    assert dtb.stats(d, True)[6:] == [2 * len(str(run)) + 1, 12] and dtb.stats(d)[7] == 2 * len(str(run)) + 4


def test_binary_op_codes_are_the_bam_ones():
    assert all(formats.BAM_CIGAR_OPS[code] == op for op, code in dtb.BAM_OP.items())


def test_what_is_not_an_alignment_is_refused():
    for t, q, cigar in ((b"AC", b"AC", [(3, "M")]), (b"AC", b"AC", [(1, "M")]), (b"AC", b"AC", [(2, "S")]), (b"AC", b"AC", [(0, "M"), (2, "M")]),
                        (b"AC", b"A", [(1, "M"), (2, "D")]), (b"A", b"AC", [(1, "M"), (2, "I")])):
        with pytest.raises(ValueError):
            dtb.describe(t, q, cigar)


def test_round_trip_through_reference_under_read():
    rng = np.random.default_rng(9)
    for _ in range(200):
        t, q, cigar = dc.random_alignment(rng, int(rng.integers(1, 10)), p_mismatch=0.15)
        d = dtb.describe(t, q, cigar)
        rec = formats.BamRecord("r", 0, 0, 0, 60, cigar, q, b"", {"MD": d.md.decode()})
        assert formats.reference_under_read(rec) == (t, dtb.nm(d))
