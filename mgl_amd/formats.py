"""Wire / on-disk formats either side of the alignment path.

Inputs: FASTA / FASTQ readers and writers (plain or gzip), a minimal BAM reader (BGZF is multi-member gzip,
so the standard library is enough) that also rebuilds the reference bases under each aligned read from
SEQ + CIGAR + MD -- which turns the reference repo's only real sequencing data,
``src/test/resources/HiSeq.1mb.1RG.2k_lines.bam`` (kept as a data fixture in tests/golden/), into realistic
(target, query) pairs.  Outputs: BAM-style binary CIGAR (``len << 4 | op``, what
``MGL_SW_FLAG_BINARY_CIGAR`` makes the kernels emit) <-> the text of sw.cpp:251-252.

The reference moves sequences as ASCII inside a direct ByteBuffer (MicrosoftSmithWaterman.java:73-75) and
CIGARs as ASCII text (…SmithWaterman.cpp:65-69); these helpers are the formats a caller actually holds.
"""
import gzip
import io
import re
import struct
from collections import namedtuple

import numpy as np

BAM_CIGAR_OPS = "MIDNSHP=X"
_SEQ_NT16 = "=ACMGRSVTWYHKDBN"


def _open(path, mode="rt"):
    path = str(path)
    with open(path, "rb") as f:
        magic = f.read(2)
    if magic == b"\x1f\x8b":
        return gzip.open(path, mode)
    return open(path, mode)


# --------------------------------------------------------------------------------------------- FASTA / FASTQ
def read_fasta(path):
    """Yield (name, description, sequence bytes) per record; sequence lines are joined, case kept
    (the aligner compares raw bytes, sw.cpp:55)."""
    name, desc, parts = None, "", []
    with _open(path) as f:
        for line in f:
            line = line.rstrip("\r\n")
            if line.startswith(">"):
                if name is not None:
                    yield name, desc, "".join(parts).encode()
                head = line[1:].split(None, 1)
                name, desc, parts = (head[0] if head else ""), (head[1] if len(head) > 1 else ""), []
            elif line and name is not None:
                parts.append(line)
    if name is not None:
        yield name, desc, "".join(parts).encode()


def write_fasta(path, records, width=80):
    """records: iterable of (name, description, sequence bytes / uint8 array)."""
    op = gzip.open if str(path).endswith(".gz") else open
    with op(path, "wt") as f:
        for name, desc, seq in records:
            seq = bytes(seq).decode()
            f.write(">" + name + (" " + desc if desc else "") + "\n")
            for k in range(0, len(seq), width):
                f.write(seq[k:k + width] + "\n")


def read_fastq(path):
    """Yield (name, description, sequence bytes, quality bytes) per four-line record."""
    with _open(path) as f:
        while True:
            head = f.readline()
            if not head:
                return
            seq = f.readline().rstrip("\r\n")
            plus = f.readline()
            qual = f.readline().rstrip("\r\n")
            if not head.startswith("@") or not plus.startswith("+") or len(seq) != len(qual):
                raise ValueError("malformed FASTQ record near %r" % head[:40])
            h = head[1:].rstrip("\r\n").split(None, 1)
            yield (h[0] if h else ""), (h[1] if len(h) > 1 else ""), seq.encode(), qual.encode()


def write_fastq(path, records):
    """records: iterable of (name, description, sequence bytes, quality bytes or None -> 'I' * len)."""
    op = gzip.open if str(path).endswith(".gz") else open
    with op(path, "wt") as f:
        for name, desc, seq, qual in records:
            seq = bytes(seq).decode()
            qual = "I" * len(seq) if qual is None else bytes(qual).decode()
            f.write("@" + name + (" " + desc if desc else "") + "\n" + seq + "\n+\n" + qual + "\n")


# --------------------------------------------------------------------------------------------- CIGAR
def cigar_text_to_elements(text):
    """'6M1D6M' -> [(6, 'M'), (1, 'D'), (6, 'M')]"""
    out = [(int(n), op) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", text)]
    if "".join("%d%s" % e for e in out) != text:
        raise ValueError("not a CIGAR: %r" % text)
    return out


def cigar_elements_to_binary(elements):
    """[(len, op)] -> uint32 array, BAM encoding (len << 4 | op code; M=0 I=1 D=2 N=3 S=4 H=5 P=6 '='=7 X=8)."""
    return np.array([(n << 4) | BAM_CIGAR_OPS.index(op) for n, op in elements], dtype=np.uint32)


def cigar_binary_to_text(words):
    return "".join("%d%s" % (int(w) >> 4, BAM_CIGAR_OPS[int(w) & 15]) for w in words)


# --------------------------------------------------------------------------------------------- BAM
BamRecord = namedtuple("BamRecord", "name ref_id pos flag mapq cigar seq qual tags")


def _bam_tags(buf, q, end):
    tags = {}
    while q < end:
        tag, ty = buf[q:q + 2].decode(), chr(buf[q + 2])
        q += 3
        if ty == "A":
            tags[tag], q = chr(buf[q]), q + 1
        elif ty in "cCsSiIf":
            fmt = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I", "f": "<f"}[ty]
            tags[tag], q = struct.unpack_from(fmt, buf, q)[0], q + struct.calcsize(fmt)
        elif ty in "ZH":
            e = buf.index(b"\0", q)
            tags[tag], q = buf[q:e].decode(), e + 1
        elif ty == "B":
            st, cnt = chr(buf[q]), struct.unpack_from("<i", buf, q + 1)[0]
            fmt = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}[st]
            tags[tag] = struct.unpack_from("<%d%s" % (cnt, fmt), buf, q + 5)
            q += 5 + cnt * struct.calcsize(fmt)
        else:
            raise ValueError("unknown BAM tag type %r" % ty)
    return tags


def read_bam(path):
    """Returns (header text, [(reference name, length)], [BamRecord]).  ``cigar`` is a list of (len, op),
    ``seq`` ASCII bytes, ``qual`` raw phred bytes (not +33)."""
    with gzip.open(path, "rb") as f:  # BGZF blocks are gzip members
        buf = f.read()
    if buf[:4] != b"BAM\x01":
        raise ValueError("not a BAM file")
    l_text = struct.unpack_from("<i", buf, 4)[0]
    text = buf[8:8 + l_text].rstrip(b"\0").decode()
    p = 8 + l_text
    n_ref = struct.unpack_from("<i", buf, p)[0]
    p += 4
    refs = []
    for _ in range(n_ref):
        ln = struct.unpack_from("<i", buf, p)[0]
        refs.append((buf[p + 4:p + 4 + ln - 1].decode(), struct.unpack_from("<i", buf, p + 4 + ln)[0]))
        p += 8 + ln
    records = []
    while p + 4 <= len(buf):
        size = struct.unpack_from("<i", buf, p)[0]
        ref_id, pos, l_name, mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHi", buf, p + 4)
        q = p + 36
        name = buf[q:q + l_name - 1].decode()
        q += l_name
        cigar = [(w >> 4, BAM_CIGAR_OPS[w & 15]) for w in struct.unpack_from("<%dI" % n_cig, buf, q)]
        q += 4 * n_cig
        packed = np.frombuffer(buf, dtype=np.uint8, count=(l_seq + 1) // 2, offset=q)
        codes = np.empty(2 * len(packed), dtype=np.uint8)
        codes[0::2], codes[1::2] = packed >> 4, packed & 15
        seq = "".join(_SEQ_NT16[c] for c in codes[:l_seq]).encode()
        q += (l_seq + 1) // 2
        qual = bytes(buf[q:q + l_seq])
        q += l_seq
        records.append(BamRecord(name, ref_id, pos, flag, mapq, cigar, seq, qual, _bam_tags(buf, q, p + 4 + size)))
        p += 4 + size
    return text, refs, records


def reference_under_read(rec):
    """Rebuild the reference bases a read is aligned to from SEQ + CIGAR + MD (SAM spec section 1.5, MD tag).
    Returns (reference bytes, edit distance implied by the reconstruction), or None without a usable MD tag.
    Indel-realigned records keep the MD of their ORIGINAL alignment (tag OC): that CIGAR is tried second."""
    if rec.tags.get("MD") is None:
        return None
    for cigar in (rec.cigar, cigar_text_to_elements(rec.tags["OC"]) if "OC" in rec.tags else None):
        if cigar is None:
            continue
        try:
            return _rebuild(rec._replace(cigar=cigar))
        except (AssertionError, IndexError):
            pass
    return None


def _rebuild(rec):
    md = rec.tags["MD"]
    # 1) the read bases that sit on reference positions (M/=/X), in reference order, with deletions as gaps
    aligned, k = [], 0
    for n, op in rec.cigar:
        if op in "M=X":
            aligned.extend(rec.seq[k:k + n])
            k += n
        elif op in "IS":
            k += n
        elif op in "DN":
            aligned.extend([None] * n)
    # 2) walk MD over them: numbers = matches, letters = reference base at a mismatch, ^letters = deleted bases
    out, pos, edits = [], 0, 0
    for num, dele, sub in re.findall(r"(\d+)|\^([A-Za-z]+)|([A-Za-z])", md):
        if num:
            for _ in range(int(num)):
                out.append(aligned[pos])
                pos += 1
        elif dele:
            for ch in dele:
                assert aligned[pos] is None, "MD deletion does not line up with the CIGAR"
                out.append(ord(ch))
                pos += 1
            edits += len(dele)
        else:
            out.append(ord(sub))
            pos += 1
            edits += 1
    assert pos == len(aligned) and None not in out, "MD does not cover the alignment"
    edits += sum(n for n, op in rec.cigar if op == "I")
    return bytes(out), edits


def bam_pairs(path, window=None, seed=7, min_mapq=0):
    """Realistic (target, query) pairs from a BAM with MD tags: query = the read as sequenced, target = the
    reference bases under it; with ``window`` the target is padded to that many bases with seeded random
    flanks (the read then sits at a random offset inside, as in BASELINE configs[1]).
    Returns (targets list of bytes, queries list of bytes, records used)."""
    rng = np.random.Generator(np.random.MT19937(seed))
    _, _, records = read_bam(path)
    ts, qs, used = [], [], []
    for rec in records:
        if rec.flag & 0x4 or rec.mapq < min_mapq:
            continue
        rebuilt = reference_under_read(rec)
        if rebuilt is None:
            continue
        ref = rebuilt[0]
        if window is not None:
            if len(ref) > window:
                continue
            pad = window - len(ref)
            left = int(rng.integers(0, pad + 1))
            flank = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=pad)].tobytes()
            ref = flank[:left] + ref + flank[left:]
        ts.append(ref)
        qs.append(rec.seq)
        used.append(rec)
    return ts, qs, used


# --------------------------------------------------------------------------------------------- SAM / PAF
def _targets(ref_name, ref_len):
    """-> ([names], [lengths], many): ``ref_name`` and ``ref_len`` as one reference sequence (a string and a number) or as lists of
    equal length, one entry per contig."""
    if isinstance(ref_name, (str, bytes)):
        return [ref_name.decode() if isinstance(ref_name, bytes) else ref_name], [int(ref_len)], False
    names, lens = list(ref_name), [int(x) for x in ref_len]
    if len(names) != len(lens) or not names:
        raise ValueError("ref_name and ref_len: lists of one length, one entry per contig")
    return names, lens, True


def _target_of(result, k, names, lens, many):
    """the (name, length) of the contig read ``k`` is mapped to: ``result.rid`` where the reference has contigs"""
    if not many:
        return names[0], lens[0]
    rid = getattr(result, "rid", None)
    if rid is None:
        raise ValueError("the result has no rid: map the reads against an index with contigs (build_index_contigs)")
    return names[int(rid[k])], lens[int(rid[k])]


def sam_header(ref_name, ref_len):
    """The header of a SAM file over one reference sequence, or -- ``ref_name`` and ``ref_len`` as lists -- over its contigs, one @SQ
    line each."""
    names, lens, _ = _targets(ref_name, ref_len)
    return "@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % x for x in zip(names, lens)) + "@PG\tID:mgl_amd\tPN:mgl_amd\n"


def _oriented(seq, strand):
    from . import synth

    return synth.revcomp(seq) if strand else bytes(seq)


def _mapped(result, k):
    return int(result.status[k]) == 0 and int(result.ref_end[k]) > int(result.ref_beg[k])


def _core_cigar(result, k, extended):
    if extended:
        if result.xcigars is None:
            raise ValueError("the result has no extended CIGARs: map_reads_described(..., extended=True)")
        return result.xcigars[k]
    return result.cigars[k]


def write_sam(path, ref_name, ref_len, names, reads, quals, result, extended=False):
    """One SAM line per read from a DescribedMapResult (MicrosoftSmithWaterman.map_reads_described).  ``reads``: the reads as they
    were given; ``quals``: their qualities as text (phred + 33), or None for ``*``.  A mapped read: FLAG 0 or 16, POS ref_beg + 1, the
    result's MAPQ, CIGAR = q_beg S, the core (the = / X form with ``extended``), (read length - q_end) S, SEQ the ORIENTED read (its
    reverse complement on strand 1, QUAL reversed with it), tags NM:i, MD:Z, AS:i.  An unmapped read: FLAG 4, ``*`` and 0, SEQ and
    QUAL as given.  ``ref_name`` and ``ref_len`` as lists (one entry per contig): RNAME is the contig ``result.rid`` names and POS counts
    from its start, as ``ref_beg`` of a result mapped against contigs does."""
    names_, lens_, many = _targets(ref_name, ref_len)
    with open(path, "wt") as f:
        f.write(sam_header(ref_name, ref_len))
        for k, (name, read) in enumerate(zip(names, reads)):
            read = bytes(read)
            qual = None if quals is None or quals[k] is None else (quals[k] if isinstance(quals[k], str) else bytes(quals[k]).decode())
            if not _mapped(result, k):
                f.write("\t".join([name, "4", "*", "0", "0", "*", "*", "0", "0", read.decode(), qual or "*"]) + "\n")
                continue
            strand, qb, qe = int(result.strand[k]), int(result.q_beg[k]), int(result.q_end[k])
            cigar = ("%dS" % qb if qb else "") + _core_cigar(result, k, extended) + ("%dS" % (len(read) - qe) if len(read) > qe else "")
            if qual is not None and strand:
                qual = qual[::-1]
            f.write("\t".join([name, "16" if strand else "0", _target_of(result, k, names_, lens_, many)[0], str(int(result.ref_beg[k]) + 1), str(int(result.mapq[k])), cigar, "*", "0", "0",
                               _oriented(read, strand).decode(), qual or "*", "NM:i:%d" % int(result.nm[k]), "MD:Z:" + bytes(result.md[k]).decode("latin-1"),
                               "AS:i:%d" % int(result.score[k])]) + "\n")


def write_paf(path, ref_name, ref_len, names, reads, result, extended=False):
    """One PAF line per MAPPED read from a DescribedMapResult: the twelve columns -- query name, length, start and end on the ORIGINAL
    strand ([ql - q_end, ql - q_beg) for strand 1), strand, target name, length, start, end, matching bases, block length, MAPQ --
    and the tags NM:i, AS:i and cg:Z: (the core CIGAR, without clips; the = / X form with ``extended``).  An unmapped read has no
    line.  ``ref_name`` and ``ref_len`` as lists (one entry per contig): the target's name and length are those of the contig
    ``result.rid`` names, start and end count from its start."""
    names_, lens_, many = _targets(ref_name, ref_len)
    with open(path, "wt") as f:
        for k, (name, read) in enumerate(zip(names, reads)):
            if not _mapped(result, k):
                continue
            tname, tlen = _target_of(result, k, names_, lens_, many)
            ql, strand, qb, qe = len(read), int(result.strand[k]), int(result.q_beg[k]), int(result.q_end[k])
            lo, hi = (ql - qe, ql - qb) if strand else (qb, qe)
            f.write("\t".join([name, str(ql), str(lo), str(hi), "-" if strand else "+", tname, str(tlen), str(int(result.ref_beg[k])),
                               str(int(result.ref_end[k])), str(int(result.n_match[k])), str(int(result.block_len[k])), str(int(result.mapq[k])),
                               "NM:i:%d" % int(result.nm[k]), "AS:i:%d" % int(result.score[k]), "cg:Z:" + _core_cigar(result, k, extended)]) + "\n")


def _line_cigar(line, ql, extended):
    """a line's CIGAR with its soft clips, over the oriented read"""
    if extended and line.xcigar is None:
        raise ValueError("the result has no extended CIGARs: map_reads_all(..., extended=True)")
    core = line.xcigar if extended else line.cigar
    return ("%dS" % line.q_beg if line.q_beg else "") + core + ("%dS" % (ql - line.q_end) if ql > line.q_end else "")


def _line_target(line, names, lens, many):
    if not many:
        return names[0], lens[0]
    if line.rid is None:
        raise ValueError("the result has no rid: map the reads against an index with contigs (build_index_contigs)")
    return names[int(line.rid)], lens[int(line.rid)]


def write_sam_all(path, ref_name, ref_len, names, reads, quals, result, extended=False):
    """One SAM line per Line of an AllMapResult (MicrosoftSmithWaterman.map_reads_all), in line order.  FLAG as classified: 0x10 on
    strand 1, 0x100 on a secondary and 0x800 on a supplementary line.  Every line carries the whole ORIENTED read (no hard clips): CIGAR
    = q_beg S, the core (the = / X form with ``extended``), (read length - q_end) S; SEQ its reverse complement on strand 1 and QUAL
    reversed with it.  Tags NM:i, MD:Z, AS:i and tp:A:P (tp:A:S on a secondary line); on each non-secondary line of a read that has
    at least two of them SA:Z: lists the OTHER non-secondary lines in line order, each as rname,pos,+|-,CIGAR with clips,mapq,NM;.
    A read without lines is written as ``write_sam`` writes an unmapped read.  ``ref_name`` and ``ref_len`` as in ``write_sam``."""
    names_, lens_, many = _targets(ref_name, ref_len)
    with open(path, "wt") as f:
        f.write(sam_header(ref_name, ref_len))
        for k, (name, read) in enumerate(zip(names, reads)):
            read = bytes(read)
            qual = None if quals is None or quals[k] is None else (quals[k] if isinstance(quals[k], str) else bytes(quals[k]).decode())
            lines = result.lines[k]
            if not lines:
                f.write("\t".join([name, "4", "*", "0", "0", "*", "*", "0", "0", read.decode(), qual or "*"]) + "\n")
                continue
            chief = [ln for ln in lines if not ln.flag & 0x100]
            sa = ["%s,%d,%s,%s,%d,%d;" % (_line_target(ln, names_, lens_, many)[0], ln.ref_beg + 1, "-" if ln.strand else "+", _line_cigar(ln, len(read), extended),
                                          ln.mapq, ln.nm) for ln in chief]
            for ln in lines:
                tags = ["NM:i:%d" % ln.nm, "MD:Z:" + bytes(ln.md).decode("latin-1"), "AS:i:%d" % ln.score, "tp:A:S" if ln.flag & 0x100 else "tp:A:P"]
                if not ln.flag & 0x100 and len(chief) >= 2:
                    tags.append("SA:Z:" + "".join(s for other, s in zip(chief, sa) if other is not ln))
                f.write("\t".join([name, str(ln.flag), _line_target(ln, names_, lens_, many)[0], str(ln.ref_beg + 1), str(ln.mapq), _line_cigar(ln, len(read), extended),
                                   "*", "0", "0", _oriented(read, ln.strand).decode(), (qual[::-1] if ln.strand else qual) if qual is not None else "*"] + tags) + "\n")


def write_paf_all(path, ref_name, ref_len, names, reads, result, extended=False):
    """One PAF line per Line of an AllMapResult, in line order: ``write_paf``'s twelve columns and tags, and tp:A:P or tp:A:S
    (secondary).  A read without lines has no line."""
    names_, lens_, many = _targets(ref_name, ref_len)
    with open(path, "wt") as f:
        for k, (name, read) in enumerate(zip(names, reads)):
            for ln in result.lines[k]:
                tname, tlen = _line_target(ln, names_, lens_, many)
                ql = len(read)
                lo, hi = (ql - ln.q_end, ql - ln.q_beg) if ln.strand else (ln.q_beg, ln.q_end)
                f.write("\t".join([name, str(ql), str(lo), str(hi), "-" if ln.strand else "+", tname, str(tlen), str(ln.ref_beg), str(ln.ref_end), str(ln.n_match),
                                   str(ln.block_len), str(ln.mapq), "NM:i:%d" % ln.nm, "AS:i:%d" % ln.score, "tp:A:S" if ln.flag & 0x100 else "tp:A:P",
                                   "cg:Z:" + (ln.xcigar if extended else ln.cigar)]) + "\n")


def read_sam(path):
    """A small SAM reader: (header text, [(reference name, length)], [BamRecord]) as ``read_bam`` gives them -- ``pos`` 0-based (-1
    for ``*``), ``cigar`` a list of (len, op), ``seq`` ASCII bytes, ``qual`` raw phred bytes (empty for ``*``), ``tags`` with i / f
    values converted -- so that ``reference_under_read`` works on the records."""
    header, refs, records = [], [], []
    with _open(path) as f:
        for line in f:
            line = line.rstrip("\r\n")
            if not line:
                continue
            if line.startswith("@"):
                header.append(line)
                if line.startswith("@SQ"):
                    kv = dict(x.split(":", 1) for x in line.split("\t")[1:])
                    refs.append((kv["SN"], int(kv["LN"])))
                continue
            c = line.split("\t")
            if len(c) < 11:
                raise ValueError("malformed SAM line %r" % line[:40])
            tags = {}
            for t in c[11:]:
                tag, ty, val = t.split(":", 2)
                tags[tag] = int(val) if ty == "i" else float(val) if ty == "f" else val
            names = [r[0] for r in refs]
            records.append(BamRecord(c[0], names.index(c[2]) if c[2] in names else -1, int(c[3]) - 1, int(c[1]), int(c[4]),
                                     [] if c[5] == "*" else cigar_text_to_elements(c[5]), b"" if c[9] == "*" else c[9].encode(),
                                     b"" if c[10] == "*" else bytes(ord(x) - 33 for x in c[10]), tags))
    return "\n".join(header) + ("\n" if header else ""), refs, records


def write_sites(path, ref_name, ref_len, sites, counts, starts=None):
    """One tab-separated line per candidate site of a pileup (MicrosoftSmithWaterman.pileup_sites_device, read back): contig, 1-based
    position, reference base, call, depth, the eight counts of the position (A C G T other, deleted, insertions, inserted bases) and
    the flags (1 covered, 2 SNV candidate, 4 deletion, 8 insertion behind the position).  ``sites``: rows of mgl_sw_site's eight
    fields, pos counted from the table's first position; ``counts``: the table [8, region_len].  ``ref_name`` and ``ref_len`` as
    ``write_sam`` takes them; as lists (one entry per contig) they want ``starts``, the contigs' first positions in the table, and a
    site's position counts from the start of its contig.  A list of candidates, no VCF: no genotype and no quality is claimed
    (``write_vcf`` writes the calls of ``map_reads_calls``)."""
    names, lens, many = _targets(ref_name, ref_len)
    if many and (starts is None or len(starts) != len(names)):
        raise ValueError("a reference of contigs wants starts: the first position of every contig")
    first = np.asarray(starts if many else [0], np.int64)
    counts = np.asarray(counts).reshape(8, -1)
    if counts.dtype == np.int32:  # (the device form's tensor carries the uint32 bits)
        counts = counts.view(np.uint32)
    with open(path, "wt") as f:
        f.write("#contig\tpos\tref\tcall\tdepth\tA\tC\tG\tT\tother\tdel\tins\tins_bases\tflags\n")
        for row in np.asarray(sites).reshape(-1, 8):
            pos, flags, depth, ref, call = (int(v) for v in row[:5])
            c = int(np.searchsorted(first, pos, side="right")) - 1
            if c < 0 or pos - int(first[c]) >= lens[c]:
                raise ValueError("site at %d lies in no contig" % pos)
            f.write("\t".join([names[c], str(pos - int(first[c]) + 1), "ACGTN"[ref], "ACGTN*"[call], str(depth)] + [str(int(v)) for v in counts[:, pos]] +
                              [str(flags)]) + "\n")


# --------------------------------------------------------------------------------------------- VCF
VcfRecord = namedtuple("VcfRecord", "chrom pos ref alt qual filter gt gq dp ad pl")
VcfRecord.__doc__ = "one line of read_vcf: pos counts from 0; ref and alt are bytes; gt is the text (0/1, 1/1); ad and pl are tuples"


def write_vcf(path, ref_name, ref_len, ref, calls, starts=None, min_qual=0, sample="sample"):
    """A VCFv4.2 file of one sample from the calls of ``MicrosoftSmithWaterman.map_reads_calls`` (``Call``: pos in the reference
    buffer ``ref``, kind, len, REF and ALT bases as the call changes them).  ``ref_name`` and ``ref_len`` as ``write_sam`` takes them;
    as lists (one entry per contig) they want ``starts``, the contigs' first positions in ``ref``.  A ##contig line per contig;
    FORMAT GT:GQ:DP:AD:PL.  An indel is anchored on the base in front of it, or on the base behind it at a contig's first position, as
    the specification says.  Calls with gt == 0 or qual < ``min_qual`` are left out; a deletion run cut at max_del (flag 1) gets
    FILTER LongDel, every other record PASS.  The genotypes are biallelic and unphased.  -> the number of records written."""
    names, lens, many = _targets(ref_name, ref_len)
    if many and (starts is None or len(starts) != len(names)):
        raise ValueError("a reference of contigs wants starts: the first position of every contig")
    first = [int(x) for x in (starts if many else [0])]

    def contig_of(pos):
        c = int(np.searchsorted(np.asarray(first, np.int64), pos, side="right")) - 1
        return c if c >= 0 and pos - first[c] < lens[c] else -1

    base = lambda at: bytes(ref[at:at + 1]).upper()  # noqa: E731
    lines = []
    for call in calls:
        if call.gt == 0 or call.qual < min_qual:
            continue
        pos = int(call.pos)
        c = contig_of(pos)
        if call.kind == 1:
            at, r, a = pos, bytes(call.ref), bytes(call.alt)
        elif call.kind == 2:
            if c >= 0 and pos > first[c]:
                at, r, a = pos - 1, base(pos - 1) + bytes(call.ref), base(pos - 1)
            else:                                                   # a contig's first base is deleted: the base behind
                behind = base(pos + len(call.ref))
                at, r, a = pos, bytes(call.ref) + behind, behind
        elif c >= 0:
            at, r, a = pos, base(pos), base(pos) + bytes(call.alt)
        else:                                                       # inserted in front of a contig's first base: the base behind
            c = contig_of(pos + 1)
            if c < 0 or first[c] != pos + 1:
                raise ValueError("insertion behind %d lies in no contig" % pos)
            at, r, a = pos + 1, base(pos + 1), bytes(call.alt) + base(pos + 1)
        if c < 0:
            raise ValueError("call at %d lies in no contig" % pos)
        fields = [names[c], str(at - first[c] + 1), ".", r.upper().decode(), a.upper().decode(), str(int(call.qual)), "LongDel" if call.flags & 1 else "PASS",
                  ".", "GT:GQ:DP:AD:PL", "%s:%d:%d:%d,%d:%d,%d,%d" % ("0/1" if call.gt == 1 else "1/1", call.gq, call.depth, call.ref_count, call.alt_count,
                                                                     *call.pl)]
        lines.append((c, at, len(lines), "\t".join(fields)))
    with open(path, "wt") as f:
        f.write("##fileformat=VCFv4.2\n##source=mgl_amd\n")
        f.write("".join("##contig=<ID=%s,length=%d>\n" % x for x in zip(names, lens)))
        f.write('##FILTER=<ID=PASS,Description="All filters passed">\n')
        f.write('##FILTER=<ID=LongDel,Description="The run of deleted positions goes on beyond max_del">\n')
        f.write('##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n')
        f.write('##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Genotype quality: the smaller PL of the other two genotypes, at most 99">\n')
        f.write('##FORMAT=<ID=DP,Number=1,Type=Integer,Description="Depth at the position: bases and deleted columns">\n')
        f.write('##FORMAT=<ID=AD,Number=R,Type=Integer,Description="Reads for the reference and for the alternate allele">\n')
        f.write('##FORMAT=<ID=PL,Number=G,Type=Integer,Description="Phred-scaled genotype likelihoods from integer costs per read">\n')
        f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t%s\n" % sample)
        for _, _, _, text in sorted(lines):
            f.write(text + "\n")
    return len(lines)


def read_vcf(path):
    """-> (the header lines, without their newline; [VcfRecord]) of a one-sample file as ``write_vcf`` writes it"""
    header, records = [], []
    with _open(path) as f:
        for line in f:
            line = line.rstrip("\n")
            if line.startswith("#"):
                header.append(line)
                continue
            if not line:
                continue
            c = line.split("\t")
            sample = dict(zip(c[8].split(":"), c[9].split(":")))
            ints = lambda x: tuple(int(v) for v in x.split(","))  # noqa: E731
            records.append(VcfRecord(c[0], int(c[1]) - 1, c[3].encode(), c[4].encode(), int(c[5]), c[6], sample["GT"], int(sample["GQ"]), int(sample["DP"]),
                                     ints(sample["AD"]), ints(sample["PL"])))
    return header, records
