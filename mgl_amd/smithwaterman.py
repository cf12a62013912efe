"""Host-side mirror of the reference's Smith-Waterman operator interface, over the C ABI.

The reference's entry point is ``MicrosoftSmithWaterman.align(ref, alt, parameters,
overhangStrategy) -> SWNativeAlignerResult(cigar, alignment_offset)``
(src/main/java/com/microsoft/mgl/smithwaterman/MicrosoftSmithWaterman.java:66-86) on top of
``align_avx`` / ``align_scalar`` (src/main/native/mgl_sw/sw_avx.h:6, sw_scalar.h:9).  The
names, argument meaning and the (cigar, offset) result are kept; a batch form is added because
one pair per launch cannot feed a GPU.  All arithmetic happens in libmgl_sw_hip.so.
"""
import ctypes as C
from collections import namedtuple
from enum import IntEnum

import numpy as np

from . import _lib


class SWOverhangStrategy(IntEnum):
    """org.broadinstitute.gatk.nativebindings SWOverhangStrategy -> sw_common.h:22-25 codes
    (the mapping of MicrosoftSmithWaterman.java:39-56)."""
    SOFTCLIP = 0x01
    INDEL = 0x02
    LEADING_INDEL = 0x04
    IGNORE = 0x08


SWParameters = namedtuple("SWParameters", "match mismatch gap_open gap_extend")
SWParameters.__doc__ = "swParameters (sw_common.h:42-47); any sign convention, normalised natively"

# GATK's NEW_SW_PARAMETERS, the set the reference is exercised with
GATK_PARAMETERS = SWParameters(200, -150, -260, -11)

SWNativeAlignerResult = namedtuple("SWNativeAlignerResult", "cigar alignment_offset")
ScoreMax = namedtuple("ScoreMax", "mqe mqe_t max max_t max_q seg_length")

BatchResult = namedtuple("BatchResult", "offsets scores cigars cigar_len")
ExtendResult = namedtuple("ExtendResult", "score t_end q_end score_qend t_end_qend rows_done dropped cigar_from cigars cigar_len")
SeedExtendResult = namedtuple("SeedExtendResult", "score t_beg t_end q_beg q_end seed_score dropped cigar_from cigars cigar_len")
ChainAlignResult = namedtuple("ChainAlignResult", "score t_beg t_end q_beg q_end anchor_score dropped cigar_from cigars cigar_len")
ChainAnchorsResult = namedtuple("ChainAnchorsResult", "chains score status")
SeedResult = namedtuple("SeedResult", "candidates status")
MapResult = namedtuple("MapResult", "ref_beg ref_end strand score cigars status")
RankedMapResult = namedtuple("RankedMapResult", "ref_beg ref_end strand score cigars status mapq n_chains secondary")
DescribedMapResult = namedtuple("DescribedMapResult", "ref_beg ref_end strand score cigars status mapq n_chains secondary q_beg q_end nm n_match block_len md "
                                "xcigars")
AlignmentStats = namedtuple("AlignmentStats", "n_match n_mismatch n_ins n_del n_ins_runs n_del_runs md_len xcigar_len")
RankedChain = namedtuple("RankedChain", "score strand n_anchors t_beg t_end q_beg q_end parent n_sub subsc mapq end_index")
Line = namedtuple("Line", "ref_beg ref_end strand score cigar q_beg q_end flag mapq parent nm n_match block_len md xcigar rid rname status")
AllMapResult = namedtuple("AllMapResult", "n_lines lines")
Call = namedtuple("Call", "pos kind len ref alt depth ref_count alt_count gt gq qual pl flags")
Call.__doc__ = ("one variant call (map_reads_calls): pos counts from 0 in the reference buffer; kind 1 SNV (ref and alt one base each), 2 deletion (ref the "
                "deleted bases from pos on, alt empty), 3 insertion (ref empty, alt the inserted bases, which stand BEHIND pos); gt 0 = 0/0, 1 = 0/1, "
                "2 = 1/1; pl = (PL0, PL1, PL2); flags 1: the deletion run was cut at max_del")
GenotypeCosts = namedtuple("GenotypeCosts", "cost_match cost_error cost_het")
IndexInfo = namedtuple("IndexInfo", "ref_len entries bytes k w")
ContigTable = namedtuple("ContigTable", "names starts lens")
ContigTable.__doc__ = "the contigs of an Index: names (a list of str), starts and lens (int64 arrays) in the reference buffer's coordinates"
# the list results of the mappers against an index with contigs: ref_beg / ref_end count from the start of contig ``rid`` (-1 and None
# for an unmapped read), whose name is ``rname``
ContigMapResult = namedtuple("ContigMapResult", MapResult._fields + ("rid", "rname"))
ContigRankedMapResult = namedtuple("ContigRankedMapResult", RankedMapResult._fields + ("rid", "rname"))
ContigDescribedMapResult = namedtuple("ContigDescribedMapResult", DescribedMapResult._fields + ("rid", "rname"))


def genotype_costs(error_phred=20):
    """The three integer costs of mgl_sw_genotype_sites_device, in 1/256 phred per read, for a per-base error of phred
    ``error_phred``: what a read costs under a genotype it agrees with (cost_match), under one it contradicts (cost_error: the error
    lands on ONE of the three other bases) and under a heterozygous one (cost_het).  For 20: (11, 6341, 778).  The device sees these
    integers only; tests/calls_textbook.py takes them from here."""
    import math

    e = 10 ** (-error_phred / 10)
    return GenotypeCosts(max(1, round(-2560 * math.log10(1 - e))), round(-2560 * math.log10(e / 3)), round(-2560 * math.log10((1 - e) / 2 + e / 6)))


def _counted_lines(lines, min_mapq):
    """the pileup's select, made on the device from the classify stage's line rows: a job is counted where it is a line (order >= 0), not
    a secondary one (flag & 0x100 == 0) and its mapq is at least ``min_mapq``"""
    return ((lines[:, 0] >= 0) & ((lines[:, 1] & 0x100) == 0) & (lines[:, 2] >= int(min_mapq))).to(lines.dtype)


def _entry_costs(costs, error_phred):
    """-> (cost_match, cost_het, cost_error) as the entry takes them: ``costs`` in that order, or genotype_costs(error_phred)"""
    if costs is None:
        c = genotype_costs(error_phred)
        return c.cost_match, c.cost_het, c.cost_error
    if isinstance(costs, GenotypeCosts):
        return costs.cost_match, costs.cost_het, costs.cost_error
    return tuple(int(c) for c in costs)


def make_call(row, seq, ref, region_beg=0):
    """mgl_sw_call's sixteen fields, the call's sequence row and the reference buffer -> Call"""
    pos, kind, n, _, alt, depth, rc, ac, gt, gq, qual, pl0, pl1, pl2, flags = (int(v) for v in row[:15])
    at = region_beg + pos
    if kind == 1:
        ra = bytes(ref[at:at + 1]), b"ACGTN"[alt:alt + 1]
    elif kind == 2:
        ra = bytes(ref[at:at + n]), b""
    else:
        ra = b"", bytes(bytearray(int(b) for b in seq[:n]))
    return Call(pos, kind, n, ra[0], ra[1], depth, rc, ac, gt, gq, qual, (pl0, pl1, pl2), flags)


class Index:
    """A minimizer index of one reference on the device (mgl_sw_index, include/mgl_sw.h; ``MicrosoftSmithWaterman.build_index``
    makes it).  It owns the native handle and keeps ``ref``, the reference's device tensor, which the index itself does not.
    ``contigs``: a ContigTable where ``build_index_contigs`` made it, None for an index of one sequence -- the mappers go through the
    contig stages where there is one."""

    def __init__(self, handle, ref, contigs=None, owner=None):
        self.handle, self.ref, self.contigs, self._owner = handle, ref, contigs, owner

    def get_contigs(self):
        """mgl_sw_index_get_contigs -> (starts, lens) int64 arrays; an index of one sequence reports one contig [0, ref_len)"""
        n = C.c_int64()
        _check(_lib.lib().mgl_sw_index_get_contigs(self.handle, 0, None, None, C.byref(n)))
        starts, lens = np.zeros(n.value, np.int64), np.zeros(n.value, np.int64)
        _check(_lib.lib().mgl_sw_index_get_contigs(self.handle, n.value, starts.ctypes.data, lens.ctypes.data, C.byref(n)))
        return starts, lens

    def contig_of_device(self, t, l, out=None):
        """mgl_sw_index_contig_of_batch_device on int32 device tensors: per anchor the contig that holds [t, t + l) whole, -1 where
        none does (tests/contig_textbook.py); enqueued on the current stream, not synchronised.  -> group (int32, as ``t``), which
        ``chain_anchors_device(group=...)`` takes; ``out``: a tensor to write into."""
        import torch

        ctx = self._owner._ensure()
        total = int(t.numel())
        if out is None:
            out = torch.empty(total, dtype=torch.int32, device=t.device)
        assert l.numel() >= total and out.numel() >= total
        ptr = _ptrs(t.device)
        _check(_lib.lib().mgl_sw_index_contig_of_batch_device(ctx, torch.cuda.current_stream(t.device).cuda_stream, self.handle, total, ptr(t), ptr(l),
                                                              ptr(out)), ctx)
        return out

    @property
    def info(self):
        out = _lib.IndexInfo()
        _check(_lib.lib().mgl_sw_index_get_info(self.handle, C.byref(out)))
        return IndexInfo(out.ref_len, out.entries, out.bytes, out.k, out.w)

    def export(self):
        """-> (keys uint32 [M], positions int32 [M]) tensors, ascending by (key, position); enqueued on the current stream"""
        import torch

        m = self.info.entries
        new, ptr = _alloc(self.ref.device), _ptrs(self.ref.device)
        keys, pos = new(m), new(m)
        _check(_lib.lib().mgl_sw_index_export_device(self.handle, torch.cuda.current_stream(self.ref.device).cuda_stream, ptr(keys), ptr(pos), m))
        return keys.view(torch.uint32), pos

    def close(self):
        if self.handle is not None:
            _lib.lib().mgl_sw_index_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CigarColumn:
    """The CIGAR texts of a batch, decoded on access (a 10 M-pair batch would otherwise spend ten times the
    alignment time building Python strings).  Behaves like a read-only list of str."""

    def __init__(self, slots, lengths):
        self.slots, self.lengths = slots, lengths      # uint8 [n, stride], int32 [n]

    def __len__(self):
        return len(self.lengths)

    def __getitem__(self, k):
        if isinstance(k, slice):
            return [self[i] for i in range(*k.indices(len(self)))]
        if k < 0:
            k += len(self)
        return self.slots[k, : self.lengths[k]].tobytes().decode()

    def __iter__(self):
        return (self[k] for k in range(len(self)))

    def __eq__(self, other):
        try:
            return len(self) == len(other) and all(a == b for a, b in zip(self, other))
        except TypeError:
            return NotImplemented

    def __repr__(self):
        return "CigarColumn(%r)" % (self[:8] + (["..."] if len(self) > 8 else []),)


def _check(rc, ctx=None):
    if rc != _lib.OK:
        detail = _lib.lib().mgl_sw_last_error(ctx).decode() if ctx else ""
        raise _lib.MglSwError(rc, detail)


def concat(seqs):
    """list of bytes -> (uint8 array, int64 offsets[n+1])"""
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    if seqs:
        np.cumsum([len(s) for s in seqs], out=off[1:])
    data = np.frombuffer(b"".join(seqs), dtype=np.uint8).copy()
    return data, off


def _default_stride(max_tl, max_ql, binary_cigar):
    return max(16, 2 * max(max_tl, max_ql)) * (4 if binary_cigar else 1)


def _pack_pairs(refs, alts, dev, cigar_stride, binary_cigar):
    """Lists of byte strings -> (n, the six device tensors and two bounds the *_device forms take, cigar_stride)."""
    ts, qs = [bytes(x) for x in refs], [bytes(x) for x in alts]
    assert len(qs) == len(ts)
    td, toff = concat(ts)
    qd, qoff = concat(qs)
    g = lambda x: _upload(x, dev)  # noqa: E731
    tlen, qlen = np.diff(toff).astype(np.int32), np.diff(qoff).astype(np.int32)
    max_tl, max_ql = int(tlen.max(initial=1)), int(qlen.max(initial=1))
    if cigar_stride is None:
        cigar_stride = _default_stride(max_tl, max_ql, binary_cigar)
    pad = np.zeros(8, np.uint8)
    return len(ts), (g(np.concatenate([td, pad])), g(toff[:-1]), g(tlen), g(np.concatenate([qd, pad])), g(qoff[:-1]), g(qlen), max_tl, max_ql), cigar_stride


def _fetch(out, dev, return_status):
    """The device form's output tensors as numpy arrays, once the stream is done; a pair's status raises unless it is asked for."""
    import torch

    torch.cuda.synchronize(dev)
    out = [None if x is None else x.cpu().numpy() for x in out]
    st = out[-1]
    if not return_status and st.any():
        k = int(np.flatnonzero(st)[0])
        raise _lib.MglSwError(int(st[k]), f"pair {k}")
    return out


def _ptrs(dev, keep_null=False):
    """-> ptr(x): the address of tensor ``x`` as a C entry takes it, None for None.  An empty tensor has no address and the entries
    want one: it gets that of a spare tensor on ``dev``, made when the first empty one is met.  ``keep_null``: the older forms
    (banded, extend, extend_seed, align_chain) pass an empty tensor's null address on as it is."""
    if keep_null:
        return lambda x: None if x is None else x.data_ptr()
    spare = None

    def spare_ptr():
        nonlocal spare
        if spare is None:
            import torch

            spare = torch.empty(2, dtype=torch.int64, device=dev)
        return spare.data_ptr()

    return lambda x: None if x is None else (x.data_ptr() or spare_ptr())  # (the expression the entries are called through)


def _alloc(dev):
    """-> new(shape, dtype=torch.int32): an uninitialised output tensor on ``dev``."""
    import torch

    return lambda shape, dtype=torch.int32: torch.empty(shape, dtype=dtype, device=dev)


def _upload(x, dev, dtype=None):
    """A host array (or list) as a contiguous tensor on ``dev``."""
    import torch

    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=dtype))).to(dev)


def _extend_flags(binary_cigar, score_only, to_query_end=False, adaptive_band=False):
    return ((_lib.FLAG_BINARY_CIGAR if binary_cigar else 0) | (_lib.FLAG_SCORE_ONLY if score_only else 0) |
            (_lib.FLAG_EXTEND_TO_QUERY_END if to_query_end else 0) | (_lib.FLAG_EXTEND_ADAPTIVE_BAND if adaptive_band else 0))


def _csr(lists):
    """Ragged lists of (t, q, l) -> (start int64 [len + 1], flat int32 [total, 3]): the CSR layout the stages take."""
    start = np.zeros(len(lists) + 1, np.int64)
    if lists:
        np.cumsum([len(c) for c in lists], out=start[1:])
    return start, np.asarray([a for c in lists for a in c], dtype=np.int32).reshape(-1, 3)


def _candidate_lists(start, t, q, l, rows):
    """The CSR arrays a stage wrote -> per row its list of (t, q, l)."""
    return [[(int(t[i]), int(q[i]), int(l[i])) for i in range(start[r], start[r + 1])] for r in range(rows)]


def _seed_rows(out, rows, cand_capacity, dev):
    """The tuple of the seed stages that work on rows -- (cand_start [rows + 1] int64, cand_t, cand_q, cand_len [cand_capacity],
    row_t_len, row_q_len, status [rows] int32; the last three may be None in a caller's) --, made where ``out`` is None, and checked."""
    import torch

    if out is None:
        new = _alloc(dev)
        out = (new(rows + 1, torch.int64), new(cand_capacity), new(cand_capacity), new(cand_capacity), new(rows), new(rows), new(rows))
    cs, ct, cq, cl, rt, rq, st = out
    assert min(ct.numel(), cq.numel(), cl.numel()) >= cand_capacity and cs.numel() >= rows + 1
    assert all(x is None or x.numel() >= rows for x in (rt, rq, st))
    return out


def _pack_reads(reads, dev):
    """A list of byte strings -> (n, the (queries, q_start, q_len) device tensors, the longest read)."""
    qs = [bytes(q) for q in reads]
    n, packed, _ = _pack_pairs(qs, qs, dev, 16, False)
    return n, packed[3:6], packed[7]


def _map_setup(reads, dev, slack, max_tl, stages):
    """What the list-form mappers do before their device form: -> (n, the reads' tensors, max_tl, max_ql, the CIGAR stride, which
    leaves ``stages``).  ``max_tl`` defaults to 1.5 times the longest read and the slack to either side."""
    n, packed, max_ql = _pack_reads(reads, dev)
    if max_tl is None:
        max_tl = max_ql + max_ql // 2 + 2 * int(slack)
    stride = stages.pop("cigar_stride", None) or _default_stride(max_tl, max_ql, False)
    return n, packed, max_tl, max_ql, stride


def _contig_fields(index, window, ok):
    """-> (rid [n] with -1 for a read that is not ``ok``, rname, the start of every read's contig) from a window tuple with rid"""
    rid = np.where(ok, window[4].cpu().numpy(), -1).astype(np.int32)
    return rid, [index.contigs.names[c] if c >= 0 else None for c in rid], np.where(rid >= 0, index.contigs.starts[np.maximum(rid, 0)], 0)


def _contig_secondary(index, secondary):
    """the ranked chains behind the first with their contig, found from ref_beg on the host: (ref_beg, ref_end, strand, score, parent,
    rid), ref_beg and ref_end from that contig's start"""
    starts = index.contigs.starts
    out = []
    for chains in secondary:
        rids = [int(np.searchsorted(starts, c[0], side="right")) - 1 for c in chains]
        out.append([(c[0] - int(starts[r]), c[1] - int(starts[r])) + tuple(c[2:]) + (r,) for c, r in zip(chains, rids)])
    return out


def _map_fields(n, stride, chosen, window, aln, index=None):
    """The device tuples of a mapper, read back (the stream is done) -> (MapResult's six fields, ok, the alignments' records, the
    contig fields): a read whose alignment has a status has zeros and an empty CIGAR, and the window's status where that refused the
    read.  With an ``index`` that has contigs ref_beg and ref_end count from the start of the read's contig and the contig fields
    are (rid, rname); otherwise they are ()."""
    rec, cg, ln, st = aln[0].cpu().numpy(), aln[4].cpu().numpy().reshape(n, stride), aln[5].cpu().numpy(), aln[6].cpu().numpy()
    t_start, wst = window[0].cpu().numpy(), window[3].cpu().numpy()
    ok = st == 0
    contig = ()
    if index is not None and index.contigs is not None:
        rid, rname, origin = _contig_fields(index, window, ok)
        t_start, contig = t_start - origin, (rid, rname)
    strand = chosen[0].cpu().numpy() if chosen is not None else np.zeros(n, np.int32)
    ln = np.where(ok, ln, 0).astype(np.int32)
    fields = (np.where(ok, t_start + rec[:, 1], 0), np.where(ok, t_start + rec[:, 2], 0), np.where(ok, strand, 0).astype(np.int32),
              np.where(ok, rec[:, 0], 0).astype(np.int32), CigarColumn(cg, ln), np.where(wst != 0, wst, st).astype(np.int32))
    return fields, ok, rec, contig


def _rank_fields(n, ranked):
    """The ranking's device tuple, read back -> (mapq, n_chains, secondary) as RankedMapResult has them."""
    nc, rr = ranked[0].cpu().numpy(), ranked[1].cpu().numpy()
    mapq = np.asarray([int(rr[p, 0, 10]) if nc[p] > 0 else 0 for p in range(n)], dtype=np.int32)
    secondary = [[(int(c[3]), int(c[4]), int(c[1]), int(c[0]), int(c[7])) for c in rr[p, 1:nc[p]]] for p in range(n)]
    return mapq, nc.astype(np.int32), secondary


class MicrosoftSmithWaterman:
    """Drop-in for the reference's SWAlignerNativeBinding implementation.

    ``load()`` / ``align()`` / ``close()`` follow MicrosoftSmithWaterman.java:35,66,89.
    One instance owns one GPU context; instances may be used from different threads.
    """

    def __init__(self, device=0):
        self._device = device
        self._ctx = None

    # -- SWAlignerNativeBinding ------------------------------------------------------------
    def load(self, temp_dir=None):
        """True when the native library is present and a GPU context could be made
        (the reference returns False when the library cannot be used, .java:27-37)."""
        try:
            self._ensure()
            return True
        except (OSError, _lib.MglSwError):
            return False

    def align(self, ref, alt, parameters=GATK_PARAMETERS, overhang_strategy=SWOverhangStrategy.SOFTCLIP):
        ref, alt = bytes(ref), bytes(alt)
        # the Java side allocates 2*max(refLength, altLength) CIGAR bytes (.java:71)
        cap = max(16, 2 * max(len(ref), len(alt)))
        res = self.align_batch([ref], [alt], parameters, overhang_strategy, cigar_stride=cap)
        return SWNativeAlignerResult(res.cigars[0], int(res.offsets[0]))

    def close(self):
        if self._ctx is not None:
            _lib.lib().mgl_sw_ctx_destroy(self._ctx)
            self._ctx = None

    # -- batch form ------------------------------------------------------------------------
    def align_batch(self, refs, alts, parameters=GATK_PARAMETERS, overhang_strategy=SWOverhangStrategy.SOFTCLIP,
                    cigar_stride=None):
        """Align refs[k] against alts[k] for every k; returns BatchResult with numpy arrays."""
        td, toff = concat([bytes(x) for x in refs])
        qd, qoff = concat([bytes(x) for x in alts])
        return self.align_packed(td, toff, qd, qoff, parameters, overhang_strategy, cigar_stride)

    def align_packed(self, targets, t_off, queries, q_off, parameters=GATK_PARAMETERS,
                     overhang_strategy=SWOverhangStrategy.SOFTCLIP, cigar_stride=None):
        """Concatenated-bytes form of align_batch (what mgl_sw_align_batch takes)."""
        ctx = self._ensure()
        n = len(t_off) - 1
        assert len(q_off) - 1 == n
        targets = np.ascontiguousarray(targets, dtype=np.uint8)
        queries = np.ascontiguousarray(queries, dtype=np.uint8)
        t_off = np.ascontiguousarray(t_off, dtype=np.int64)
        q_off = np.ascontiguousarray(q_off, dtype=np.int64)
        if cigar_stride is None:
            longest = int(max(np.diff(t_off).max(initial=1), np.diff(q_off).max(initial=1)))
            cigar_stride = max(16, 2 * longest)
        off = np.empty(n, np.int32)
        sc = np.empty((n, 6), np.int32)
        cg = np.empty(n * cigar_stride, np.uint8)
        ln = np.empty(n, np.int32)
        p = SWParameters(*parameters)
        rc = _lib.lib().mgl_sw_align_batch(ctx, n, targets.ctypes.data, t_off.ctypes.data, queries.ctypes.data,
                                           q_off.ctypes.data, p.match, p.mismatch, p.gap_open, p.gap_extend,
                                           int(overhang_strategy), off.ctypes.data, sc.ctypes.data, cg.ctypes.data,
                                           cigar_stride, ln.ctypes.data)
        _check(rc, ctx)
        return BatchResult(off, sc, CigarColumn(cg.reshape(n, cigar_stride), ln), ln)

    def align_banded(self, refs, alts, band, parameters=GATK_PARAMETERS, overhang_strategy=SWOverhangStrategy.SOFTCLIP, cigar_stride=None,
                     binary_cigar=False, score_only=False, return_status=False):
        """mgl_sw_align_batch_device_banded over lists of byte strings: the alignment of refs[k] against alts[k] computed over the cells
        within ``band`` of the main diagonal only (lo = min(0, ql - tl) - band <= j - i <= max(0, ql - tl) + band).  NOT a reference
        function: a band that holds a pair's full-matrix path gives the full-matrix offset and CIGAR, a narrower one need not.  Returns
        what align_batch returns (with ``return_status`` the per-pair status array as well, and no exception for a pair's status)."""
        import torch

        dev = torch.device("cuda", self._device)
        n, packed, cigar_stride = _pack_pairs(refs, alts, dev, cigar_stride, binary_cigar)
        out = self.align_banded_device(*packed, band, parameters, overhang_strategy, cigar_stride, binary_cigar, score_only)
        off, sc, cg, ln, st = _fetch(out, dev, return_status)
        if score_only:
            res = BatchResult(off, sc, None, None)
        else:
            res = BatchResult(off, sc, CigarColumn(cg.reshape(n, cigar_stride), ln), ln)
        return (res, st) if return_status else res

    def align_banded_device(self, targets, t_start, t_len, queries, q_start, q_len, max_tl, max_ql, band, parameters=GATK_PARAMETERS,
                            overhang_strategy=SWOverhangStrategy.SOFTCLIP, cigar_stride=None, binary_cigar=False, score_only=False, out=None):
        """The device-tensor form: torch tensors on this context's GPU (uint8 bytes, int64 starts, int32 lengths); enqueued on the current
        stream, not synchronised.  Returns (offsets, scores[n, 6], cigar bytes[n * stride] or None, cigar lengths or None, status)
        tensors; ``out``: such a tuple to write into."""
        import torch

        ctx = self._ensure()
        n = int(t_start.numel())
        dev = targets.device
        if cigar_stride is None:
            cigar_stride = _default_stride(max_tl, max_ql, binary_cigar)
        if out is None:
            new = _alloc(dev)
            out = (new(n), new((n, 6)), None if score_only else new(n * cigar_stride, torch.uint8), None if score_only else new(n), new(n))
        off, sc, cg, ln, st = out
        p = SWParameters(*parameters)
        flags = _extend_flags(binary_cigar, score_only)
        ptr = _ptrs(dev, keep_null=True)
        rc = _lib.lib().mgl_sw_align_batch_device_banded(
            ctx, torch.cuda.current_stream(dev).cuda_stream, n, ptr(targets), ptr(t_start), ptr(t_len), ptr(queries), ptr(q_start), ptr(q_len),
            int(max_tl), int(max_ql), p.match, p.mismatch, p.gap_open, p.gap_extend, int(overhang_strategy), int(band), ptr(off), ptr(sc), ptr(cg),
            int(cigar_stride), ptr(ln), ptr(st), flags)
        _check(rc, ctx)
        return out

    def extend(self, refs, alts, band, zdrop, parameters=GATK_PARAMETERS, to_query_end=False, cigar_stride=None, binary_cigar=False,
               score_only=False, return_status=False, adaptive_band=False):
        """mgl_sw_extend_batch_device over lists of byte strings: the extension of alts[k] along refs[k] from the anchored start (0, 0)
        to a free end, over the cells with -band <= j - i <= band, stopped by the Z-drop rule (``zdrop`` < 0: off).  NOT a reference
        function.  ``adaptive_band``: the band is re-centred every 64 target rows on the diagonal of the row maximum
        (MGL_SW_FLAG_EXTEND_ADAPTIVE_BAND), so ``band`` need only cover the largest indel between two re-centrings.  Returns
        ExtendResult: the eight fields of mgl_sw_extension as arrays, the CIGARs and their lengths (with ``return_status`` the per-pair
        status array as well, and no exception for a pair's status)."""
        import torch

        dev = torch.device("cuda", self._device)
        n, packed, cigar_stride = _pack_pairs(refs, alts, dev, cigar_stride, binary_cigar)
        out = self.extend_device(*packed, band, zdrop, parameters, to_query_end, cigar_stride, binary_cigar, score_only,
                                 adaptive_band=adaptive_band)
        ext, cg, ln, st = _fetch(out, dev, return_status)
        fields = [ext[:, c] for c in range(8)]
        res = ExtendResult(*fields, None, None) if score_only else ExtendResult(*fields, CigarColumn(cg.reshape(n, cigar_stride), ln), ln)
        return (res, st) if return_status else res

    def extend_device(self, targets, t_start, t_len, queries, q_start, q_len, max_tl, max_ql, band, zdrop, parameters=GATK_PARAMETERS,
                      to_query_end=False, cigar_stride=None, binary_cigar=False, score_only=False, out=None, adaptive_band=False):
        """The device-tensor form: torch tensors on this context's GPU (uint8 bytes, int64 starts, int32 lengths); enqueued on the current
        stream, not synchronised.  Returns (extensions[n, 8], cigar bytes[n * stride] or None, cigar lengths or None, status) tensors;
        ``out``: such a tuple to write into."""
        import torch

        ctx = self._ensure()
        n = int(t_start.numel())
        dev = targets.device
        if cigar_stride is None:
            cigar_stride = _default_stride(max_tl, max_ql, binary_cigar)
        if out is None:
            new = _alloc(dev)
            out = (new((n, 8)), None if score_only else new(n * cigar_stride, torch.uint8), None if score_only else new(n), new(n))
        ext, cg, ln, st = out
        p = SWParameters(*parameters)
        flags = _extend_flags(binary_cigar, score_only, to_query_end, adaptive_band)
        ptr = _ptrs(dev, keep_null=True)
        rc = _lib.lib().mgl_sw_extend_batch_device(
            ctx, torch.cuda.current_stream(dev).cuda_stream, n, ptr(targets), ptr(t_start), ptr(t_len), ptr(queries), ptr(q_start), ptr(q_len),
            int(max_tl), int(max_ql), p.match, p.mismatch, p.gap_open, p.gap_extend, int(band), int(zdrop), ptr(ext), ptr(cg), int(cigar_stride),
            ptr(ln), ptr(st), flags)
        _check(rc, ctx)
        return out

    def extend_seed(self, refs, alts, seeds, band, zdrop, parameters=GATK_PARAMETERS, to_query_end=False, cigar_stride=None, binary_cigar=False,
                    score_only=False, return_status=False, adaptive_band=False, return_sides=False):
        """mgl_sw_extend_seed_batch_device over lists of byte strings: ``seeds[k]`` = (st, sq, sl) lays refs[k][st:st + sl] against
        alts[k][sq:sq + sl]; the seed is extended to the right and -- on the reversed flanks -- to the left with the function of
        ``extend`` (same band, zdrop and options on each side), and the two sides are joined across the seed into one alignment on the
        device.  NOT a reference function.  Returns SeedExtendResult: the eight fields of mgl_sw_seed_alignment as arrays (spans half
        open, in the coordinates of refs[k] and alts[k]), the joined CIGARs (M / I / D, no clips) and their lengths; with
        ``return_sides`` also the two sides' records as int32 arrays [n, 8] (mgl_sw_extension, in flank coordinates), with
        ``return_status`` the per-pair status array (and no exception for a pair's status): (result[, left, right][, status])."""
        import torch

        dev = torch.device("cuda", self._device)
        n, packed, cigar_stride = _pack_pairs(refs, alts, dev, cigar_stride, binary_cigar)
        sd = np.ascontiguousarray(np.asarray(seeds, dtype=np.int32).reshape(n, 3).T)
        seed_t, seed_q, seed_len = (_upload(sd[c], dev) for c in range(3))
        out = self.extend_seed_device(*packed[:6], seed_t, seed_q, seed_len, *packed[6:], band, zdrop, parameters, to_query_end, cigar_stride,
                                      binary_cigar, score_only, adaptive_band=adaptive_band, sides=return_sides)
        aln, left, right, cg, ln, st = _fetch(out, dev, return_status)
        fields = [aln[:, c] for c in range(8)]
        res = SeedExtendResult(*fields, None, None) if score_only else SeedExtendResult(*fields, CigarColumn(cg.reshape(n, cigar_stride), ln), ln)
        ret = (res,) + ((left, right) if return_sides else ()) + ((st,) if return_status else ())
        return ret if len(ret) > 1 else res

    def extend_seed_device(self, targets, t_start, t_len, queries, q_start, q_len, seed_t, seed_q, seed_len, max_tl, max_ql, band, zdrop,
                           parameters=GATK_PARAMETERS, to_query_end=False, cigar_stride=None, binary_cigar=False, score_only=False, out=None,
                           adaptive_band=False, sides=False):
        """The device-tensor form: torch tensors on this context's GPU (uint8 bytes, int64 starts, int32 lengths and seeds); enqueued on
        the current stream, not synchronised.  Returns (alignments[n, 8], left[n, 8] or None, right[n, 8] or None, cigar bytes
        [n * stride] or None, cigar lengths or None, status) tensors -- the side records with ``sides`` --; ``out``: such a tuple to
        write into."""
        import torch

        ctx = self._ensure()
        n = int(t_start.numel())
        dev = targets.device
        if cigar_stride is None:
            cigar_stride = _default_stride(max_tl, max_ql, binary_cigar)
        if out is None:
            new = _alloc(dev)
            out = (new((n, 8)), new((n, 8)) if sides else None, new((n, 8)) if sides else None,
                   None if score_only else new(n * cigar_stride, torch.uint8), None if score_only else new(n), new(n))
        aln, left, right, cg, ln, st = out
        p = SWParameters(*parameters)
        flags = _extend_flags(binary_cigar, score_only, to_query_end, adaptive_band)
        ptr = _ptrs(dev, keep_null=True)
        rc = _lib.lib().mgl_sw_extend_seed_batch_device(
            ctx, torch.cuda.current_stream(dev).cuda_stream, n, ptr(targets), ptr(t_start), ptr(t_len), ptr(queries), ptr(q_start), ptr(q_len),
            ptr(seed_t), ptr(seed_q), ptr(seed_len), int(max_tl), int(max_ql), p.match, p.mismatch, p.gap_open, p.gap_extend, int(band), int(zdrop),
            ptr(aln), ptr(left), ptr(right), ptr(cg), int(cigar_stride), ptr(ln), ptr(st), flags)
        _check(rc, ctx)
        return out

    def align_chain(self, refs, alts, chains, band, zdrop, parameters=GATK_PARAMETERS, to_query_end=False, cigar_stride=None, binary_cigar=False,
                    score_only=False, return_status=False, adaptive_band=False, return_sides=False, return_gap_scores=False, max_gap=None):
        """mgl_sw_align_chain_batch_device over lists of byte strings: ``chains[k]`` = a list of anchors (st, sq, sl), colinear and in
        order, each laying refs[k][st:st + sl] against alts[k][sq:sq + sl].  The left side of the first anchor and the right side of the
        last one are extended as ``extend_seed`` extends a seed's, every gap between two anchors is filled globally over the band, and
        all of it is joined into one alignment on the device.  NOT a reference function.  ``max_gap``: (max_gap_tl, max_gap_ql), by
        default the largest gap of the batch.  Returns ChainAlignResult: the eight fields of mgl_sw_chain_alignment as arrays, the
        joined CIGARs and their lengths; with ``return_sides`` also the two sides' records [n, 8], with ``return_gap_scores`` the int32
        array of one gap score per anchor (in the order of the chains, 0 behind a pair's last anchor), with ``return_status`` the
        per-pair status array (and no exception for a pair's status): (result[, left, right][, gap scores][, status])."""
        import torch

        dev = torch.device("cuda", self._device)
        n, packed, cigar_stride = _pack_pairs(refs, alts, dev, cigar_stride, binary_cigar)
        assert len(chains) == n
        start, flat = _csr(chains)
        if max_gap is None:
            gt = gq = 0
            for c in chains:
                for (st, sq, sl), (nt, nq, _) in zip(c, c[1:]):
                    gt, gq = max(gt, nt - st - sl), max(gq, nq - sq - sl)
            max_gap = (max(gt, 0), max(gq, 0))
        g = lambda x: _upload(x, dev)  # noqa: E731
        out = self.align_chain_device(*packed[:6], g(start), g(flat[:, 0]), g(flat[:, 1]), g(flat[:, 2]), *packed[6:], max_gap[0], max_gap[1], band, zdrop,
                                      parameters, to_query_end, cigar_stride, binary_cigar, score_only, adaptive_band=adaptive_band, sides=return_sides,
                                      gap_scores=return_gap_scores)
        aln, left, right, gs, cg, ln, st = _fetch(out, dev, return_status)
        fields = [aln[:, c] for c in range(8)]
        res = ChainAlignResult(*fields, None, None) if score_only else ChainAlignResult(*fields, CigarColumn(cg.reshape(n, cigar_stride), ln), ln)
        ret = (res,) + ((left, right) if return_sides else ()) + ((gs,) if return_gap_scores else ()) + ((st,) if return_status else ())
        return ret if len(ret) > 1 else res

    def align_chain_device(self, targets, t_start, t_len, queries, q_start, q_len, anchor_start, anchor_t, anchor_q, anchor_len, max_tl, max_ql,
                           max_gap_tl, max_gap_ql, band, zdrop, parameters=GATK_PARAMETERS, to_query_end=False, cigar_stride=None, binary_cigar=False,
                           score_only=False, out=None, adaptive_band=False, sides=False, gap_scores=False):
        """The device-tensor form: torch tensors on this context's GPU (uint8 bytes, int64 starts and ``anchor_start`` [n + 1], int32
        lengths and anchors); enqueued on the current stream, not synchronised.  Returns (alignments[n, 8], left[n, 8] or None,
        right[n, 8] or None, gap scores [anchors] or None, cigar bytes [n * stride] or None, cigar lengths or None, status) tensors --
        the side records with ``sides``, the gap scores with ``gap_scores`` --; ``out``: such a tuple to write into."""
        import torch

        ctx = self._ensure()
        n = int(t_start.numel())
        total = int(anchor_t.numel())
        dev = targets.device
        if cigar_stride is None:
            cigar_stride = _default_stride(max_tl, max_ql, binary_cigar)
        if out is None:
            new = _alloc(dev)
            out = (new((n, 8)), new((n, 8)) if sides else None, new((n, 8)) if sides else None, new(total) if gap_scores else None,
                   None if score_only else new(n * cigar_stride, torch.uint8), None if score_only else new(n), new(n))
        aln, left, right, gs, cg, ln, st = out
        p = SWParameters(*parameters)
        flags = _extend_flags(binary_cigar, score_only, to_query_end, adaptive_band)
        ptr = _ptrs(dev, keep_null=True)
        rc = _lib.lib().mgl_sw_align_chain_batch_device(
            ctx, torch.cuda.current_stream(dev).cuda_stream, n, ptr(targets), ptr(t_start), ptr(t_len), ptr(queries), ptr(q_start), ptr(q_len),
            ptr(anchor_start), ptr(anchor_t), ptr(anchor_q), ptr(anchor_len), total, int(max_tl), int(max_ql), int(max_gap_tl), int(max_gap_ql),
            p.match, p.mismatch, p.gap_open, p.gap_extend, int(band), int(zdrop), ptr(aln), ptr(left), ptr(right), ptr(gs), ptr(cg), int(cigar_stride),
            ptr(ln), ptr(st), flags)
        _check(rc, ctx)
        return out

    def chain_anchors(self, t_lens, q_lens, candidates, max_pred=64, max_dist=5000, bw=500, pen_gap=38, pen_skip=0, max_cand=None, return_dp=False,
                      groups=None):
        """mgl_sw_chain_anchors_batch_device over lists: ``candidates[k]`` = a list of (t, q, l) for read k -- t_lens[k] and q_lens[k]
        are its window's and its query's length --, sorted by the caller (by target position) if the window of ``max_pred`` predecessors
        is to mean something.  ``max_dist``: one bound or (max_dist_t, max_dist_q).  The colinear chaining DP of
        tests/chain_dp_textbook.py and the best chain of every read.  NOT a reference function.  Returns ChainAnchorsResult: ``chains``
        (a list of lists of (t, q, l)), ``score`` and ``status`` arrays (a refused read has an empty chain; no exception for a read's
        status); with ``return_dp`` also f and pred of every candidate (int32 arrays in the order of the lists; what a refused read's
        candidates hold is unspecified): (result, f, pred).  ``groups[k]``: a group per candidate of read k -- a candidate is chained
        only to candidates of its own group, and one of group -1 to none (mgl_sw_chain_anchors_grouped_batch_device); None: no groups."""
        import torch

        dev = torch.device("cuda", self._device)
        n = len(candidates)
        assert len(t_lens) == len(q_lens) == n
        start, flat = _csr(candidates)
        if max_cand is None:
            max_cand = int(np.diff(start).max(initial=0))
        g = lambda x, dt: _upload(x, dev, dt)  # noqa: E731
        out = self.chain_anchors_device(g(t_lens, np.int32), g(q_lens, np.int32), g(start, np.int64), g(flat[:, 0], np.int32), g(flat[:, 1], np.int32),
                                        g(flat[:, 2], np.int32), max_cand, max_pred, max_dist, bw, pen_gap, pen_skip, dp=return_dp,
                                        group=None if groups is None else g([x for r in groups for x in r], np.int32))
        torch.cuda.synchronize(dev)
        cs, ct, cq, cl, score, f, pred, st = (None if x is None else x.cpu().numpy() for x in out)
        res = ChainAnchorsResult(_candidate_lists(cs, ct, cq, cl, n), score, st)
        return (res, f, pred) if return_dp else res

    def chain_anchors_device(self, t_len, q_len, cand_start, cand_t, cand_q, cand_len, max_cand, max_pred=64, max_dist=5000, bw=500, pen_gap=38,
                             pen_skip=0, out=None, dp=False, group=None):
        """The device-tensor form: torch tensors on this context's GPU (int32 lengths and candidates, int64 ``cand_start`` [n + 1]);
        enqueued on the current stream, not synchronised.  Returns (chain_start [n + 1] int64, chain_t, chain_q, chain_len [candidates],
        score [n], f or None, pred or None [candidates], status [n]) tensors -- f and pred with ``dp`` --; ``out``: such a tuple to
        write into.  The first four are ``align_chain_device``'s anchor arguments as they are.  ``group``: an int32 tensor, one entry
        per candidate (``Index.contig_of_device`` makes it): mgl_sw_chain_anchors_grouped_batch_device, where a candidate is chained
        only to candidates of its own group and one of group -1 to none (tests/contig_textbook.py); None: the entry without groups."""
        import torch

        ctx = self._ensure()
        n = int(t_len.numel())
        total = int(cand_t.numel())
        dev = t_len.device
        if out is None:
            new = _alloc(dev)
            out = (new(n + 1, torch.int64), new(total), new(total), new(total), new(n), new(total) if dp else None, new(total) if dp else None, new(n))
        cs, ct, cq, cl, score, f, pred, st = out
        dist_t, dist_q = (max_dist, max_dist) if np.isscalar(max_dist) else max_dist
        ptr = _ptrs(dev)
        head = (ctx, torch.cuda.current_stream(dev).cuda_stream, n, ptr(t_len), ptr(q_len), ptr(cand_start), ptr(cand_t), ptr(cand_q), ptr(cand_len))
        tail = (total, int(max_cand), int(max_pred), int(dist_t), int(dist_q), int(bw), int(pen_gap), int(pen_skip), ptr(cs), ptr(ct), ptr(cq), ptr(cl),
                ptr(score), ptr(f), ptr(pred), ptr(st))
        if group is None:
            rc = _lib.lib().mgl_sw_chain_anchors_batch_device(*head, *tail)
        else:
            assert group.numel() >= total
            rc = _lib.lib().mgl_sw_chain_anchors_grouped_batch_device(*head, ptr(group), *tail)
        _check(rc, ctx)
        return out

    def align_candidates_device(self, targets, t_start, t_len, queries, q_start, q_len, cand_start, cand_t, cand_q, cand_len, max_tl, max_ql, max_cand,
                                band, zdrop, parameters=GATK_PARAMETERS, max_pred=64, max_dist=5000, bw=500, pen_gap=38, pen_skip=0, chain_out=None,
                                **align):
        """Candidates -> chain -> alignment on the current stream: ``chain_anchors_device`` and then ``align_chain_device`` on the
        tensors it wrote (max_gap = max_dist), nothing read back and nothing synchronised in between.  ``align``: the further
        arguments of ``align_chain_device``.  Returns (the chain stage's tuple, the alignment's tuple).  A read with no candidates or
        a refused one has K = 0 and is status MGL_SW_ERR_BAD_ARG in the alignment's tuple.  ``max_dist`` is also the gap bound of the
        alignment, which stages a CIGAR row of 4 (max_dist_t + max_dist_q) bytes per candidate: keep it near the largest gap expected."""
        chain = self.chain_anchors_device(t_len, q_len, cand_start, cand_t, cand_q, cand_len, max_cand, max_pred, max_dist, bw, pen_gap, pen_skip,
                                          out=chain_out)
        dist_t, dist_q = (max_dist, max_dist) if np.isscalar(max_dist) else max_dist
        return chain, self.align_chain_device(targets, t_start, t_len, queries, q_start, q_len, *chain[:4], max_tl, max_ql, dist_t, dist_q, band, zdrop,
                                              parameters, **align)

    def seed(self, targets, queries, k=15, w=10, max_occ=8, merge=True, max_cand=4096):
        """mgl_sw_seed_batch_device over lists of byte strings: read k (``queries[k]``) is seeded against its own window
        (``targets[k]``) -- the (w, k) minimizers of both, their common keys as hits, a key that occurs more than ``max_occ`` times in
        the read's sketch dropped, and with ``merge`` the hits on one diagonal that overlap or touch merged into maximal exact runs
        (tests/seed_textbook.py).  NOT a reference function.  ``max_cand`` bounds a pair's raw hits.  Returns SeedResult:
        ``candidates`` (a list of lists of (t, q, l), ascending by (t, q): what ``chain_anchors`` takes) and ``status`` (a refused pair
        has no candidates; no exception for a pair's status)."""
        import torch

        dev = torch.device("cuda", self._device)
        n, packed, _ = _pack_pairs(targets, queries, dev, 16, False)
        out = self.seed_device(*packed[:6], k, w, max_occ, merge, max_cand)
        torch.cuda.synchronize(dev)
        cs, ct, cq, cl, st = (x.cpu().numpy() for x in out)
        return SeedResult(_candidate_lists(cs, ct, cq, cl, n), st)

    def seed_device(self, targets, t_start, t_len, queries, q_start, q_len, k=15, w=10, max_occ=8, merge=True, max_cand=4096, cand_capacity=None,
                    out=None):
        """The device-tensor form: torch tensors on this context's GPU (uint8 bytes, int64 starts, int32 lengths); enqueued on the
        current stream, not synchronised.  Returns (cand_start [n + 1] int64, cand_t, cand_q, cand_len [cand_capacity] int32, status
        [n]) tensors; ``out``: such a tuple to write into (its status may be None), whose candidate arrays then give the capacity.
        ``cand_capacity`` defaults to n * max_cand, which always fits; pairs from the first that does not fit on are status
        MGL_SW_ERR_NOMEM.  The first four are ``chain_anchors_device``'s candidate arguments as they are."""
        import torch

        ctx = self._ensure()
        n = int(t_start.numel())
        dev = targets.device
        if cand_capacity is None:
            cand_capacity = int(out[1].numel()) if out is not None else min(n * int(max_cand), 1 << 30)
        if out is None:
            new = _alloc(dev)
            out = (new(n + 1, torch.int64), new(cand_capacity), new(cand_capacity), new(cand_capacity), new(n))
        cs, ct, cq, cl, st = out
        assert min(ct.numel(), cq.numel(), cl.numel()) >= cand_capacity and cs.numel() >= n + 1
        ptr = _ptrs(dev)
        rc = _lib.lib().mgl_sw_seed_batch_device(
            ctx, torch.cuda.current_stream(dev).cuda_stream, n, ptr(targets), ptr(t_start), ptr(t_len), ptr(queries), ptr(q_start), ptr(q_len), int(k),
            int(w), int(max_occ), int(merge), int(max_cand), int(cand_capacity), ptr(cs), ptr(ct), ptr(cq), ptr(cl), ptr(st))
        _check(rc, ctx)
        return out

    def align_reads_device(self, targets, t_start, t_len, queries, q_start, q_len, max_tl, max_ql, band, zdrop, parameters=GATK_PARAMETERS, k=15,
                           w=10, max_occ=8, merge=True, max_cand=4096, cand_capacity=None, seed_out=None, **chain_align):
        """Reads -> seeds -> chain -> alignment on the current stream: ``seed_device`` and then ``align_candidates_device`` on the
        tensors it wrote, nothing read back and nothing synchronised in between.  ``chain_align``: the further arguments of
        ``align_candidates_device`` (the chaining parameters, ``chain_out`` and those of ``align_chain_device``).  Returns (the seed
        stage's tuple, the chain stage's tuple, the alignment's tuple).  A pair the seed stage refused or found nothing for has no
        chain and is status MGL_SW_ERR_BAD_ARG in the alignment's tuple."""
        seeds = self.seed_device(targets, t_start, t_len, queries, q_start, q_len, k, w, max_occ, merge, max_cand, cand_capacity, out=seed_out)
        chain, aln = self.align_candidates_device(targets, t_start, t_len, queries, q_start, q_len, *seeds[:4], max_tl, max_ql, max_cand, band, zdrop,
                                                  parameters, **chain_align)
        return seeds, chain, aln

    def seed_strands(self, targets, queries, k=15, w=10, max_occ=8, merge=True, max_cand=4096):
        """mgl_sw_seed_strands_batch_device over lists of byte strings: ``seed`` for reads of unknown orientation
        (tests/strand_textbook.py).  Pair p gives two rows: row 2p is ``seed``'s result for (targets[p], queries[p]), row 2p + 1 that
        for (targets[p], the reverse complement of queries[p]) -- a candidate's q is a coordinate of that row's oriented read.  NOT a
        reference function.  Returns SeedResult over the 2n rows."""
        import torch

        dev = torch.device("cuda", self._device)
        n, packed, _ = _pack_pairs(targets, queries, dev, 16, False)
        out = self.seed_strands_device(*packed[:6], k, w, max_occ, merge, max_cand)
        torch.cuda.synchronize(dev)
        cs, ct, cq, cl, _, _, st = (x.cpu().numpy() for x in out)
        return SeedResult(_candidate_lists(cs, ct, cq, cl, 2 * n), st)

    def seed_strands_device(self, targets, t_start, t_len, queries, q_start, q_len, k=15, w=10, max_occ=8, merge=True, max_cand=4096,
                            cand_capacity=None, out=None):
        """The device-tensor form: ``seed_device``'s arguments; enqueued on the current stream, not synchronised.  Returns (cand_start
        [2n + 1] int64, cand_t, cand_q, cand_len [cand_capacity] int32, row_t_len, row_q_len, status [2n] int32) tensors over the 2n
        rows; ``out``: such a tuple to write into (its last three may be None), whose candidate arrays then give the capacity.
        ``cand_capacity`` defaults to 2n * max_cand, which always fits.  (row_t_len, row_q_len) and the first four are
        ``chain_anchors_device``'s arguments over the 2n rows as they are."""
        import torch

        ctx = self._ensure()
        n = int(t_start.numel())
        dev = targets.device
        if cand_capacity is None:
            cand_capacity = int(out[1].numel()) if out is not None else min(2 * n * int(max_cand), 1 << 30)
        cs, ct, cq, cl, rt, rq, st = out = _seed_rows(out, 2 * n, cand_capacity, dev)
        ptr = _ptrs(dev)
        rc = _lib.lib().mgl_sw_seed_strands_batch_device(
            ctx, torch.cuda.current_stream(dev).cuda_stream, n, ptr(targets), ptr(t_start), ptr(t_len), ptr(queries), ptr(q_start), ptr(q_len), int(k),
            int(w), int(max_occ), int(merge), int(max_cand), int(cand_capacity), ptr(cs), ptr(ct), ptr(cq), ptr(cl), ptr(rt), ptr(rq), ptr(st))
        _check(rc, ctx)
        return out

    def select_strand_device(self, queries, q_start, q_len, chain_start, chain_t, chain_q, chain_len, chain_score, out=None):
        """mgl_sw_select_strand_batch_device on device tensors: the n reads and ``chain_anchors_device``'s first five outputs over the 2n
        rows of ``seed_strands_device``; enqueued on the current stream, not synchronised.  Read p's strand is 1 iff the chain of row
        2p + 1 scores higher than that of row 2p (tests/strand_textbook.py).  Returns (strand [n] int32, queries_out uint8 (as large as
        ``queries``: read p oriented at q_start[p]; bytes outside the reads are not written), anchor_start [n + 1] int64, anchor_t,
        anchor_q, anchor_len [as chain_t] int32, score [n], status [n]) tensors; ``out``: such a tuple to write into (its last two may
        be None).  With queries_out for the queries, the four anchor arrays are ``align_chain_device``'s arguments as they are."""
        import torch

        ctx = self._ensure()
        n = int(q_start.numel())
        total = int(chain_t.numel())
        dev = queries.device
        if out is None:
            new = _alloc(dev)
            out = (new(n), torch.empty_like(queries), new(n + 1, torch.int64), new(total), new(total), new(total), new(n), new(n))
        strand, qo, as_, at, aq, al, score, st = out
        assert chain_start.numel() >= 2 * n + 1 and chain_score.numel() >= 2 * n and min(chain_q.numel(), chain_len.numel()) >= total
        assert qo.numel() >= queries.numel() and as_.numel() >= n + 1 and min(at.numel(), aq.numel(), al.numel()) >= total and strand.numel() >= n
        ptr = _ptrs(dev)
        rc = _lib.lib().mgl_sw_select_strand_batch_device(
            ctx, torch.cuda.current_stream(dev).cuda_stream, n, ptr(queries), ptr(q_start), ptr(q_len), ptr(chain_start), ptr(chain_t), ptr(chain_q),
            ptr(chain_len), ptr(chain_score), total, int(queries.numel()), ptr(strand), ptr(qo), ptr(as_), ptr(at), ptr(aq), ptr(al), ptr(score), ptr(st))
        _check(rc, ctx)
        return out

    def align_reads_strands_device(self, targets, t_start, t_len, queries, q_start, q_len, max_tl, max_ql, band, zdrop, parameters=GATK_PARAMETERS,
                                   k=15, w=10, max_occ=8, merge=True, max_cand=4096, cand_capacity=None, seed_out=None, max_pred=64, max_dist=5000,
                                   bw=500, pen_gap=38, pen_skip=0, chain_out=None, select_out=None, **align):
        """``align_reads_device`` for reads of unknown orientation, on the current stream: ``seed_strands_device`` ->
        ``chain_anchors_device`` over the 2n rows -> ``select_strand_device`` -> ``align_chain_device`` on the oriented reads, nothing
        read back and nothing synchronised in between.  ``align``: the further arguments of ``align_chain_device``.  Returns (the seed
        stage's tuple, the chain stage's tuple, the choice's tuple, the alignment's tuple).  q_beg / q_end and the CIGAR of the alignment
        are in the ORIENTED read's coordinates (the choice's queries_out): on the read as given, a pair of strand 1 spans
        [ql - q_end, ql - q_beg).  A pair with a chain on neither row is strand 0 and status MGL_SW_ERR_BAD_ARG in the alignment's
        tuple."""
        seeds = self.seed_strands_device(targets, t_start, t_len, queries, q_start, q_len, k, w, max_occ, merge, max_cand, cand_capacity, out=seed_out)
        chain = self.chain_anchors_device(seeds[4], seeds[5], *seeds[:4], max_cand, max_pred, max_dist, bw, pen_gap, pen_skip, out=chain_out)
        chosen = self.select_strand_device(queries, q_start, q_len, *chain[:5], out=select_out)
        dist_t, dist_q = (max_dist, max_dist) if np.isscalar(max_dist) else max_dist
        aln = self.align_chain_device(targets, t_start, t_len, chosen[1], q_start, q_len, *chosen[2:6], max_tl, max_ql, dist_t, dist_q, band, zdrop,
                                      parameters, **align)
        return seeds, chain, chosen, aln

    def build_index(self, ref, k=15, w=10):
        """mgl_sw_index_build_device: the minimizer index of one reference, built on the device (tests/index_textbook.py).  ``ref``:
        a uint8 tensor on this context's GPU, or bytes (copied there).  NOT a reference function.  Synchronises the current stream.
        Returns an ``Index``, which keeps the reference tensor: ``map_reads_device`` aligns against it in place.  No byte beyond the
        reference is read by any stage (the band kernels load a window's bytes one by one), so the tensor needs no padding."""
        import torch

        ctx = self._ensure()
        dev = torch.device("cuda", self._device)
        if not isinstance(ref, torch.Tensor):
            ref = torch.from_numpy(np.frombuffer(bytes(ref), dtype=np.uint8).copy()).to(dev)
        assert ref.dtype == torch.uint8 and ref.is_contiguous()
        handle = C.c_void_p()
        rc = _lib.lib().mgl_sw_index_build_device(ctx, torch.cuda.current_stream(dev).cuda_stream, ref.data_ptr() or None, int(ref.numel()), int(k), int(w),
                                                  C.byref(handle))
        _check(rc, ctx)
        return Index(handle, ref, None, self)

    def build_index_contigs(self, contigs, k=15, w=10, gap=1):
        """mgl_sw_index_build_contigs_device over a list of (name, bytes): the contigs laid into one buffer with ``gap`` >= 1 bytes
        of ``N`` between two of them, that buffer indexed as ``build_index`` does, and the table kept (DESIGN.md section 9m,
        tests/contig_textbook.py).  NOT a reference function.  Returns an ``Index`` whose ``contigs`` is the ContigTable: the
        mappers then chain and place a read inside ONE contig and report positions from that contig's start."""
        assert gap >= 1 and len(contigs) >= 1
        names, seqs = [n for n, _ in contigs], [bytes(s) for _, s in contigs]
        starts = np.cumsum([0] + [len(s) + gap for s in seqs[:-1]]).astype(np.int64)
        return self.build_index_contigs_device((b"N" * gap).join(seqs), starts, [len(s) for s in seqs], names, k, w)

    def build_index_contigs_device(self, ref, starts, lens, names=None, k=15, w=10):
        """The variant for a buffer that is laid out already: ``ref`` a uint8 tensor on this context's GPU (or bytes, copied there),
        ``starts`` and ``lens`` its contigs (host integers; include/mgl_sw.h has the rules: they and the gaps tile the buffer, and
        a gap holds no base), ``names`` default to contig0 ...  Synchronises the current stream."""
        import torch

        ctx = self._ensure()
        dev = torch.device("cuda", self._device)
        if not isinstance(ref, torch.Tensor):
            ref = torch.from_numpy(np.frombuffer(bytes(ref), dtype=np.uint8).copy()).to(dev)
        assert ref.dtype == torch.uint8 and ref.is_contiguous()
        starts, lens = np.ascontiguousarray(starts, dtype=np.int64), np.ascontiguousarray(lens, dtype=np.int64)
        assert starts.ndim == lens.ndim == 1 and len(starts) == len(lens)
        names = ["contig%d" % c for c in range(len(starts))] if names is None else [str(x) for x in names]
        assert len(names) == len(starts)
        handle = C.c_void_p()
        rc = _lib.lib().mgl_sw_index_build_contigs_device(ctx, torch.cuda.current_stream(dev).cuda_stream, ref.data_ptr() or None, int(ref.numel()),
                                                          starts.ctypes.data, lens.ctypes.data, len(starts), int(k), int(w), C.byref(handle))
        _check(rc, ctx)
        return Index(handle, ref, ContigTable(names, starts, lens), self)

    def locate_window_contigs_device(self, index, q_len, anchor_start, anchor_t, anchor_q, anchor_len, slack, max_tl, out=None, in_place=False):
        """mgl_sw_locate_window_contigs_batch_device on device tensors: ``locate_window_device`` with the window kept inside the contig
        of the read's first anchor, and a read whose anchors lie in two contigs (or in none) refused (tests/contig_textbook.py).
        Returns (t_start [n] int64 -- in the BUFFER's coordinates --, t_len [n], anchor_t, status [n], rid [n] int32: the read's contig,
        -1 for an unmapped or a refused read); ``out``: such a tuple (its status may be None).  An index of one sequence is one contig."""
        import torch

        ctx = self._ensure()
        n = int(q_len.numel())
        total = int(anchor_t.numel())
        dev = q_len.device
        if out is None:
            new = _alloc(dev)
            out = (new(n, torch.int64), new(n), anchor_t if in_place else new(total), new(n), new(n))
        ts, tl, at, st, rid = out
        assert anchor_start.numel() >= n + 1 and min(anchor_q.numel(), anchor_len.numel(), at.numel()) >= total and min(ts.numel(), tl.numel(), rid.numel()) >= n
        ptr = _ptrs(dev)
        rc = _lib.lib().mgl_sw_locate_window_contigs_batch_device(
            ctx, torch.cuda.current_stream(dev).cuda_stream, n, index.handle, ptr(q_len), ptr(anchor_start), ptr(anchor_t), ptr(anchor_q), ptr(anchor_len),
            total, int(slack), int(max_tl), ptr(ts), ptr(tl), ptr(at), ptr(rid), ptr(st))
        _check(rc, ctx)
        return out

    def seed_index(self, index, queries, strands=2, max_occ=8, max_occ_ref=64, merge=True, max_cand=4096):
        """mgl_sw_seed_index_batch_device over a list of byte strings: ``seed_strands`` with the whole indexed reference for every
        read's window -- no window is needed (tests/index_textbook.py).  A key that occurs more than ``max_occ`` times in a read's
        sketch or more than ``max_occ_ref`` times in the index is dropped.  NOT a reference function.  Returns SeedResult over the
        ``strands`` * n rows; a candidate's t is a position of the reference."""
        import torch

        dev = torch.device("cuda", self._device)
        n, packed, _ = _pack_reads(queries, dev)
        out = self.seed_index_device(index, *packed, strands, max_occ, max_occ_ref, merge, max_cand)
        torch.cuda.synchronize(dev)
        cs, ct, cq, cl, _, _, st = (x.cpu().numpy() for x in out)
        return SeedResult(_candidate_lists(cs, ct, cq, cl, strands * n), st)

    def seed_index_device(self, index, queries, q_start, q_len, strands=2, max_occ=8, max_occ_ref=64, merge=True, max_cand=4096, cand_capacity=None,
                          out=None):
        """The device-tensor form: ``seed_strands_device``'s read arguments and its tuple over the ``strands`` * n rows (row_t_len is
        the reference's length); enqueued on the current stream, not synchronised.  ``cand_capacity`` defaults to strands * n *
        max_cand, which always fits."""
        import torch

        ctx = self._ensure()
        n = int(q_start.numel())
        rows = max(int(strands), 0) * n
        dev = queries.device
        if cand_capacity is None:
            cand_capacity = int(out[1].numel()) if out is not None else min(rows * int(max_cand), 1 << 30)
        cs, ct, cq, cl, rt, rq, st = out = _seed_rows(out, rows, cand_capacity, dev)
        ptr = _ptrs(dev)
        rc = _lib.lib().mgl_sw_seed_index_batch_device(
            ctx, torch.cuda.current_stream(dev).cuda_stream, index.handle, n, ptr(queries), ptr(q_start), ptr(q_len), int(strands), int(max_occ),
            int(max_occ_ref), int(merge), int(max_cand), int(cand_capacity), ptr(cs), ptr(ct), ptr(cq), ptr(cl), ptr(rt), ptr(rq), ptr(st))
        _check(rc, ctx)
        return out

    def locate_window_device(self, index_or_ref_len, q_len, anchor_start, anchor_t, anchor_q, anchor_len, slack, max_tl, out=None, in_place=False):
        """mgl_sw_locate_window_batch_device on device tensors: every read's chain (``chain_anchors_device``'s or
        ``select_strand_device``'s anchor arrays, t in the reference's coordinates) -> its window of the reference, ``slack`` bases
        beyond what the read's ends need, and the anchors' t relative to it (tests/index_textbook.py); enqueued on the current
        stream, not synchronised.  Returns (t_start [n] int64, t_len [n] int32, anchor_t [as anchor_t] int32, status [n]) tensors;
        ``out``: such a tuple to write into (its status may be None); ``in_place``: the rebased t overwrite ``anchor_t``.  With the
        reference for the targets they are ``align_chain_device``'s arguments as they are.  A read without anchors has t_len 0."""
        import torch

        ctx = self._ensure()
        ref_len = index_or_ref_len.info.ref_len if isinstance(index_or_ref_len, Index) else int(index_or_ref_len)
        n = int(q_len.numel())
        total = int(anchor_t.numel())
        dev = q_len.device
        if out is None:
            new = _alloc(dev)
            out = (new(n, torch.int64), new(n), anchor_t if in_place else new(total), new(n))
        ts, tl, at, st = out
        assert anchor_start.numel() >= n + 1 and min(anchor_q.numel(), anchor_len.numel(), at.numel()) >= total and min(ts.numel(), tl.numel()) >= n
        ptr = _ptrs(dev)
        rc = _lib.lib().mgl_sw_locate_window_batch_device(
            ctx, torch.cuda.current_stream(dev).cuda_stream, n, ref_len, ptr(q_len), ptr(anchor_start), ptr(anchor_t), ptr(anchor_q), ptr(anchor_len), total,
            int(slack), int(max_tl), ptr(ts), ptr(tl), ptr(at), ptr(st))
        _check(rc, ctx)
        return out

    def map_reads_device(self, index, queries, q_start, q_len, max_tl, max_ql, band, zdrop, parameters=GATK_PARAMETERS, slack=200, strands=2, max_occ=8,
                         max_occ_ref=64, merge=True, max_cand=4096, cand_capacity=None, seed_out=None, max_pred=64, max_dist=5000, bw=500, pen_gap=38,
                         pen_skip=0, chain_out=None, select_out=None, locate_out=None, **align):
        """Reads in, positions and CIGARs out, on the current stream: ``seed_index_device`` -> ``chain_anchors_device`` over the rows
        -> (``strands`` = 2) ``select_strand_device`` -> ``locate_window_device`` -> ``align_chain_device`` on the index's reference
        in place, nothing read back and nothing synchronised in between.  ``max_tl`` bounds a read's window of the reference;
        ``align``: the further arguments of ``align_chain_device``.  Returns (the seed stage's tuple, the chain stage's tuple, the
        choice's tuple or None, the window's tuple, the alignment's tuple).  The alignment's t_beg / t_end are relative to the read's
        window: on the reference it spans [t_start + t_beg, t_start + t_end); q and the CIGAR are the ORIENTED read's, as in
        ``align_reads_strands_device``.  A read without a chain (unmapped) has t_len 0 and is status MGL_SW_ERR_BAD_ARG in the
        alignment's tuple.  Where the index has contigs (``build_index_contigs``) the candidates get their contig
        (``Index.contig_of_device``), the chain stage runs grouped by it and the window comes from ``locate_window_contigs_device``:
        its tuple then has rid as a fifth element, and t_start still counts from the start of the buffer."""
        seeds = self.seed_index_device(index, queries, q_start, q_len, strands, max_occ, max_occ_ref, merge, max_cand, cand_capacity, out=seed_out)
        group = index.contig_of_device(seeds[1], seeds[3]) if index.contigs is not None else None
        chain = self.chain_anchors_device(seeds[4], seeds[5], *seeds[:4], max_cand, max_pred, max_dist, bw, pen_gap, pen_skip, out=chain_out, group=group)
        chosen = self.select_strand_device(queries, q_start, q_len, *chain[:5], out=select_out) if strands == 2 else None
        oriented, anchors = (chosen[1], chosen[2:6]) if chosen is not None else (queries, chain[:4])
        locate = self.locate_window_contigs_device if index.contigs is not None else self.locate_window_device
        window = locate(index, q_len, *anchors, slack, max_tl, out=locate_out)
        dist_t, dist_q = (max_dist, max_dist) if np.isscalar(max_dist) else max_dist
        aln = self.align_chain_device(index.ref, window[0], window[1], oriented, q_start, q_len, anchors[0], window[2], anchors[2], anchors[3], max_tl,
                                      max_ql, dist_t, dist_q, band, zdrop, parameters, **align)
        return seeds, chain, chosen, window, aln

    def map_reads(self, index, reads, band=64, zdrop=-1, parameters=GATK_PARAMETERS, slack=200, strands=2, max_tl=None, **stages):
        """``map_reads_device`` over a list of byte strings.  ``max_tl`` defaults to 1.5 times the longest read and the slack to
        either side; ``stages``: the further arguments of ``map_reads_device``.  Returns MapResult, per read: ``ref_beg`` and
        ``ref_end`` (the alignment spans [ref_beg, ref_end) of the reference), ``strand``, ``score``, ``cigars`` (of the oriented
        read) and ``status`` (0; the window's status where it refused the read; MGL_SW_ERR_BAD_ARG for an unmapped read -- such a
        read's other fields are 0 and its CIGAR empty; no exception for a read's status).  Against an index with contigs
        (``build_index_contigs``) it returns ContigMapResult: the same fields with ``ref_beg`` and ``ref_end`` counted from the start
        of the read's contig, and ``rid`` (-1: unmapped) and ``rname``."""
        import torch

        dev = torch.device("cuda", self._device)
        n, packed, max_tl, max_ql, stride = _map_setup(reads, dev, slack, max_tl, stages)
        _, _, chosen, window, aln = self.map_reads_device(index, *packed, max_tl, max_ql, band, zdrop, parameters, slack, strands, cigar_stride=stride,
                                                          **stages)
        torch.cuda.synchronize(dev)
        fields, _, _, contig = _map_fields(n, stride, chosen, window, aln, index)
        return ContigMapResult(*fields, *contig) if contig else MapResult(*fields)

    def rank_chains(self, row_q_lens, candidates, f, pred, row_status=None, strands=2, max_chains=4, min_score=40, min_cnt=3, mask_level=128,
                    max_cand=None, return_anchors=False):
        """mgl_sw_rank_chains_batch_device over lists: ``candidates[r]`` = the (t, q, l) of row r, ``f[r]`` and ``pred[r]`` the chain
        stage's values for them (``chain_anchors(..., return_dp=True)``), ``row_q_lens[r]`` the row's read length; read p has the rows
        strands * p .. (tests/rank_textbook.py).  NOT a reference function.  Returns (chains, status): ``chains[p]`` the RankedChain
        records of read p in rank order (a refused read has none; no exception for a read's status); with ``return_anchors`` also,
        per read and chain, the chain's [(t, q, l)] ascending: (chains, anchors, status)."""
        import torch

        dev = torch.device("cuda", self._device)
        rows = len(candidates)
        assert len(row_q_lens) == len(f) == len(pred) == rows and strands in (1, 2) and rows % strands == 0
        start, flat = _csr(candidates)
        cat = lambda xs: np.asarray([v for x in xs for v in x], dtype=np.int32)  # noqa: E731
        if max_cand is None:
            max_cand = int(np.diff(start).max(initial=0))
        g = lambda x, dt: _upload(x, dev, dt)  # noqa: E731
        out = self.rank_chains_device(g(row_q_lens, np.int32), g(start, np.int64), g(flat[:, 0], np.int32), g(flat[:, 1], np.int32), g(flat[:, 2], np.int32),
                                      g(cat(f), np.int32), g(cat(pred), np.int32), None if row_status is None else g(row_status, np.int32), strands, max_cand,
                                      max_chains, min_score, min_cnt, mask_level, anchors=return_anchors)
        torch.cuda.synchronize(dev)
        nc, rec, rs, rt, rq, rl, st = (None if x is None else x.cpu().numpy() for x in out)
        chains = [[RankedChain(*(int(v) for v in rec[p, c])) for c in range(nc[p])] for p in range(rows // strands)]
        if not return_anchors:
            return chains, st
        # a read's chains stand one behind the other from ranked_start[p] on
        anchors = [_candidate_lists(int(rs[p]) + np.cumsum([0] + [c.n_anchors for c in cs]), rt, rq, rl, len(cs)) for p, cs in enumerate(chains)]
        return chains, anchors, st

    def rank_chains_device(self, row_q_len, cand_start, cand_t, cand_q, cand_len, f, pred, row_status=None, strands=2, max_cand=4096, max_chains=4,
                           min_score=40, min_cnt=3, mask_level=128, anchors=False, out=None):
        """The device-tensor form: the rows' tensors as ``seed_index_device`` and ``chain_anchors_device(dp=True)`` wrote them (int32;
        int64 ``cand_start`` [rows + 1]); enqueued on the current stream, not synchronised.  Returns (n_chains [n] int32, records
        [n, max_chains, 12] int32 -- mgl_sw_ranked_chain's fields; rows at or beyond n_chains are not written --, ranked_start [n + 1]
        int64, ranked_t, ranked_q, ranked_len [candidates] int32 -- all four None without ``anchors`` --, status [n] int32) tensors;
        ``out``: such a tuple to write into (its status may be None), whose anchor tensors decide whether anchors are written."""
        import torch

        ctx = self._ensure()
        rows = int(row_q_len.numel())
        n = rows // strands if strands in (1, 2) else rows
        total = int(cand_t.numel())
        dev = row_q_len.device
        if out is None:
            new = _alloc(dev)
            out = (new(n), new((n, max(int(max_chains), 0), 12)), new(n + 1, torch.int64) if anchors else None,
                   *((new(total) if anchors else None) for _ in range(3)), new(n))
        nc, rec, rs, rt, rq, rl, st = out
        assert strands not in (1, 2) or (rows % strands == 0 and cand_start.numel() >= rows + 1)
        assert nc.numel() >= n and rec.numel() >= n * max_chains * 12 and min(cand_q.numel(), cand_len.numel(), f.numel(), pred.numel()) >= total
        ptr = _ptrs(dev)
        rc = _lib.lib().mgl_sw_rank_chains_batch_device(
            ctx, torch.cuda.current_stream(dev).cuda_stream, n, int(strands), ptr(row_q_len), ptr(cand_start), ptr(cand_t), ptr(cand_q), ptr(cand_len), total,
            ptr(f), ptr(pred), ptr(row_status), int(max_cand), int(max_chains), int(min_score), int(min_cnt), int(mask_level), ptr(nc), ptr(rec), ptr(rs),
            ptr(rt), ptr(rq), ptr(rl), ptr(st))
        _check(rc, ctx)
        return out

    def expand_chains_device(self, queries, q_start, q_len, rank_status, n_chains, records, ranked_start, ranked_t, ranked_q, ranked_len, max_chains=4,
                             keep_secondary=True, job_capacity=None, out=None):
        """mgl_sw_expand_chains_batch_device on device tensors: the reads (uint8 ``queries``, int64 ``q_start``, int32 ``q_len``) and
        what ``rank_chains_device(anchors=True)`` wrote for them (its status may be None) -> one alignment job per ranked chain
        (tests/lines_textbook.py); enqueued on the current stream, not synchronised.  ``job_capacity`` defaults to n * max_chains.
        Returns (n_jobs [1] int64, job_start [n + 1] int64, jobs [job_capacity, 8] int32 -- mgl_sw_job's fields --, job_q_start
        [job_capacity] int64, job_q_len [job_capacity] int32, job_anchor_start [job_capacity + 1] int64, job_anchor_t, job_anchor_q,
        job_anchor_len [as ranked_t] int32, oriented [2 * queries.numel()] uint8, status [n] int32) tensors; ``out``: such a tuple to
        write into (its status may be None).  Jobs at or beyond n_jobs are empty (read -1, q_len 0): the stages behind this one run
        over all job_capacity of them and refuse those."""
        import torch

        ctx = self._ensure()
        n = int(q_start.numel())
        total, qbytes = int(ranked_t.numel()), int(queries.numel())
        dev = queries.device
        if job_capacity is None:
            job_capacity = n * max(int(max_chains), 0)
        cap = int(job_capacity)
        if out is None:
            new = _alloc(dev)
            c = max(cap, 0)
            out = (new(1, torch.int64), new(n + 1, torch.int64), new((c, 8)), new(c, torch.int64), new(c), new(c + 1, torch.int64), new(total), new(total),
                   new(total), new(2 * qbytes, torch.uint8), new(n))
        nj, js, jobs, jqs, jql, jas, jat, jaq, jal, ori, st = out
        assert q_len.numel() >= n and n_chains.numel() >= n and records.numel() >= n * max_chains * 12 and ranked_start.numel() >= n + 1
        assert min(ranked_q.numel(), ranked_len.numel(), jat.numel(), jaq.numel(), jal.numel()) >= total
        assert js.numel() >= n + 1 and jobs.numel() >= 8 * cap and min(jqs.numel(), jql.numel()) >= cap and jas.numel() >= cap + 1 and ori.numel() >= 2 * qbytes
        ptr = _ptrs(dev)
        rc = _lib.lib().mgl_sw_expand_chains_batch_device(
            ctx, torch.cuda.current_stream(dev).cuda_stream, n, ptr(queries), ptr(q_start), ptr(q_len), qbytes, ptr(rank_status), ptr(n_chains), ptr(records),
            int(max_chains), ptr(ranked_start), ptr(ranked_t), ptr(ranked_q), ptr(ranked_len), total, int(bool(keep_secondary)), cap, ptr(nj), ptr(js),
            ptr(jobs), ptr(jqs), ptr(jql), ptr(jas), ptr(jat), ptr(jaq), ptr(jal), ptr(ori), ptr(st))
        _check(rc, ctx)
        return out

    def classify_alignments_device(self, job_start, jobs, aln, aln_status, match=None, min_score=40, mask_level=128, out=None):
        """mgl_sw_classify_alignments_batch_device on device tensors: ``expand_chains_device``'s job_start [n + 1] and jobs
        [job_capacity, 8] and ``align_chain_device``'s records [job_capacity, 8] and status over those jobs -> the lines of every read
        (tests/lines_textbook.py); enqueued on the current stream, not synchronised.  ``match`` defaults to GATK_PARAMETERS'.  Returns
        (lines [job_capacity, 8] int32 -- mgl_sw_line's fields, per job; only the jobs of accepted reads are written --, n_lines [n],
        primary_job [n], status [n]) tensors; ``out``: such a tuple to write into (its status may be None)."""
        ctx = self._ensure()
        n = int(job_start.numel()) - 1
        cap = int(jobs.numel()) // 8
        dev = jobs.device
        if match is None:
            match = GATK_PARAMETERS.match
        if out is None:
            new = _alloc(dev)
            out = (new((cap, 8)), new(max(n, 0)), new(max(n, 0)), new(max(n, 0)))
        lines, nl, pj, st = out
        assert aln.numel() >= 8 * cap and aln_status.numel() >= cap and lines.numel() >= 8 * cap and min(nl.numel(), pj.numel()) >= n
        import torch

        ptr = _ptrs(dev)
        rc = _lib.lib().mgl_sw_classify_alignments_batch_device(
            ctx, torch.cuda.current_stream(dev).cuda_stream, n, ptr(job_start), ptr(jobs), cap, ptr(aln), ptr(aln_status), int(match), int(min_score),
            int(mask_level), ptr(lines), ptr(nl), ptr(pj), ptr(st))
        _check(rc, ctx)
        return out

    def map_reads_all_device(self, index, queries, q_start, q_len, max_tl, max_ql, band, zdrop, parameters=GATK_PARAMETERS, slack=200, strands=2, max_occ=8,
                             max_occ_ref=64, merge=True, max_cand=4096, cand_capacity=None, max_pred=64, max_dist=5000, bw=500, pen_gap=38, pen_skip=0,
                             max_chains=4, min_score=40, min_cnt=3, mask_level=128, keep_secondary=True, job_capacity=None, md_stride=None,
                             xcigar_stride=None, xcigar=True, **align):
        """Reads in, EVERY ranked chain aligned and classified, on the current stream with nothing read back and nothing synchronised:
        ``seed_index_device`` -> (``Index.contig_of_device`` where the index has contigs) -> ``chain_anchors_device`` with f and pred
        -> ``rank_chains_device(anchors=True)`` -> ``expand_chains_device`` -> ``locate_window_device`` /
        ``locate_window_contigs_device`` over the JOBS -> ``align_chain_device`` on the index's reference and the oriented buffer ->
        ``describe_device`` -> ``classify_alignments_device``.  ``job_capacity`` defaults to n * max_chains; the stages behind the
        expansion run over all of them and refuse the empty ones (status MGL_SW_ERR_BAD_ARG).  ``align``: the further arguments of
        ``align_chain_device``.  Returns the stages' tuples: (seeds, chain, ranked, jobs, window, aln, described, lines).  Rows of
        window, aln and described are per job; a line's t_beg / t_end are relative to its job's window, its q and CIGAR those of the
        job's strand's oriented read.  Split reads want ``to_query_end=False`` or a Z-drop: an extension to the query's end aligns
        through a breakpoint."""
        import torch

        n = int(q_start.numel())
        dev = queries.device
        binary = bool(align.get("binary_cigar", False))
        if align.get("cigar_stride") is None:
            align["cigar_stride"] = _default_stride(max_tl, max_ql, binary)
        stride = int(align["cigar_stride"])
        rows = max(int(strands), 0) * n
        total = cand_capacity if cand_capacity is not None else min(rows * int(max_cand), 1 << 30)
        new = _alloc(dev)
        chain_out = (new(rows + 1, torch.int64), new(total), new(total), new(total), new(rows), new(total), new(total), new(rows))
        seeds = self.seed_index_device(index, queries, q_start, q_len, strands, max_occ, max_occ_ref, merge, max_cand, cand_capacity)
        group = index.contig_of_device(seeds[1], seeds[3]) if index.contigs is not None else None
        chain = self.chain_anchors_device(seeds[4], seeds[5], *seeds[:4], max_cand, max_pred, max_dist, bw, pen_gap, pen_skip, out=chain_out, group=group)
        ranked = self.rank_chains_device(seeds[5], *seeds[:4], chain[5], chain[6], chain[7], strands, max_cand, max_chains, min_score, min_cnt, mask_level,
                                         anchors=True)
        jobs = self.expand_chains_device(queries, q_start, q_len, ranked[6], ranked[0], ranked[1], *ranked[2:6], max_chains, keep_secondary, job_capacity)
        locate = self.locate_window_contigs_device if index.contigs is not None else self.locate_window_device
        window = locate(index, jobs[4], jobs[5], jobs[6], jobs[7], jobs[8], slack, max_tl)
        dist_t, dist_q = (max_dist, max_dist) if np.isscalar(max_dist) else max_dist
        aln = self.align_chain_device(index.ref, window[0], window[1], jobs[9], jobs[3], jobs[4], jobs[5], window[2], jobs[7], jobs[8], max_tl, max_ql,
                                      dist_t, dist_q, band, zdrop, parameters, **align)
        described = self.describe_device(index.ref, window[0], window[1], jobs[9], jobs[3], jobs[4], aln[0], aln[4], stride, aln[5], aln[6], md_stride,
                                         xcigar_stride, binary, xcigar=xcigar)
        lines = self.classify_alignments_device(jobs[1], jobs[2], aln[0], aln[6], parameters[0], min_score, mask_level)
        return seeds, chain, ranked, jobs, window, aln, described, lines

    def map_reads_all(self, index, reads, band=64, zdrop=-1, parameters=GATK_PARAMETERS, slack=200, strands=2, max_tl=None, extended=False, **stages):
        """``map_reads_all_device`` over a list of byte strings.  Returns AllMapResult, per read: ``n_lines`` and ``lines``, a list in
        line order (the primary first) of Line(ref_beg, ref_end, strand, score, cigar, q_beg, q_end, flag, mapq, parent, nm, n_match,
        block_len, md, xcigar, rid, rname, status): the alignment spans [ref_beg, ref_end) -- counted from the start of the line's
        contig where the index has contigs, ``rid`` / ``rname`` set then and None otherwise --, ``cigar``, ``q_beg`` / ``q_end`` are
        those of the ORIENTED read (what lies outside is a soft clip), ``flag`` has 0x10, 0x100 (secondary) and 0x800
        (supplementary), ``parent`` is the place in the list of the line this one is secondary to (its own otherwise), ``md`` is
        bytes and ``xcigar`` the = / X CIGAR with ``extended`` (None otherwise).  An unmapped read has no lines.  ``formats.
        write_sam_all`` / ``write_paf_all`` take the result as it is."""
        import torch

        dev = torch.device("cuda", self._device)
        n, packed, max_tl, max_ql, stride = _map_setup(reads, dev, slack, max_tl, stages)
        _, _, _, jobs, window, aln, desc, lines = self.map_reads_all_device(index, *packed, max_tl, max_ql, band, zdrop, parameters, slack=slack, strands=strands,
                                                                            cigar_stride=stride, xcigar=bool(extended), **stages)
        torch.cuda.synchronize(dev)
        return self._all_result(index, n, stride, jobs, window, aln, desc, lines, extended)

    @staticmethod
    def _all_result(index, n, stride, jobs, window, aln, desc, lines, extended):
        """The device tuples of ``map_reads_all_device``, read back (the stream is done) -> AllMapResult."""
        job_start, job = jobs[1].cpu().numpy(), jobs[2].cpu().numpy()
        cap = job.shape[0]
        t_start, rec, ln, st = window[0].cpu().numpy(), aln[0].cpu().numpy(), aln[5].cpu().numpy(), aln[6].cpu().numpy()
        cg = aln[4].cpu().numpy().reshape(cap, stride)
        stats, dst, md = desc[0].cpu().numpy().reshape(cap, 8), desc[3].cpu().numpy(), desc[1].cpu().numpy().reshape(cap, -1)
        xc = desc[2].cpu().numpy().reshape(cap, -1) if extended else None
        line, n_lines = lines[0].cpu().numpy(), lines[1].cpu().numpy()
        contigs = index.contigs
        rid = window[4].cpu().numpy() if contigs is not None else None
        out = []
        for p in range(n):
            mine = [j for j in range(int(job_start[p]), int(job_start[p + 1])) if line[j, 0] >= 0]
            mine.sort(key=lambda j: line[j, 0])
            place = {j: k for k, j in enumerate(mine)}
            rows = []
            for j in mine:
                if dst[j] != 0:  # the alignment stands and its description does not: a text beyond its stride
                    raise _lib.MglSwError(int(dst[j]), f"describing read {p}")
                r = int(rid[j]) if rid is not None else None
                origin = int(contigs.starts[r]) if r is not None else 0
                nm = int(stats[j, 1] + stats[j, 2] + stats[j, 3])
                rows.append(Line(int(t_start[j] + rec[j, 1]) - origin, int(t_start[j] + rec[j, 2]) - origin, int(job[j, 2]), int(rec[j, 0]),
                                 cg[j, :ln[j]].tobytes().decode(), int(rec[j, 3]), int(rec[j, 4]), int(line[j, 1]), int(line[j, 2]), place[int(line[j, 3])], nm,
                                 int(stats[j, 0]), int(stats[j, 0]) + nm, md[j, :stats[j, 6]].tobytes(), xc[j, :stats[j, 7]].tobytes().decode() if extended else None,
                                 r, contigs.names[r] if r is not None else None, int(st[j])))
            out.append(rows)
        return AllMapResult(n_lines.astype(np.int32), out)

    def map_reads_ranked_device(self, index, queries, q_start, q_len, max_tl, max_ql, band, zdrop, parameters=GATK_PARAMETERS, strands=2, max_cand=4096,
                                cand_capacity=None, seed_out=None, chain_out=None, max_chains=4, min_score=40, min_cnt=3, mask_level=128, rank_anchors=False,
                                rank_out=None, **stages):
        """``map_reads_device`` with the chain stage's f and pred kept and ``rank_chains_device`` on them, on the current stream,
        nothing read back and nothing synchronised in between: the strand choice, the window and the alignment are
        ``map_reads_device``'s own, unchanged.  ``stages``: its further arguments.  Returns its five tuples and the ranking's:
        (seeds, chain, chosen, window, aln, ranked).  A ranked chain's t_beg / t_end are positions of the reference as they stand,
        its q_beg / q_end those of its strand's oriented read."""
        import torch

        n = int(q_start.numel())
        dev = queries.device
        if chain_out is None:  # the chain stage's tuple with f and pred in it: sized as map_reads_device sizes the seed stage's
            rows = max(int(strands), 0) * n
            total = int(seed_out[1].numel()) if seed_out is not None else cand_capacity if cand_capacity is not None else min(rows * int(max_cand), 1 << 30)
            new = _alloc(dev)
            chain_out = (new(rows + 1, torch.int64), new(total), new(total), new(total), new(rows), new(total), new(total), new(rows))
        assert chain_out[5] is not None and chain_out[6] is not None, "chain_out needs f and pred (chain_anchors_device(dp=True))"
        seeds, chain, chosen, window, aln = self.map_reads_device(index, queries, q_start, q_len, max_tl, max_ql, band, zdrop, parameters, strands=strands,
                                                                  max_cand=max_cand, cand_capacity=cand_capacity, seed_out=seed_out, chain_out=chain_out,
                                                                  **stages)
        ranked = self.rank_chains_device(seeds[5], *seeds[:4], chain[5], chain[6], chain[7], strands, max_cand, max_chains, min_score, min_cnt, mask_level,
                                         anchors=rank_anchors, out=rank_out)
        return seeds, chain, chosen, window, aln, ranked

    def map_reads_ranked(self, index, reads, band=64, zdrop=-1, parameters=GATK_PARAMETERS, slack=200, strands=2, max_tl=None, **stages):
        """``map_reads_ranked_device`` over a list of byte strings: ``map_reads`` with a mapping quality.  Returns RankedMapResult:
        MapResult's fields as ``map_reads`` gives them, and per read ``mapq`` (that of its first ranked chain, which is the chain
        that was aligned; 0 for a read without ranked chains, whether it was aligned or not), ``n_chains`` and ``secondary``: the
        ranked chains behind the first as (ref_beg, ref_end, strand, score, parent) -- parent is the rank of the primary chain it
        is secondary to, or its own rank where it is primary on another part of the read.  They are reported, not aligned."""
        import torch

        dev = torch.device("cuda", self._device)
        n, packed, max_tl, max_ql, stride = _map_setup(reads, dev, slack, max_tl, stages)
        _, _, chosen, window, aln, ranked = self.map_reads_ranked_device(index, *packed, max_tl, max_ql, band, zdrop, parameters, strands=strands,
                                                                         slack=slack, cigar_stride=stride, **stages)
        torch.cuda.synchronize(dev)
        fields, _, _, contig = _map_fields(n, stride, chosen, window, aln, index)
        mapq, nc, secondary = _rank_fields(n, ranked)
        if contig:
            return ContigRankedMapResult(*fields, mapq, nc, _contig_secondary(index, secondary), *contig)
        return RankedMapResult(*fields, mapq, nc, secondary)

    def describe_device(self, targets, t_start, t_len, queries, q_start, q_len, aln, cigar, cigar_stride, cigar_len, status_in=None, md_stride=None,
                        xcigar_stride=None, binary_cigar=False, md=True, xcigar=True, out=None):
        """mgl_sw_describe_alignments_batch_device on device tensors: the six sequence tensors, the records [n, 8], the CIGAR bytes
        [n * cigar_stride] and their lengths as ``align_chain_device`` or ``extend_seed_device`` took and wrote them, and optionally
        their status (an alignment with a non-zero one is not read); enqueued on the current stream, not synchronised.  Returns
        (stats [n, 8] int32 -- mgl_sw_alignment_stats' fields --, md bytes [n * md_stride] or None, xcigar bytes [n * xcigar_stride]
        or None, status [n]) tensors; without ``md`` / ``xcigar`` that text is not written and its length still is (a sizing pass).
        The strides default to ``cigar_stride``; a text that does not fit is MGL_SW_ERR_CIGAR_OVERFLOW in the status.  ``out``: such
        a tuple to write into (its status may be None), whose text tensors decide what is written."""
        import torch

        ctx = self._ensure()
        n = int(t_start.numel())
        dev = targets.device
        md_stride = int(cigar_stride if md_stride is None else md_stride)
        xcigar_stride = int(cigar_stride if xcigar_stride is None else xcigar_stride)
        if out is None:
            new = _alloc(dev)
            out = (new((n, 8)), new(n * max(md_stride, 0), torch.uint8) if md else None, new(n * max(xcigar_stride, 0), torch.uint8) if xcigar else None, new(n))
        stats, mdt, xct, st = out
        assert stats.numel() >= 8 * n and (mdt is None or mdt.numel() >= n * md_stride) and (xct is None or xct.numel() >= n * xcigar_stride)
        ptr = _ptrs(dev)
        rc = _lib.lib().mgl_sw_describe_alignments_batch_device(
            ctx, torch.cuda.current_stream(dev).cuda_stream, n, ptr(targets), ptr(t_start), ptr(t_len), ptr(queries), ptr(q_start), ptr(q_len), ptr(aln),
            ptr(cigar), int(cigar_stride), ptr(cigar_len), ptr(status_in), ptr(stats), ptr(mdt), md_stride, ptr(xct), xcigar_stride, ptr(st),
            _lib.FLAG_BINARY_CIGAR if binary_cigar else 0)
        _check(rc, ctx)
        return out

    def describe(self, refs, alts, cigars, spans=None, binary_cigar=False, return_status=False):
        """mgl_sw_describe_alignments_batch_device over lists: ``cigars[k]`` (text, M / I / D) lays ``refs[k][t_beg:t_end]`` against
        ``alts[k][q_beg:q_end]``, ``spans[k]`` = (t_beg, t_end, q_beg, q_end), by default the whole of both (tests/describe_textbook.py).
        NOT a reference function.  A sizing pass finds the longest texts, a second call writes them.  Returns ([AlignmentStats], [md
        bytes], [extended CIGAR text]); with ``binary_cigar`` the CIGARs travel in the BAM encoding both ways (the result is text all
        the same); with ``return_status`` also the status array, and no exception for an alignment's status."""
        import torch

        from . import formats

        dev = torch.device("cuda", self._device)
        n, packed, _ = _pack_pairs(refs, alts, dev, 16, False)
        assert len(cigars) == n
        if binary_cigar:
            rows = [formats.cigar_elements_to_binary(formats.cigar_text_to_elements(c)).astype("<u4").tobytes() for c in cigars]
        else:
            rows = [c.encode() if isinstance(c, str) else bytes(c) for c in cigars]
        stride = (max([len(r) for r in rows] + [4]) + 3) // 4 * 4
        slots = np.zeros((n, stride), np.uint8)
        for k, r in enumerate(rows):
            slots[k, :len(r)] = np.frombuffer(r, np.uint8)
        if spans is None:
            spans = [(0, len(t), 0, len(q)) for t, q in zip(refs, alts)]
        rec = np.zeros((n, 8), np.int32)
        rec[:, 1:5] = np.asarray(spans, np.int32).reshape(n, 4)
        g = lambda x: _upload(x, dev)  # noqa: E731
        args = (*packed[:6], g(rec), g(slots.reshape(-1)), stride, g(np.asarray([len(r) for r in rows], np.int32)))
        sized = self.describe_device(*args, binary_cigar=binary_cigar, md=False, xcigar=False)
        need = _fetch(sized, dev, True)[0].reshape(n, 8)
        ms, xs = max(int(need[:, 6].max(initial=1)), 1), (max(int(need[:, 7].max(initial=4)), 4) + 3) // 4 * 4
        stats, md, xc, st = _fetch(self.describe_device(*args, md_stride=ms, xcigar_stride=xs, binary_cigar=binary_cigar), dev, return_status)
        stats, md, xc = stats.reshape(n, 8), md.reshape(n, ms), xc.reshape(n, xs)
        mds = [md[k, :stats[k, 6]].tobytes() for k in range(n)]
        if binary_cigar:
            xcs = [formats.cigar_binary_to_text(np.frombuffer(xc[k, :stats[k, 7]].tobytes(), "<u4")) for k in range(n)]
        else:
            xcs = [xc[k, :stats[k, 7]].tobytes().decode() for k in range(n)]
        res = ([AlignmentStats(*(int(v) for v in row)) for row in stats], mds, xcs)
        return res + (st,) if return_status else res

    def map_reads_described_device(self, index, queries, q_start, q_len, max_tl, max_ql, band, zdrop, parameters=GATK_PARAMETERS, md_stride=None,
                                   xcigar_stride=None, xcigar=True, describe_out=None, **stages):
        """``map_reads_ranked_device`` and ``describe_device`` behind it on the index's reference, the read's window, the oriented
        reads and the alignment's own tensors, on the current stream, nothing read back and nothing synchronised in between.  A read
        the alignment refused (unmapped ones among them) keeps that status and has an all-zero record.  ``stages``: the further
        arguments of ``map_reads_ranked_device``.  Returns its six tuples and ``describe_device``'s:
        (seeds, chain, chosen, window, aln, ranked, described)."""
        binary = bool(stages.get("binary_cigar", False))
        if stages.get("cigar_stride") is None:
            stages["cigar_stride"] = _default_stride(max_tl, max_ql, binary)
        stride = int(stages["cigar_stride"])
        seeds, chain, chosen, window, aln, ranked = self.map_reads_ranked_device(index, queries, q_start, q_len, max_tl, max_ql, band, zdrop, parameters, **stages)
        oriented = chosen[1] if chosen is not None else queries
        described = self.describe_device(index.ref, window[0], window[1], oriented, q_start, q_len, aln[0], aln[4], stride, aln[5], aln[6], md_stride,
                                         xcigar_stride, binary, xcigar=xcigar, out=describe_out)
        return seeds, chain, chosen, window, aln, ranked, described

    def map_reads_described(self, index, reads, band=64, zdrop=-1, parameters=GATK_PARAMETERS, slack=200, strands=2, max_tl=None, extended=False, **stages):
        """``map_reads_described_device`` over a list of byte strings: ``map_reads_ranked`` with what a SAM or PAF record needs
        (``formats.write_sam`` / ``write_paf`` take the result as it is).  Returns DescribedMapResult: RankedMapResult's fields as
        ``map_reads_ranked`` gives them, and per read ``q_beg`` / ``q_end`` (the aligned part of the ORIENTED read; what lies outside
        is a soft clip), ``nm`` (mismatches + inserted + deleted bases), ``n_match``, ``block_len`` (n_match + nm), ``md`` (a list of
        bytes) and, with ``extended``, ``xcigars`` (the = / X CIGARs; None otherwise).  An unmapped or refused read has zeros, an
        empty MD and an empty extended CIGAR."""
        import torch

        dev = torch.device("cuda", self._device)
        n, packed, max_tl, max_ql, stride = _map_setup(reads, dev, slack, max_tl, stages)
        _, _, chosen, window, aln, ranked, desc = self.map_reads_described_device(index, *packed, max_tl, max_ql, band, zdrop, parameters, strands=strands,
                                                                                  slack=slack, cigar_stride=stride, xcigar=bool(extended), **stages)
        torch.cuda.synchronize(dev)
        fields, ok, rec, contig = _map_fields(n, stride, chosen, window, aln, index)
        stats, dst = desc[0].cpu().numpy().reshape(n, 8), desc[3].cpu().numpy()
        over = np.flatnonzero(ok & (dst != 0))
        if over.size:  # the alignment stands and its description does not: a text beyond its stride
            raise _lib.MglSwError(int(dst[over[0]]), f"describing read {int(over[0])}")
        md = desc[1].cpu().numpy().reshape(n, -1)
        mds = [md[p, :stats[p, 6]].tobytes() for p in range(n)]
        nm = (stats[:, 1] + stats[:, 2] + stats[:, 3]).astype(np.int32)
        z = lambda x: np.where(ok, x, 0).astype(np.int32)  # noqa: E731
        mapq, nc, secondary = _rank_fields(n, ranked)
        if contig:
            secondary = _contig_secondary(index, secondary)
        return (ContigDescribedMapResult if contig else DescribedMapResult)(
            *fields, mapq, nc, secondary, z(rec[:, 3]), z(rec[:, 4]), nm, stats[:, 0].astype(np.int32), (stats[:, 0] + nm).astype(np.int32), mds,
            CigarColumn(desc[2].cpu().numpy().reshape(n, -1), stats[:, 7].astype(np.int32)) if extended else None, *contig)

    def pileup_device(self, targets, t_start, t_len, queries, q_start, q_len, aln, cigar, cigar_stride, cigar_len, status_in=None, select=None,
                      region=None, counts=None, binary_cigar=False, out=None):
        """mgl_sw_pileup_alignments_batch_device on device tensors: ``describe_device``'s first eleven arguments, optionally a
        ``select`` [n] int32 (an alignment with a zero is not counted) and ``region`` = (beg, len) in byte offsets of ``targets``, by
        default the whole of it (tests/pileup_textbook.py); enqueued on the current stream, not synchronised.  Returns (counts
        [8, region_len] int32 -- the uint32 bits; planes A C G T other, deleted, insertions, inserted bases --, status [n]).  The entry
        ADDS: ``counts=None`` allocates zeros, a tensor given accumulates.  ``out``: a (counts, status) tuple to write into (its
        status may be None)."""
        import torch

        ctx = self._ensure()
        n = int(t_start.numel())
        dev = targets.device
        beg, length = (0, int(targets.numel())) if region is None else (int(region[0]), int(region[1]))
        if out is None:
            out = (torch.zeros((8, max(length, 0)), dtype=torch.int32, device=dev) if counts is None else counts, _alloc(dev)(n))
        table, st = out
        assert table.numel() >= 8 * length and table.dtype == torch.int32 and table.is_contiguous() and (st is None or st.numel() >= n)
        ptr = _ptrs(dev)
        rc = _lib.lib().mgl_sw_pileup_alignments_batch_device(
            ctx, torch.cuda.current_stream(dev).cuda_stream, n, ptr(targets), ptr(t_start), ptr(t_len), ptr(queries), ptr(q_start), ptr(q_len), ptr(aln),
            ptr(cigar), int(cigar_stride), ptr(cigar_len), ptr(status_in), ptr(select), beg, length, ptr(table), ptr(st),
            _lib.FLAG_BINARY_CIGAR if binary_cigar else 0)
        _check(rc, ctx)
        return out

    def pileup_sites_device(self, counts, ref, region_beg=0, min_depth=4, min_alt=2, min_frac=64, site_capacity=None, call=True, flags=True, out=None):
        """mgl_sw_pileup_sites_device on device tensors: ``pileup_device``'s counts [8, region_len] and the reference bytes they were
        piled up over (position i of the table is ``ref[region_beg + i]``); enqueued on the current stream, not synchronised.  Returns
        (call [region_len] uint8 or None, flags [region_len] uint8 or None, sites [site_capacity, 8] int32 -- mgl_sw_site's fields,
        in position order --, n_sites [1] int64: the total, those beyond the capacity included).  ``site_capacity`` defaults to
        region_len; 0 is a sizing pass.  ``out``: such a tuple to write into, whose tensors decide what is written."""
        import torch

        ctx = self._ensure()
        dev = counts.device
        length = int(counts.numel()) // 8
        if out is None:
            cap = length if site_capacity is None else int(site_capacity)
            new = _alloc(dev)
            out = (new(length, torch.uint8) if call else None, new(length, torch.uint8) if flags else None, new((max(cap, 0), 8)), new(1, torch.int64))
        cl, fl, sites, ns = out
        cap = (int(sites.numel()) // 8 if sites is not None else 0) if site_capacity is None else int(site_capacity)
        assert counts.is_contiguous() and (sites is None or sites.numel() >= 8 * cap) and all(x is None or x.numel() >= length for x in (cl, fl))
        assert ref.numel() >= int(region_beg) + length
        ptr = _ptrs(dev)
        rc = _lib.lib().mgl_sw_pileup_sites_device(ctx, torch.cuda.current_stream(dev).cuda_stream, ptr(counts), length, ptr(ref), int(region_beg),
                                                   int(min_depth), int(min_alt), int(min_frac), ptr(cl), ptr(fl), ptr(sites), cap, ptr(ns))
        _check(rc, ctx)
        return out

    def pileup(self, refs, alts, cigars, spans=None, positions=None, region=None, binary_cigar=False, return_status=False):
        """mgl_sw_pileup_alignments_batch_device over lists: ``describe``'s alignments, ``positions[k]`` the absolute position of
        ``refs[k][0]`` (by default the targets lie end to end), ``region`` = (beg, len), by default from 0 to the end of the last
        target.  NOT a reference function.  Returns counts, a numpy uint32 array [8, region_len]; with ``return_status`` also the
        status array, and no exception for an alignment's status."""
        import torch

        from . import formats

        dev = torch.device("cuda", self._device)
        n, packed, _ = _pack_pairs(refs, alts, dev, 16, False)
        assert len(cigars) == n
        if binary_cigar:
            rows = [formats.cigar_elements_to_binary(formats.cigar_text_to_elements(c)).astype("<u4").tobytes() for c in cigars]
        else:
            rows = [c.encode() if isinstance(c, str) else bytes(c) for c in cigars]
        stride = (max([len(r) for r in rows] + [4]) + 3) // 4 * 4
        slots = np.zeros((n, stride), np.uint8)
        for k, r in enumerate(rows):
            slots[k, :len(r)] = np.frombuffer(r, np.uint8)
        if spans is None:
            spans = [(0, len(t), 0, len(q)) for t, q in zip(refs, alts)]
        rec = np.zeros((n, 8), np.int32)
        rec[:, 1:5] = np.asarray(spans, np.int32).reshape(n, 4)
        g = lambda x: _upload(x, dev)  # noqa: E731
        t_start = packed[1] if positions is None else g(np.asarray(positions, np.int64))
        if region is None:
            ends = [int(p) + len(t) for p, t in zip(t_start.cpu().numpy(), refs)]
            region = (0, max(ends + [1]))
        got = self.pileup_device(packed[0], t_start, packed[2], *packed[3:6], g(rec), g(slots.reshape(-1)), stride,
                                 g(np.asarray([len(r) for r in rows], np.int32)), region=region, binary_cigar=binary_cigar)
        counts, st = _fetch(got, dev, return_status)
        counts = counts.view(np.uint32)
        return (counts, st) if return_status else counts

    def map_reads_pileup_device(self, index, queries, q_start, q_len, max_tl, max_ql, band, zdrop, parameters=GATK_PARAMETERS, counts=None, min_mapq=0,
                                **stages):
        """``map_reads_all_device`` and ``pileup_device`` behind it over [0, ref_len), on the current stream, nothing read back and
        nothing synchronised in between.  The pileup takes exactly the tensors ``map_reads_all_device`` hands ``describe_device``, the
        alignment status, and a select made on the device from the lines: a job is counted where it is a line (order >= 0), not a
        secondary one (flag & 0x100 == 0) and its mapq is at least ``min_mapq``.  (The line rows of the empty jobs are uninitialised;
        their alignment status is non-zero, and the status is what excludes them.)  ``counts``: a table to add into, so that batches
        accumulate.  ``stages``: the further arguments of ``map_reads_all_device``.  Returns its eight tuples and (counts, status)."""
        binary = bool(stages.get("binary_cigar", False))
        if stages.get("cigar_stride") is None:
            stages["cigar_stride"] = _default_stride(max_tl, max_ql, binary)
        stride = int(stages["cigar_stride"])
        res = self.map_reads_all_device(index, queries, q_start, q_len, max_tl, max_ql, band, zdrop, parameters, **stages)
        jobs, window, aln, lines = res[3], res[4], res[5], res[7][0]
        select = _counted_lines(lines, min_mapq)
        piled = self.pileup_device(index.ref, window[0], window[1], jobs[9], jobs[3], jobs[4], aln[0], aln[4], stride, aln[5], aln[6], select,
                                   (0, int(index.info.ref_len)), counts, binary)
        return res + (piled,)

    def map_reads_pileup(self, index, reads, band=64, zdrop=-1, parameters=GATK_PARAMETERS, slack=200, strands=2, max_tl=None, counts=None, min_mapq=0,
                         **stages):
        """``map_reads_pileup_device`` over a list of byte strings.  Returns (AllMapResult as ``map_reads_all`` gives it, counts: a
        numpy uint32 array [8, ref_len]).  ``counts``: a device table of an earlier batch to add into."""
        import torch

        dev = torch.device("cuda", self._device)
        n, packed, max_tl, max_ql, stride = _map_setup(reads, dev, slack, max_tl, stages)
        res = self.map_reads_pileup_device(index, *packed, max_tl, max_ql, band, zdrop, parameters, counts=counts, min_mapq=min_mapq, slack=slack,
                                           strands=strands, cigar_stride=stride, xcigar=False, **stages)
        torch.cuda.synchronize(dev)
        return self._all_result(index, n, stride, *res[3:8], False), res[8][0].cpu().numpy().view(np.uint32)

    def pileup_insertions_device(self, targets, t_start, t_len, queries, q_start, q_len, aln, cigar, cigar_stride, cigar_len, sites, n_sites,
                                 status_in=None, select=None, region_beg=0, max_ins=16, ins=None, binary_cigar=False, out=None):
        """mgl_sw_pileup_insertions_batch_device on device tensors: ``pileup_device``'s alignments (give it exactly the tensors,
        status and select the pileup took) and ``pileup_sites_device``'s sites [site_capacity, 8] and n_sites [1] int64, which stay on
        the device (tests/calls_textbook.py); enqueued on the current stream, not synchronised.  Returns (ins [site_capacity,
        6 * max_ins + 1] int32 -- the uint32 bits: word 0 the insertions longer than max_ins, word L those of L bases, then five
        channel counts per column --, status [n]).  The entry ADDS: ``ins=None`` allocates zeros, a tensor given accumulates.
        ``out``: an (ins, status) tuple to write into (its status may be None)."""
        import torch

        ctx = self._ensure()
        n = int(t_start.numel())
        dev = targets.device
        cap = int(sites.numel()) // 8
        width = 6 * int(max_ins) + 1
        if out is None:
            out = (torch.zeros((max(cap, 0), width), dtype=torch.int32, device=dev) if ins is None else ins, _alloc(dev)(n))
        table, st = out
        assert table.numel() >= cap * width and table.dtype == torch.int32 and table.is_contiguous() and sites.is_contiguous()
        assert st is None or st.numel() >= n
        ptr = _ptrs(dev)
        rc = _lib.lib().mgl_sw_pileup_insertions_batch_device(
            ctx, torch.cuda.current_stream(dev).cuda_stream, n, ptr(targets), ptr(t_start), ptr(t_len), ptr(queries), ptr(q_start), ptr(q_len), ptr(aln),
            ptr(cigar), int(cigar_stride), ptr(cigar_len), ptr(status_in), ptr(select), int(region_beg), ptr(sites), ptr(n_sites), cap, int(max_ins),
            ptr(table), ptr(st), _lib.FLAG_BINARY_CIGAR if binary_cigar else 0)
        _check(rc, ctx)
        return out

    def genotype_sites_device(self, counts, ref, sites, n_sites, ins=None, region_beg=0, max_ins=16, max_del=64, error_phred=20, costs=None,
                              call_capacity=None, out=None):
        """mgl_sw_genotype_sites_device on device tensors: ``pileup_device``'s counts, the reference bytes, ``pileup_sites_device``'s
        sites and n_sites and ``pileup_insertions_device``'s table (None: no insertion is called); enqueued on the current stream, not
        synchronised.  ``costs``: (cost_match, cost_het, cost_error), by default ``genotype_costs(error_phred)``.  Returns (calls
        [call_capacity, 16] int32 -- mgl_sw_call's fields, in site order --, n_calls [1] int64: the total, those beyond the capacity
        included, seq [call_capacity, max_ins] uint8: an insertion call's bases and zeros behind them).  ``call_capacity`` defaults to
        three per site slot; 0 is a sizing pass.  ``out``: such a tuple to write into, whose tensors decide what is written."""
        import torch

        ctx = self._ensure()
        dev = counts.device
        length = int(counts.numel()) // 8
        slots = int(sites.numel()) // 8
        if out is None:
            cap = 3 * slots if call_capacity is None else int(call_capacity)
            new = _alloc(dev)
            out = (new((max(cap, 0), 16)), new(1, torch.int64), new((max(cap, 0), int(max_ins)), torch.uint8))
        calls, nc, seq = out
        cap = (int(calls.numel()) // 16 if calls is not None else 0) if call_capacity is None else int(call_capacity)
        assert counts.is_contiguous() and sites.is_contiguous() and (calls is None or calls.numel() >= 16 * cap)
        assert seq is None or seq.numel() >= cap * int(max_ins)
        assert ins is None or (ins.is_contiguous() and ins.numel() >= slots * (6 * int(max_ins) + 1))
        assert ref.numel() >= int(region_beg) + length
        ptr = _ptrs(dev)
        rc = _lib.lib().mgl_sw_genotype_sites_device(ctx, torch.cuda.current_stream(dev).cuda_stream, ptr(counts), length, ptr(ref), int(region_beg), ptr(sites),
                                                     ptr(n_sites), slots, ptr(ins), int(max_ins), int(max_del), *_entry_costs(costs, error_phred), ptr(calls),
                                                     cap, ptr(nc), ptr(seq))
        _check(rc, ctx)
        return out

    def map_reads_calls_device(self, index, queries, q_start, q_len, max_tl, max_ql, band, zdrop, parameters=GATK_PARAMETERS, min_mapq=0, min_depth=4,
                               min_alt=2, min_frac=64, site_capacity=None, max_ins=16, max_del=64, error_phred=20, costs=None, call_capacity=None,
                               **stages):
        """``map_reads_pileup_device``, then ``pileup_sites_device`` over its table, then ``pileup_insertions_device`` on exactly the
        tensors the pileup took, then ``genotype_sites_device``: reads in, calls out, on the current stream, nothing read back and
        nothing synchronised in between.  ONE batch: the insertion evidence needs the alignments AFTER the sites are known, and a
        batch's alignments are gone when the next one is mapped.  ``site_capacity`` defaults to min(ref_len, 2^18) site slots.  Returns ``map_reads_pileup_device``'s nine tuples, then the sites'
        tuple, the insertions' (ins, status) and the genotype's (calls, n_calls, seq)."""
        binary = bool(stages.get("binary_cigar", False))
        if stages.get("cigar_stride") is None:
            stages["cigar_stride"] = _default_stride(max_tl, max_ql, binary)
        stride = int(stages["cigar_stride"])
        res = self.map_reads_pileup_device(index, queries, q_start, q_len, max_tl, max_ql, band, zdrop, parameters, min_mapq=min_mapq, **stages)
        jobs, window, aln, lines, counts = res[3], res[4], res[5], res[7][0], res[8][0]
        select = _counted_lines(lines, min_mapq)
        if site_capacity is None:  # (a row of the insertion table per slot: not one per position of the reference)
            site_capacity = min(int(index.info.ref_len), 1 << 18)
        found = self.pileup_sites_device(counts, index.ref, 0, min_depth, min_alt, min_frac, site_capacity, call=False, flags=False)
        ins = self.pileup_insertions_device(index.ref, window[0], window[1], jobs[9], jobs[3], jobs[4], aln[0], aln[4], stride, aln[5], found[2], found[3],
                                            aln[6], select, 0, max_ins, None, binary)
        called = self.genotype_sites_device(counts, index.ref, found[2], found[3], ins[0], 0, max_ins, max_del, error_phred, costs, call_capacity)
        return res + (found, ins, called)

    def map_reads_calls(self, index, reads, band=64, zdrop=-1, parameters=GATK_PARAMETERS, slack=200, strands=2, max_tl=None, min_mapq=0, min_depth=4,
                        min_alt=2, min_frac=64, site_capacity=None, max_ins=16, max_del=64, error_phred=20, costs=None, **stages):
        """``map_reads_calls_device`` over a list of byte strings.  Returns (AllMapResult as ``map_reads_all`` gives it, counts: a numpy
        uint32 array [8, ref_len], calls: a list of ``Call`` in position order, whose REF / ALT bases are built here on the host from
        the reference, the call's length and its sequence row).  It handles ONE batch: the insertion evidence needs the alignments
        after the sites are known, so batches cannot accumulate into one call set without keeping their alignments."""
        import torch

        dev = torch.device("cuda", self._device)
        n, packed, max_tl, max_ql, stride = _map_setup(reads, dev, slack, max_tl, stages)
        res = self.map_reads_calls_device(index, *packed, max_tl, max_ql, band, zdrop, parameters, min_mapq=min_mapq, min_depth=min_depth, min_alt=min_alt,
                                          min_frac=min_frac, site_capacity=site_capacity, max_ins=max_ins, max_del=max_del, error_phred=error_phred,
                                          costs=costs, slack=slack, strands=strands, cigar_stride=stride, xcigar=False, **stages)
        torch.cuda.synchronize(dev)
        found, called = res[9], res[11]
        total, slots = int(found[3][0]), int(found[2].shape[0])
        if total > slots:
            raise _lib.MglSwError(_lib.ERR_NOMEM, f"{total} candidate sites, site_capacity {slots}")
        n_calls = int(called[1][0])
        ref = index.ref.cpu().numpy().tobytes()
        rows = called[0].cpu().numpy()[:n_calls]
        seq = called[2].cpu().numpy()[:n_calls]
        return (self._all_result(index, n, stride, *res[3:8], False), res[8][0].cpu().numpy().view(np.uint32),
                [make_call(r, s, ref) for r, s in zip(rows, seq)])

    def align_packed_2bit(self, target_bases, target_base_count, t_start, t_len, query_bases, query_base_count, q_start, q_len,
                          max_tl, max_ql, parameters=GATK_PARAMETERS, overhang_strategy=SWOverhangStrategy.SOFTCLIP, cigar_stride=None,
                          out=None):
        """mgl_sw_align_batch_2bit: 2-bit packed bases in host memory (four per byte), pair k = t_len[k] bases from base index
        t_start[k] against q_len[k] from q_start[k]; t_len = q_len = None: every pair max_tl x max_ql.  ``out``: (offsets,
        scores, cigars, lengths) arrays to write into (e.g. registered ones) instead of fresh ones."""
        ctx = self._ensure()
        n = len(t_start)
        uniform = t_len is None and q_len is None
        t_start = np.ascontiguousarray(t_start, dtype=np.int64)
        q_start = np.ascontiguousarray(q_start, dtype=np.int64)
        if not uniform:
            t_len = np.ascontiguousarray(t_len, dtype=np.int32)
            q_len = np.ascontiguousarray(q_len, dtype=np.int32)
        if cigar_stride is None:
            cigar_stride = max(16, 2 * max(max_tl, max_ql))
        if out is None:
            out = (np.empty(n, np.int32), np.empty((n, 6), np.int32), np.empty(n * cigar_stride, np.uint8), np.empty(n, np.int32))
        off, sc, cg, ln = out
        p = SWParameters(*parameters)
        rc = _lib.lib().mgl_sw_align_batch_2bit(
            ctx, n, target_bases.ctypes.data, int(target_base_count), t_start.ctypes.data, None if uniform else t_len.ctypes.data,
            query_bases.ctypes.data, int(query_base_count), q_start.ctypes.data, None if uniform else q_len.ctypes.data, int(max_tl),
            int(max_ql), p.match, p.mismatch, p.gap_open, p.gap_extend, int(overhang_strategy), off.ctypes.data, sc.ctypes.data,
            cg.ctypes.data, cigar_stride, ln.ctypes.data, None, _lib.FLAG_UNIFORM_GEOMETRY if uniform else 0)
        _check(rc, ctx)
        return BatchResult(off, sc, CigarColumn(cg.reshape(n, cigar_stride), ln), ln)

    def register_host_buffer(self, array):
        """Page-lock a numpy array for this context (mgl_sw_register_host_buffer): the host entries then copy from / into it
        asynchronously.  Keep the array alive and unregister it before it is freed."""
        _check(_lib.lib().mgl_sw_register_host_buffer(self._ensure(), array.ctypes.data, array.nbytes), self._ctx)

    def unregister_host_buffer(self, array):
        _check(_lib.lib().mgl_sw_unregister_host_buffer(self._ensure(), array.ctypes.data), self._ctx)

    def expand_slot(self, slot, tl, ql):
        """Logical backtrack matrix of pair ``slot`` of the last chunk of the last batch call."""
        btr = np.zeros((tl + 1, ql + 1), dtype=np.int32)
        _check(_lib.lib().mgl_sw_ctx_expand_slot(self._ensure(), slot, tl, ql,
                                                 btr.ctypes.data_as(C.POINTER(C.c_int32))), self._ctx)
        return btr

    def slot_layout(self, slot):
        """Traceback layout of pair ``slot`` of the last chunk (0 int32, 1 packed16, 2 lane16, 3 coop16)."""
        v = C.c_int(-1)
        _check(_lib.lib().mgl_sw_ctx_slot_layout(self._ensure(), slot, C.byref(v)), self._ctx)
        return v.value

    # -- extras the reference keeps internal -----------------------------------------------
    def set_workspace(self, nbytes):
        _check(_lib.lib().mgl_sw_ctx_set_workspace(self._ensure(), int(nbytes)))

    def set_precision(self, bits):
        """0 = per batch (packed int16 when possible), 32 = always the int32 fill kernels, 16 = like 0 but the self-checking
        16-bit long-read kernel is tried whenever its constants fit."""
        _check(_lib.lib().mgl_sw_ctx_set_precision(self._ensure(), int(bits)))

    def set_strip_kernel(self, mode):
        """Long reads, one 32-row strip per lane-half: 0 = by size, 1 = never, 2 = whenever eligible."""
        _check(_lib.lib().mgl_sw_ctx_set_strip_kernel(self._ensure(), int(mode)))

    def set_carry_memory(self, mode):
        """0 = stripe carry in LDS when the query fits, 1 = always in the HBM scratch (long-query path)."""
        _check(_lib.lib().mgl_sw_ctx_set_carry_memory(self._ensure(), int(mode)))

    def set_stripe_rows(self, rows):
        """Lanes per pair of the int32 fill kernel: 0 = by query length, 16 or 64 = forced."""
        _check(_lib.lib().mgl_sw_ctx_set_stripe_rows(self._ensure(), int(rows)))

    def set_cooperative(self, mode):
        """Long-read fill kernel (one pair per workgroup): 0 = when the query does not fit the one-wave LDS carve,
        1 = never, 2..16 = always with that many waves per pair."""
        _check(_lib.lib().mgl_sw_ctx_set_cooperative(self._ensure(), int(mode)))

    def set_lane_kernel(self, mode):
        """Packed kernel for uniform batches: 0 = by batch size, 1 = never the two-pairs-per-lane kernel, 2 = always when eligible."""
        _check(_lib.lib().mgl_sw_ctx_set_lane_kernel(self._ensure(), int(mode)))

    def set_lane_checkpoint(self, mode):
        """The lane kernel's checkpointed form (no stored traceback, the walk recomputes the blocks it crosses): 0 = default (on),
        1 = never (needed before expand_slot), 2 = on."""
        _check(_lib.lib().mgl_sw_ctx_set_lane_checkpoint(self._ensure(), int(mode)))

    def set_small_kernel(self, mode):
        """Small batches (up to 5 120 pairs of one promised geometry, 8 192 without a promise -- half where one matrix fills more than half a CU's LDS --: one wave per pair, fill + walk in one launch.
        0 = default (on, unless another kernel choice is forced), 1 = never, 2 = whenever the bounds allow."""
        _check(_lib.lib().mgl_sw_ctx_set_small_kernel(self._ensure(), int(mode)))

    def set_profiling(self, on=True):
        _check(_lib.lib().mgl_sw_ctx_set_profiling(self._ensure(), int(on)))

    def timing(self):
        t = _lib.Timing()
        _check(_lib.lib().mgl_sw_ctx_get_timing(self._ensure(), C.byref(t)))
        return t

    def check(self):
        """mgl_sw_ctx_check: what a kernel found out about itself after the (asynchronous) device entry that enqueued it returned --
        synchronise the stream first.  Raises MglSwError(ERR_DEVICE) when a persistent grid found its tile counter out of range."""
        _check(_lib.lib().mgl_sw_ctx_check(self._ensure()), self._ctx)

    @staticmethod
    def fill_kernel_name(timing):
        """Name of the fill kernel a Timing record belongs to (MGL_SW_KERNEL_*)."""
        return _lib.fill_kernel_name(timing.fill_kernel)

    @property
    def ctx(self):
        return self._ensure()

    def _ensure(self):
        if self._ctx is None:
            h = C.c_void_p()
            _check(_lib.lib().mgl_sw_ctx_create(self._device, C.byref(h)))
            self._ctx = h
        return self._ctx

    def __enter__(self):
        self._ensure()
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiGpuSmithWaterman:
    """Several GPUs from one process (mgl_sw_align_batch_multi): contiguous shards of a host batch, one per device,
    balanced by DP cells, each on its own context and host thread; results in the caller's order.
    ``devices``: HIP ordinals (an ordinal may repeat: every entry gets its own context and thread)."""

    def __init__(self, devices):
        self._devices = [int(d) for d in devices]
        arr = (C.c_int * len(self._devices))(*self._devices)
        h = C.c_void_p()
        rc = _lib.lib().mgl_sw_multi_create(len(self._devices), arr, C.byref(h))
        if rc != _lib.OK:
            raise _lib.MglSwError(rc, "mgl_sw_multi_create")
        self._h = h

    def set_workspace(self, nbytes_per_device):
        rc = _lib.lib().mgl_sw_multi_set_workspace(self._h, int(nbytes_per_device))
        if rc != _lib.OK:
            raise _lib.MglSwError(rc, "mgl_sw_multi_set_workspace")

    def align_packed(self, targets, t_off, queries, q_off, parameters=GATK_PARAMETERS,
                     overhang_strategy=SWOverhangStrategy.SOFTCLIP, cigar_stride=64, per_pair_status=False):
        L = _lib.lib()
        n = len(t_off) - 1
        targets = np.ascontiguousarray(targets, dtype=np.uint8)
        queries = np.ascontiguousarray(queries, dtype=np.uint8)
        t_off = np.ascontiguousarray(t_off, dtype=np.int64)
        q_off = np.ascontiguousarray(q_off, dtype=np.int64)
        off = np.empty(n, np.int32)
        sc = np.empty((n, 6), np.int32)
        cg = np.empty(n * cigar_stride, np.uint8)
        ln = np.empty(n, np.int32)
        st = np.zeros(n, np.int32) if per_pair_status else None
        p = SWParameters(*parameters)
        rc = L.mgl_sw_align_batch_multi(self._h, n, targets.ctypes.data, t_off.ctypes.data, queries.ctypes.data, q_off.ctypes.data,
                                        p.match, p.mismatch, p.gap_open, p.gap_extend, int(overhang_strategy), off.ctypes.data,
                                        sc.ctypes.data, cg.ctypes.data, cigar_stride, ln.ctypes.data,
                                        st.ctypes.data if st is not None else None)
        if rc != _lib.OK:
            raise _lib.MglSwError(rc, L.mgl_sw_multi_last_error(self._h).decode())
        res = BatchResult(off, sc, CigarColumn(cg.reshape(n, cigar_stride), ln), ln)
        return (res, st) if per_pair_status else res

    def align_batch(self, refs, alts, parameters=GATK_PARAMETERS, overhang_strategy=SWOverhangStrategy.SOFTCLIP, cigar_stride=64):
        td, toff = concat([bytes(x) for x in refs])
        qd, qoff = concat([bytes(x) for x in alts])
        return self.align_packed(td, toff, qd, qoff, parameters, overhang_strategy, cigar_stride)

    def last_shards(self):
        first = np.zeros(len(self._devices) + 1, np.int64)
        _lib.lib().mgl_sw_multi_last_shards(self._h, first.ctypes.data)
        return first

    def close(self):
        if self._h is not None:
            _lib.lib().mgl_sw_multi_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def align(ref, alt, parameters=GATK_PARAMETERS, overhang_strategy=SWOverhangStrategy.SOFTCLIP):
    """One pair through mgl_sw_align (thread-local context), returning (cigar, offset, ScoreMax)."""
    ref, alt = bytes(ref), bytes(alt)
    L = _lib.lib()
    cap = 12 * (len(ref) + len(alt) + 4)
    buf = C.create_string_buffer(cap)
    ln, off, ez = C.c_int(), C.c_int(), _lib.Score()
    p = SWParameters(*parameters)
    rc = L.mgl_sw_align(ref, len(ref), alt, len(alt), p.match, p.mismatch, p.gap_open, p.gap_extend,
                        int(overhang_strategy), buf, cap, C.byref(ln), C.byref(off), C.byref(ez))
    _check(rc)
    return buf.raw[: ln.value].decode(), off.value, ScoreMax(ez.mqe, ez.mqe_t, ez.max, ez.max_t, ez.max_q,
                                                            ez.seg_length)


def set_coalescing(max_batch, max_wait_us):
    """The front-ends of the one-pair entry (mgl_sw_align / alignNative): max_batch = 0 makes every call a direct call."""
    _check(_lib.lib().mgl_sw_set_coalescing(int(max_batch), int(max_wait_us)))


def set_service(slots, idle_us=0):
    """Mailboxes of the one-pair entry (one resident wave per calling thread, no launch per call): `slots` of them at most, 0 = off
    (every call through the coalescer); the service grid ends after idle_us of silence (0: keep the current value)."""
    _check(_lib.lib().mgl_sw_set_service(int(slots), int(idle_us)))


def service_stats():
    """(calls served through mailboxes, launches of the service grid) so far."""
    calls, launches = C.c_int64(), C.c_int64()
    _check(_lib.lib().mgl_sw_service_stats(C.byref(calls), C.byref(launches)))
    return calls.value, launches.value


def backtrack_matrix(ref, alt, parameters=GATK_PARAMETERS, overhang_strategy=SWOverhangStrategy.SOFTCLIP):
    """The reference's logical backtrack matrix (calculateMatrix, sw.cpp:5-146) rebuilt on the GPU."""
    ref, alt = bytes(ref), bytes(alt)
    btr = np.zeros((len(ref) + 1, len(alt) + 1), dtype=np.int32)
    ez = _lib.Score()
    p = SWParameters(*parameters)
    rc = _lib.lib().mgl_sw_backtrack_matrix(ref, len(ref), alt, len(alt), p.match, p.mismatch, p.gap_open,
                                            p.gap_extend, int(overhang_strategy),
                                            btr.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(ez))
    _check(rc)
    return btr, ScoreMax(ez.mqe, ez.mqe_t, ez.max, ez.max_t, ez.max_q, ez.seg_length)
