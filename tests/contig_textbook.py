"""The functions of mgl_sw_index_build_contigs_device, mgl_sw_index_contig_of_batch_device, mgl_sw_chain_anchors_grouped_batch_device and
mgl_sw_locate_window_contigs_batch_device (include/mgl_sw.h), stated once in plain Python on top of
index_textbook.py, chain_dp_textbook.py, rank_textbook.py, chain_textbook.py and describe_textbook.py.  Integers only.

A reference of C contigs is ONE buffer: contig c is [start[c], start[c] + len[c]), start[0] = 0, len[c] >= 1, at least one gap byte
between two contigs, the last contig ends where the buffer does, and no gap byte is a base (upper-case A, C, G, T).  The index is
index_textbook.build_index of the whole buffer: a window of w k-mer positions that straddles a gap selects among the valid positions it
sees on both sides.

contig_of(t, l): the c with start[c] <= t and t + l <= end[c]; -1 where there is none -- t < 0, l < 1, inside a gap, over a contig's end.

chain_dp_grouped: chain_dp_textbook.chain_dp where j may precede i only if group[j] == group[i] and group[i] >= 0.  Everything else --
the window of max_pred INDEX positions in the whole row, the ties, the chain's end -- is as it stands there.

locate_window_contigs: index_textbook.locate_window with, c being the contig of the read's first anchor, status 1 (BAD_ARG) for an anchor
in another contig or in none, lo = max(start[c], t0 - q0 - slack), hi = min(end[c], tK + lK + (ql - qK - lK) + slack) and rid = c for
a kept read, -1 for an unmapped or a refused one.  t_start stays a position of the buffer.
"""
import bisect

import chain_dp_textbook as ctb
import index_textbook as itb
import rank_textbook as ktb
import strand_textbook as rtb

BAD_ARG, UNSUPPORTED = itb.BAD_ARG, itb.UNSUPPORTED
MAX_CONTIGS = 1 << 20
BASES = frozenset(b"ACGT")


def layout(contigs, gap=1, fill=b"N"):
    """[bytes] -> (the buffer, start [C], len [C]): the contigs with ``gap`` bytes of ``fill`` between two of them"""
    assert gap >= 1 and len(fill) == 1 and fill[0] not in BASES and contigs
    start, at = [], 0
    for s in contigs:
        start.append(at)
        at += len(s) + gap
    return (fill * gap).join(bytes(s) for s in contigs), start, [len(s) for s in contigs]


def table_ok(ref_len, start, length):
    """the rules the build checks on the host"""
    C = len(start)
    if len(length) != C or not 1 <= C <= MAX_CONTIGS or start[0] != 0:
        return False
    if any(l < 1 for l in length) or any(start[c] + length[c] >= start[c + 1] for c in range(C - 1)):
        return False
    return start[-1] + length[-1] == ref_len


def gaps_ok(buffer, start, length):
    """the rule the build checks on the device: no base in a gap"""
    return all(b not in BASES for c in range(len(start) - 1) for b in buffer[start[c] + length[c]:start[c + 1]])


def contig_of(start, length, t, l):
    if t < 0 or l < 1:
        return -1
    c = bisect.bisect_right(start, t) - 1  # the last contig that starts at or before t: the starts ascend
    return c if c >= 0 and t + l <= start[c] + length[c] else -1


def chain_dp_grouped(tl, ql, cands, groups, max_pred, max_dist_t, max_dist_q, bw, pen_gap, pen_skip, max_cand=None):
    """one read -> chain_dp_textbook.Chained"""
    assert 1 <= max_pred <= 64 and min(max_dist_t, max_dist_q, bw, pen_gap, pen_skip) >= 0
    assert ctb.guard_ok(max_dist_t, max_dist_q, bw, pen_gap, pen_skip) and len(groups) == len(cands)
    cands = [tuple(int(x) for x in c) for c in cands]
    groups = [int(g) for g in groups]
    n = len(cands)
    if tl < 1 or ql < 1 or any(l < 1 or t < 0 or q < 0 or t + l > tl or q + l > ql for t, q, l in cands):
        return ctb.Chained(BAD_ARG, [], 0, [], [])
    if max_cand is not None and n > max_cand:
        return ctb.Chained(UNSUPPORTED, [], 0, [], [])
    f, pred = [0] * n, [-1] * n
    for i, (ti, qi, li) in enumerate(cands):
        best, arg = li, -1
        for j in range(max(0, i - max_pred), i):
            if groups[j] != groups[i] or groups[i] < 0:
                continue
            tj, qj, lj = cands[j]
            dt, dq = ti - (tj + lj), qi - (qj + lj)
            if dt < 0 or dq < 0 or dt > max_dist_t or dq > max_dist_q or abs(dt - dq) > bw:
                continue
            s = f[j] + li - ctb.pen(dt, dq, pen_gap, pen_skip)
            if s >= best:
                best, arg = s, j
        f[i], pred[i] = best, arg
    if n == 0:
        return ctb.Chained(0, [], 0, [], [])
    end = max(range(n), key=lambda i: (f[i], -i))
    chain, i = [], end
    while i >= 0:
        chain.append(cands[i])
        i = pred[i]
    return ctb.Chained(0, chain[::-1], f[end], f, pred)


def chain_batch_grouped(t_lens, q_lens, cand_start, cand_t, cand_q, cand_len, cand_group, max_cand, max_pred, max_dist_t, max_dist_q, bw, pen_gap, pen_skip):
    """chain_dp_textbook.chain_batch with a group per candidate: the same tuple"""
    n, total = len(t_lens), len(cand_t)
    start, ct, cq, cl, score, status = [0], [], [], [], [], []
    f, pred = [None] * total, [None] * total
    for p in range(n):
        a, b = int(cand_start[p]), int(cand_start[p + 1])
        if a < 0 or b < a or b > total:
            r = ctb.Chained(BAD_ARG, [], 0, [], [])
        else:
            r = chain_dp_grouped(int(t_lens[p]), int(q_lens[p]), list(zip(cand_t[a:b], cand_q[a:b], cand_len[a:b])), cand_group[a:b], max_pred, max_dist_t,
                                 max_dist_q, bw, pen_gap, pen_skip, max_cand)
        if r.f:
            f[a:b], pred[a:b] = r.f, r.pred
        for t, q, l in r.chain:
            ct.append(t), cq.append(q), cl.append(l)
        start.append(len(ct))
        score.append(r.score)
        status.append(r.status)
    return start, ct, cq, cl, score, f, pred, status


def locate_window_contigs(start, length, q_len, anchor_start, anchor_t, anchor_q, anchor_len, slack, max_tl, total_anchors=None):
    """-> (t_start [n], t_len [n], anchor_t_out (one per anchor, None where no pair wrote it), status [n], rid [n])"""
    assert slack >= 0 and max_tl >= 1
    total = len(anchor_t) if total_anchors is None else total_anchors
    t_start, t_len, status, rid, out = [], [], [], [], [None] * len(anchor_t)
    for p, ql in enumerate(q_len):
        ql, a, b = int(ql), int(anchor_start[p]), int(anchor_start[p + 1])
        ranged = not (a < 0 or b < a or b > total)
        anchors = [(int(anchor_t[i]), int(anchor_q[i]), int(anchor_len[i])) for i in range(a, b)] if ranged else []
        st, lo, hi, c = 0, 0, 0, -1
        if anchors:
            c = contig_of(start, length, anchors[0][0], anchors[0][2])
        if ql < 1 or not ranged or any(q < 0 or q + l > ql or contig_of(start, length, t, l) != c or c < 0 for t, q, l in anchors):
            st = BAD_ARG
        elif anchors:
            (t0, q0, _), (tk, qk, lk) = anchors[0], anchors[-1]
            lo = max(start[c], t0 - q0 - slack)
            hi = min(start[c] + length[c], tk + lk + (ql - qk - lk) + slack)
            if hi - lo > max_tl:
                st = UNSUPPORTED
        if st or not anchors:
            lo = hi = 0
            c = -1
        else:
            for i in range(a, b):
                out[i] = int(anchor_t[i]) - lo
        t_start.append(lo), t_len.append(hi - lo), status.append(st), rid.append(c)
    return t_start, t_len, out, status, rid


def map_reads_contigs(index, buffer_len, start, length, Qs, k, w, strands, max_occ, max_occ_ref, merge, max_cand, cand_capacity, max_pred, max_dist_t,
                      max_dist_q, bw, pen_gap, pen_skip, slack, max_tl, ranking=None):
    """index_textbook.map_reads through the contig stages: rows -> the candidates' contigs -> grouped chains -> (strands = 2) the strand
    -> the window inside the contig.  -> (seeded, groups, chained, chosen or None, located (with rid), fed, ranked or None): ``fed`` as
    index_textbook.map_reads has it (t_start in the buffer's coordinates); ``ranked``: rank_textbook.rank_batch's tuple over the grouped
    chains' f and pred, with ``ranking`` = (max_chains, min_score, min_cnt, mask_level)."""
    seeded = itb.seed_index_batch(index, buffer_len, Qs, k, w, strands, max_occ, max_occ_ref, merge, max_cand, cand_capacity)
    cs, ct, cq, cl, row_status, row_t_len, row_q_len = seeded
    groups = [contig_of(start, length, t, l) for t, l in zip(ct, cl)]
    chained = chain_batch_grouped(row_t_len, row_q_len, cs, ct, cq, cl, groups, max_cand, max_pred, max_dist_t, max_dist_q, bw, pen_gap, pen_skip)
    queries, q_start, q_len = itb.concat(Qs)
    if strands == 2:
        chosen = rtb.select_strand(queries, q_start, q_len, *chained[:5])
        reads, (a_start, at, aq, al) = chosen[1], chosen[2:6]
    else:
        chosen, reads, (a_start, at, aq, al) = None, queries, chained[:4]
    located = locate_window_contigs(start, length, q_len, a_start, at, aq, al, slack, max_tl)
    fed = [(reads[s:s + n], located[0][p], located[1][p], [(located[2][i], aq[i], al[i]) for i in range(a_start[p], a_start[p + 1])])
           for p, (s, n) in enumerate(zip(q_start, q_len))]
    ranked = None
    if ranking is not None:
        ranked = ktb.rank_batch(strands, row_q_len, cs, ct, cq, cl, chained[5], chained[6], chained[7], max_cand, *ranking)
    return seeded, groups, chained, chosen, located, fed, ranked


def describe_mapped(buffer, start, names, fed, chosen, located, ranked, parameters, band, zdrop, to_query_end):
    """What the list form of the described mapper reports for ``map_reads_contigs``' tuples: a dict of DescribedMapResult's fields and
    rid / rname, ref_beg and ref_end from the start of the read's contig, a secondary chain as (ref_beg, ref_end, strand, score,
    parent, rid) with its contig found from its t_beg."""
    import chain_textbook as atb
    import describe_textbook as dtb
    from mgl_amd import formats

    cols = {f: [] for f in ("ref_beg", "ref_end", "strand", "score", "cigars", "status", "mapq", "n_chains", "secondary", "q_beg", "q_end", "nm", "n_match",
                            "block_len", "md", "xcigars", "rid", "rname")}
    length = [10 ** 12] * len(start)  # (a ranked chain lies inside a contig: its start alone finds it)
    for p, (oriented, t_start, t_len, anchors) in enumerate(fed):
        if not anchors:
            for f in ("ref_beg", "ref_end", "strand", "score", "q_beg", "q_end", "nm", "n_match", "block_len"):
                cols[f].append(0)
            cols["cigars"].append(""), cols["xcigars"].append(""), cols["md"].append(b""), cols["rid"].append(-1), cols["rname"].append(None)
            cols["status"].append(located[3][p] or BAD_ARG)
        else:
            T = buffer[t_start:t_start + t_len]
            aln, cigar, *_ = atb.chain_align(T, oriented, anchors, *parameters, band, zdrop, to_query_end)
            d = dtb.describe(T[aln.t_beg:aln.t_end], oriented[aln.q_beg:aln.q_end], formats.cigar_text_to_elements(cigar))
            c = located[4][p]
            for f, v in (("ref_beg", t_start + aln.t_beg - start[c]), ("ref_end", t_start + aln.t_end - start[c]), ("strand", chosen[0][p] if chosen else 0),
                         ("score", aln.score), ("q_beg", aln.q_beg), ("q_end", aln.q_end), ("nm", dtb.nm(d)), ("n_match", d.n_match),
                         ("block_len", dtb.block_len(d)), ("cigars", cigar), ("xcigars", dtb.xcigar_text(d.xcigar)), ("md", d.md), ("status", 0), ("rid", c),
                         ("rname", names[c])):
                cols[f].append(v)
        recs = ranked[1][p]
        cols["mapq"].append(recs[0].mapq if recs else 0)
        cols["n_chains"].append(ranked[0][p])
        sec = []
        for r in recs[1:]:
            c = max(x for x in range(len(start)) if start[x] <= r.t_beg)
            assert contig_of(start, length, r.t_beg, 1) >= c
            sec.append((r.t_beg - start[c], r.t_end - start[c], r.strand, r.score, r.parent, c))
        cols["secondary"].append(sec)
    return cols
