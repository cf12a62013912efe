"""The functions of mgl_sw_index_build_device, mgl_sw_seed_index_batch_device and mgl_sw_locate_window_batch_device (include/mgl_sw.h,
DESIGN.md section 9j), stated once in plain Python on top of seed_textbook.py (what a sketch, a hit and the merge are),
strand_textbook.py (the reverse complement, the choice of a strand) and chain_dp_textbook.py (chaining).  Integers only.

The index of a reference R is R's sketch as M entries (key, position), ascending.  A key is the whole k-mer, so an entry with a read's
key IS an exact match of k bases.

A row is one oriented read Q against the whole reference.  occ_Q(x): the positions of Q's sketch with key x; occ_I(x): the index's
entries with key x.  Every position q of Q's sketch with key x, 1 <= occ_Q(x) <= max_occ and 1 <= occ_I(x) <= max_occ_ref gives one raw
hit (t, q, k) per entry t with key x; R_p is their number; they ascend by (t, q).  Merge, statuses and the capacity rule are
seed_textbook's, per row in row order.  strands = 1: row p is Q_p; strands = 2: row 2p is Q_p, row 2p + 1 is rc(Q_p).

The window of a chain with K >= 1 anchors, first (t0, q0, l0), last (tK, qK, lK): lo = max(0, t0 - q0 - slack),
hi = min(ref_len, tK + lK + (ql - qK - lK) + slack); t_start = lo, t_len = hi - lo, every anchor's t becomes t - lo.  K = 0: an
unmapped read, t_start = t_len = 0, status 0.  Status 1 (BAD_ARG) for ql < 1, a range of anchor_start that descends or leaves
[0, total_anchors], or an anchor with l < 1, t < 0, q < 0, t + l > ref_len or q + l > ql; 5 (UNSUPPORTED) for hi - lo > max_tl.  A
refused pair has t_start = t_len = 0 and no anchor written.
"""
import chain_dp_textbook as ctb
import seed_textbook as stb
import strand_textbook as rtb

BAD_ARG, NOMEM, UNSUPPORTED = stb.BAD_ARG, stb.NOMEM, stb.UNSUPPORTED
MAX_OCC_REF = 8192


def build_index(R, k, w):
    """-> [(key, position)] ascending"""
    assert 4 <= k <= 16 and 1 <= w <= 32 and 1 <= len(R) < 1 << 31
    return sorted((key, pos) for pos, key in stb.sketch(R, k, w))


def by_key(index):
    """the index as {key: [positions ascending]}: what seed_index_row looks up in (an index may be handed to it in either form)"""
    table = {}
    for key, pos in index:
        table.setdefault(key, []).append(pos)
    return table


def seed_index_row(index, ref_len, Q, k, w, max_occ, max_occ_ref, merge, max_cand):
    """one row -> seed_textbook.Seeded (the capacity rule is the batch's)"""
    assert 1 <= max_occ <= 64 and 1 <= max_occ_ref <= MAX_OCC_REF and merge in (0, 1, False, True) and 1 <= max_cand <= 8192 and ref_len >= 1
    table = index if isinstance(index, dict) else by_key(index)
    if len(Q) < 1:
        return stb.Seeded(BAD_ARG, [], [], 0)
    qs = stb.sketch(Q, k, w)
    if len(qs) > stb.MAX_QUERY_SEEDS:
        return stb.Seeded(UNSUPPORTED, [], [], len(qs))
    occ_q = {}
    for _, key in qs:
        occ_q[key] = occ_q.get(key, 0) + 1
    raw = sorted((t, q, k) for q, key in qs if occ_q[key] <= max_occ and len(table.get(key, ())) <= max_occ_ref for t in table.get(key, ()))
    if len(raw) > max_cand:
        return stb.Seeded(UNSUPPORTED, [], raw, len(qs))
    return stb.Seeded(0, stb.merge_hits(raw, k) if merge else raw, raw, len(qs))


def rows(Qs, strands):
    """-> the rows' oriented reads"""
    assert strands in (1, 2)
    return [bytes(Q) for Q in Qs] if strands == 1 else rtb.rows(Qs, Qs)[1]


def seed_index_batch(index, ref_len, Qs, k, w, strands, max_occ, max_occ_ref, merge, max_cand, cand_capacity):
    """The batch as the entry sees it -> strand_textbook.seed_strands_batch's tuple over the strands * n rows: (cand_start [rows + 1],
    cand_t, cand_q, cand_len, status [rows], row_t_len, row_q_len)."""
    assert 0 <= cand_capacity <= 1 << 30
    table = index if isinstance(index, dict) else by_key(index)
    oriented = rows(Qs, strands)
    start, ct, cq, cl, status = [0], [], [], [], []
    cut = False
    for Q in oriented:
        r = seed_index_row(table, ref_len, Q, k, w, max_occ, max_occ_ref, merge, max_cand)
        cut = cut or len(ct) + len(r.cands) > cand_capacity
        if cut or r.status:
            status.append(r.status or NOMEM)
        else:
            status.append(0)
            for t, q, l in r.cands:
                ct.append(t), cq.append(q), cl.append(l)
        start.append(len(ct))
    return start, ct, cq, cl, status, [ref_len] * len(oriented), [len(Q) for Q in oriented]


def locate_window(ref_len, q_len, anchor_start, anchor_t, anchor_q, anchor_len, slack, max_tl, total_anchors=None):
    """-> (t_start [n], t_len [n], anchor_t_out (one per anchor, None where no pair wrote it), status [n])"""
    assert slack >= 0 and max_tl >= 1 and 1 <= ref_len < 1 << 31
    total = len(anchor_t) if total_anchors is None else total_anchors
    t_start, t_len, status, out = [], [], [], [None] * len(anchor_t)
    for p, ql in enumerate(q_len):
        ql, a, b = int(ql), int(anchor_start[p]), int(anchor_start[p + 1])
        anchors = [] if a < 0 or b < a or b > total else [(int(anchor_t[i]), int(anchor_q[i]), int(anchor_len[i])) for i in range(a, b)]
        st, lo, hi = 0, 0, 0
        if ql < 1 or a < 0 or b < a or b > total or any(l < 1 or t < 0 or q < 0 or t + l > ref_len or q + l > ql for t, q, l in anchors):
            st = BAD_ARG
        elif anchors:
            (t0, q0, _), (tk, qk, lk) = anchors[0], anchors[-1]
            lo = max(0, t0 - q0 - slack)
            hi = min(ref_len, tk + lk + (ql - qk - lk) + slack)
            if hi - lo > max_tl:
                st = UNSUPPORTED
        if st or not anchors:
            lo = hi = 0
        else:
            for i in range(a, b):
                out[i] = int(anchor_t[i]) - lo
        t_start.append(lo), t_len.append(hi - lo), status.append(st)
    return t_start, t_len, out, status


def concat(Qs):
    """-> (one buffer, q_start, q_len)"""
    start, at = [], 0
    for Q in Qs:
        start.append(at)
        at += len(Q)
    return b"".join(bytes(Q) for Q in Qs), start, [len(Q) for Q in Qs]


def map_reads(index, ref_len, Qs, k, w, strands, max_occ, max_occ_ref, merge, max_cand, cand_capacity, max_pred, max_dist_t, max_dist_q, bw, pen_gap,
              pen_skip, slack, max_tl):
    """rows -> chains -> (strands = 2) the strand -> the window.  -> (seeded, chained, chosen or None, located, oriented): the tuples of
    seed_index_batch, chain_dp_textbook.chain_batch, strand_textbook.select_strand and locate_window, and what the alignment is then
    fed: per read (the oriented read, t_start, t_len, its anchors [(t - t_start, q, l)])."""
    seeded = seed_index_batch(index, ref_len, Qs, k, w, strands, max_occ, max_occ_ref, merge, max_cand, cand_capacity)
    chained = rtb.chain_rows(seeded, max_cand, max_pred, max_dist_t, max_dist_q, bw, pen_gap, pen_skip)
    queries, q_start, q_len = concat(Qs)
    if strands == 2:
        chosen = rtb.select_strand(queries, q_start, q_len, *chained[:5])
        reads, (start, at, aq, al) = chosen[1], chosen[2:6]
    else:
        chosen, reads, (start, at, aq, al) = None, queries, chained[:4]
    located = locate_window(ref_len, q_len, start, at, aq, al, slack, max_tl)
    fed = [(reads[s:s + n], located[0][p], located[1][p], [(located[2][i], aq[i], al[i]) for i in range(start[p], start[p + 1])])
           for p, (s, n) in enumerate(zip(q_start, q_len))]
    return seeded, chained, chosen, located, fed
