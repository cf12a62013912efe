"""The functions of mgl_sw_seed_strands_batch_device and mgl_sw_select_strand_batch_device (include/mgl_sw.h), stated
once in plain Python on top of seed_textbook.py and chain_dp_textbook.py, which say what seeding and chaining are.

The reverse complement.  rc(Q)[i] = comp(Q[ql - 1 - i]); comp swaps upper-case A <-> T and C <-> G and maps every other byte (N, lower
case, anything) to itself, so a k-mer that is not valid stays so at its mirrored place.

Rows.  A batch of n pairs is a batch of 2n rows, row r = 2p + s: row 2p is (T_p, Q_p), row 2p + 1 is (T_p, rc(Q_p)).  Seeding both
strands is seed_textbook.seed_batch on the rows: statuses, the max_cand and sketch bounds and the capacity rule per row and in row order;
a candidate's q is a coordinate of that row's oriented read.

The choice.  Row r has K_r chained anchors and the chain score c_r, 0 for a row with no chain (K_r = 0: nothing to chain, or refused).
strand_p = 1 iff c_(2p+1) > c_(2p): ties and two zeros give strand 0.  Pair p gets the K_p anchors of row 2p + strand_p and the oriented
read.  Status 1 (BAD_ARG) for ql < 1, a read that leaves [0, query_bytes) or a row's range of chain_start that descends or leaves
[0, total_chain]: strand 0, K_p = 0, score 0, nothing written.
"""
import chain_dp_textbook as ctb
import seed_textbook as stb

BAD_ARG = 1
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(Q):
    return bytes(Q).translate(COMP)[::-1]


def rows(Ts, Qs):
    """-> the 2n rows' (targets, oriented reads)"""
    return [T for T in Ts for _ in (0, 1)], [R for Q in Qs for R in (bytes(Q), revcomp(Q))]


def seed_strands_batch(Ts, Qs, k, w, max_occ, merge, max_cand, cand_capacity):
    """-> seed_batch's tuple over the 2n rows, and the rows' (t_len, q_len)"""
    rT, rQ = rows(Ts, Qs)
    return stb.seed_batch(rT, rQ, k, w, max_occ, merge, max_cand, cand_capacity) + ([len(T) for T in rT], [len(Q) for Q in rQ])


def chain_rows(seeded, max_cand, max_pred, max_dist_t, max_dist_q, bw, pen_gap, pen_skip):
    """seed_strands_batch's tuple -> chain_dp_textbook.chain_batch's over the 2n rows"""
    start, ct, cq, cl, _, t_len, q_len = seeded
    return ctb.chain_batch(t_len, q_len, start, ct, cq, cl, max_cand, max_pred, max_dist_t, max_dist_q, bw, pen_gap, pen_skip)


def select_strand(queries, q_start, q_len, chain_start, chain_t, chain_q, chain_len, chain_score, total_chain=None):
    """The choice as the entry sees it: ``queries`` one buffer of bytes, the chain arrays over 2n rows ->
    (strand [n], queries_out (bytes outside a chosen read are 0), anchor_start [n + 1], anchor_t, anchor_q, anchor_len, score [n],
    status [n])."""
    n = len(q_start)
    total = len(chain_t) if total_chain is None else total_chain
    out = bytearray(len(queries))
    strand, start, at, aq, al, score, status = [], [0], [], [], [], [], []
    for p in range(n):
        ql, qs = int(q_len[p]), int(q_start[p])
        c = [int(x) for x in chain_start[2 * p:2 * p + 3]]
        if ql < 1 or qs < 0 or qs + ql > len(queries) or c[0] < 0 or c[1] < c[0] or c[2] < c[1] or c[2] > total:
            strand.append(0), score.append(0), status.append(BAD_ARG), start.append(len(at))
            continue
        sc = [int(chain_score[2 * p + s]) if c[s + 1] > c[s] else 0 for s in (0, 1)]
        s = 1 if sc[1] > sc[0] else 0
        Q = bytes(queries[qs:qs + ql])
        out[qs:qs + ql] = revcomp(Q) if s else Q
        for i in range(c[s], c[s + 1]):
            at.append(int(chain_t[i])), aq.append(int(chain_q[i])), al.append(int(chain_len[i]))
        strand.append(s), score.append(sc[s]), status.append(0), start.append(len(at))
    return strand, bytes(out), start, at, aq, al, score, status
