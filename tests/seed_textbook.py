"""The function of mgl_sw_seed_batch_device (include/mgl_sw.h), stated once in plain Python: the minimizer seeds of
a read against its own window, as candidate anchors (t, q, l) -- T[t .. t + l) equals Q[q .. q + l) -- in the CSR layout and the order
mgl_sw_chain_anchors_batch_device reads.  Integers only.

k-mers.  Codes are A = 0, C = 1, G = 2, T = 3, upper case only.  The k-mer at position i is valid iff all of its k bytes are one of these
four; its key is the 2k-bit number with the first base in the top bits (all 32 bits at k = 16); h = fmix32(key ^ 0x9E3779B9), fmix32
being murmur3's 32-bit finaliser.

The sketch of a sequence of L bytes, nk = L - k + 1 k-mer positions: empty for nk < 1; the windows are [a, a + w) for a = 0 .. nk - w,
and the one window [0, nk) if nk < w; a window selects its valid position with the smallest h, ties to the smallest position, and
nothing if it has no valid position; the sketch is the set of selected positions with their keys, ascending.

Hits.  occ(x) is the number of positions of the query's sketch with key x.  Every position t of the window's sketch with key x and
1 <= occ(x) <= max_occ gives one raw hit (t, q, k) per position q of the query's sketch with key x.  R is their number.

Merge (merge = 1).  Raw hits on one diagonal t - q, ascending in t, are joined while the next starts at or before the end of the run so
far (t <= t0 + l0: overlapping or touching); a run becomes the candidate (t0, q0, t_last + k - t0): the maximal diagonal runs of the
cells the raw hits cover.  With merge = 0 the candidates are the raw hits.  A pair's candidates are sorted ascending by (t, q).

Statuses (mgl_sw_status) per pair, the first that applies: 1 (BAD_ARG) for tl < 1 or ql < 1; 5 (UNSUPPORTED) for a query sketch of more
than MAX_QUERY_SEEDS positions or R > max_cand; 3 (NOMEM) by the capacity rule: with N_p the candidates of pair p (0 for a refused one)
and S_p the sum of N_j over j < p, pairs are kept in index order while S_p + N_p <= cand_capacity, and from the first pair P* that does
not fit on EVERY pair -- empty ones included, all but those refused above, which keep their status -- is 3.  A pair with a non-zero
status has no candidates.  cand_start[p] = S_p for p <= P* and S_(P*) beyond it.
"""
from collections import namedtuple

BAD_ARG, NOMEM, UNSUPPORTED = 1, 3, 5
MAX_QUERY_SEEDS = 8192
CODE = {65: 0, 67: 1, 71: 2, 84: 3}  # A C G T

Seeded = namedtuple("Seeded", "status cands raw query_seeds")  # cands, raw: [(t, q, l)]; raw: the hits before the merge


def fmix32(h):
    h &= 0xFFFFFFFF
    h ^= h >> 16
    h = h * 0x85EBCA6B & 0xFFFFFFFF
    h ^= h >> 13
    h = h * 0xC2B2AE35 & 0xFFFFFFFF
    return h ^ h >> 16


def kmer_hash(key):
    return fmix32(key ^ 0x9E3779B9)


def kmers(seq, k):
    """-> per k-mer position the key, or None where the k-mer is not valid"""
    out = []
    for i in range(len(seq) - k + 1):
        key = 0
        for b in seq[i:i + k]:
            c = CODE.get(b)
            if c is None:
                key = None
                break
            key = key << 2 | c
        out.append(key)
    return out


def sketch(seq, k, w):
    """-> [(position, key)] ascending by position"""
    keys = kmers(bytes(seq), k)
    nk = len(keys)
    if nk < 1:
        return []
    hs = [None if key is None else kmer_hash(key) for key in keys]
    picked = set()
    for a in range(max(nk - w, 0) + 1):
        best = None
        for i in range(a, min(a + w, nk)):
            if hs[i] is not None and (best is None or hs[i] < hs[best]):
                best = i
        if best is not None:
            picked.add(best)
    return [(i, keys[i]) for i in sorted(picked)]


def raw_hits(ts, qs, k, max_occ):
    """the sketches of the window and of the query -> [(t, q, k)] ascending by (t, q)"""
    where = {}
    for q, key in qs:
        where.setdefault(key, []).append(q)
    return [(t, q, k) for t, key in ts if len(where.get(key, ())) <= max_occ for q in where.get(key, ())]


def merge_hits(hits, k):
    """raw hits -> the maximal runs per diagonal, ascending by (t, q)"""
    out = []
    run = None  # [t0, q0, l0]
    for d, t in sorted((t - q, t) for t, q, _ in hits):
        if run is not None and d == run[0] - run[1] and t <= run[0] + run[2]:
            run[2] = t + k - run[0]
        else:
            if run is not None:
                out.append(tuple(run))
            run = [t, t - d, k]
    if run is not None:
        out.append(tuple(run))
    return sorted(out)


def seed_pair(T, Q, k, w, max_occ, merge, max_cand):
    """one pair -> Seeded (the capacity rule is the batch's)"""
    assert 4 <= k <= 16 and 1 <= w <= 32 and 1 <= max_occ <= 64 and merge in (0, 1, False, True) and 1 <= max_cand <= 8192
    if len(T) < 1 or len(Q) < 1:
        return Seeded(BAD_ARG, [], [], 0)
    qs = sketch(Q, k, w)
    if len(qs) > MAX_QUERY_SEEDS:
        return Seeded(UNSUPPORTED, [], [], len(qs))
    raw = raw_hits(sketch(T, k, w), qs, k, max_occ)
    if len(raw) > max_cand:
        return Seeded(UNSUPPORTED, [], raw, len(qs))
    return Seeded(0, merge_hits(raw, k) if merge else raw, raw, len(qs))


def seed_batch(Ts, Qs, k, w, max_occ, merge, max_cand, cand_capacity):
    """The batch as the entry sees it -> (cand_start [n + 1], cand_t, cand_q, cand_len (each cand_start[n] long), status [n])."""
    assert 0 <= cand_capacity <= 1 << 30
    start, ct, cq, cl, status = [0], [], [], [], []
    cut = False
    for T, Q in zip(Ts, Qs):
        r = seed_pair(T, Q, k, w, max_occ, merge, max_cand)
        cut = cut or len(ct) + len(r.cands) > cand_capacity
        if cut or r.status:
            status.append(r.status or NOMEM)
        else:
            status.append(0)
            for t, q, l in r.cands:
                ct.append(t), cq.append(q), cl.append(l)
        start.append(len(ct))
    return start, ct, cq, cl, status
