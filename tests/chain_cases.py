"""Constructed inputs that tests/test_chain_textbook.py (CPU), tests/test_gpu_chain.py (GPU) and scripts/chain_align_fuzz.py share: a
window, a query and a chain of anchors with flanks and gaps of given lengths.  Seeded by the caller: all see the same bytes."""
import extend_adaptive_cases as cases


def chain_pair(rng, flanks, gaps, lens, alphabet=b"ACGT", exact=True):
    """a window, a query and a chain: flanks = (lt, lq, rt, rq), gaps = [(gt, gq)] between the anchors of lens bases; every gap's and
    flank's query part is a noisy copy of its target part"""
    def part(a, b, rev=False):
        t, q = cases.noisy_pair(rng, a, b, alphabet) if a and b else (cases.seq(rng, a), cases.seq(rng, b))
        return (t[::-1], q[::-1]) if rev else (t, q)

    lt, lq, rt, rq = flanks
    T, Q = part(lt, lq, True)
    anchors = []
    for k, sl in enumerate(lens):
        a = cases.seq(rng, sl)
        b = bytearray(a)
        if not exact and sl > 2:
            b[sl // 2] = ord("N")
        anchors.append((len(T), len(Q), sl))
        T, Q = T + a, Q + bytes(b)
        if k < len(gaps):
            gt, gq = part(*gaps[k])
            T, Q = T + gt, Q + gq
    t, q = part(rt, rq)
    return T + t, Q + q, anchors
