"""The textbook of mgl_sw_describe_alignments_batch_device: what an alignment's CIGAR says about its two
spans -- the counts, the MD text of the SAM specification and the extended (= / X) CIGAR.  Plain Python, written for clarity;
the kernel is bit for bit this function.  Bases are compared as BYTES, as every alignment kernel here scores them: no case
folding and no special N."""
from collections import namedtuple

Description = namedtuple("Description", "n_match n_mismatch n_ins n_del n_ins_runs n_del_runs md xcigar")

BAM_OP = {"M": 0, "I": 1, "D": 2, "=": 7, "X": 8}


def describe(target_span, query_span, cigar):
    """``cigar``: a list of (len, op), op in M / I / D, len >= 1, that spends exactly the two spans.  Returns Description: the six
    counts, ``md`` (bytes) and ``xcigar``, a list of (len, op) with op in = / X / I / D and adjacent equal operations merged."""
    t, q = bytes(target_span), bytes(query_span)
    n_match = n_mismatch = n_ins = n_del = n_ins_runs = n_del_runs = 0
    md, run = [], 0                   # run: the matches since the last MD token
    xc = []

    def push(n, op):                  # the extended CIGAR, merged across element borders
        if xc and xc[-1][1] == op:
            xc[-1] = (xc[-1][0] + n, op)
        else:
            xc.append((n, op))

    i = j = 0
    for n, op in cigar:
        if n < 1 or op not in ("M", "I", "D"):
            raise ValueError("not an M / I / D element of at least one base: %r" % ((n, op),))
        if op == "M":
            if i + n > len(t) or j + n > len(q):
                raise ValueError("the CIGAR spends more than the spans hold")
            for c in range(n):
                if t[i + c] == q[j + c]:
                    n_match += 1
                    run += 1
                    push(1, "=")
                else:
                    n_mismatch += 1
                    md.append(b"%d" % run + t[i + c:i + c + 1])
                    run = 0
                    push(1, "X")
            i += n
            j += n
        elif op == "I":               # nothing in MD, and a run of matches goes on across it
            if j + n > len(q):
                raise ValueError("the CIGAR spends more than the spans hold")
            n_ins += n
            n_ins_runs += 1
            push(n, "I")
            j += n
        else:
            if i + n > len(t):
                raise ValueError("the CIGAR spends more than the spans hold")
            n_del += n
            n_del_runs += 1
            md.append(b"%d" % run + b"^" + t[i:i + n])
            run = 0
            push(n, "D")
            i += n
    if i != len(t) or j != len(q):
        raise ValueError("the CIGAR spends %d target and %d query bytes of %d and %d" % (i, j, len(t), len(q)))
    md.append(b"%d" % run)
    return Description(n_match, n_mismatch, n_ins, n_del, n_ins_runs, n_del_runs, b"".join(md), xc)


def nm(d):
    return d.n_mismatch + d.n_ins + d.n_del


def block_len(d):
    return d.n_match + nm(d)


def stats(d, binary=False):
    """The eight int32 of mgl_sw_alignment_stats; xcigar_len in bytes of the text, or of the BAM words with ``binary``."""
    return [d.n_match, d.n_mismatch, d.n_ins, d.n_del, d.n_ins_runs, d.n_del_runs, len(d.md), len(xcigar_bytes(d.xcigar, binary))]


def xcigar_text(xc):
    return "".join("%d%s" % e for e in xc)


def xcigar_bytes(xc, binary=False):
    """The extended CIGAR as the entry writes it: text, or little-endian uint32 words len << 4 | op code (= is 7, X is 8)."""
    if not binary:
        return xcigar_text(xc).encode()
    return b"".join(((n << 4) | BAM_OP[op]).to_bytes(4, "little") for n, op in xc)


def cigar_bytes(cigar, binary=False):
    """An M / I / D CIGAR as the alignment entries write it."""
    return xcigar_bytes(cigar, binary)


def describe_by_columns(target_span, query_span, cigar):
    """The same function stated another way, for the tests: the alignment is expanded to columns first, then run-length encoded."""
    t, q = bytes(target_span), bytes(query_span)
    cols, i, j = [], 0, 0              # (kind, target byte or None)
    for n, op in cigar:
        for _ in range(n):
            if op == "M":
                cols.append(("=" if t[i] == q[j] else "X", t[i]))
                i, j = i + 1, j + 1
            elif op == "I":
                cols.append(("I", None))
                j += 1
            else:
                cols.append(("D", t[i]))
                i += 1
    assert i == len(t) and j == len(q)
    kinds = [k for k, _ in cols]
    xc, runs = [], {"I": 0, "D": 0}
    for k, kind in enumerate(kinds):
        if k and kinds[k - 1] == kind:
            xc[-1] = (xc[-1][0] + 1, kind)
        else:
            xc.append((1, kind))
    # runs count ELEMENTS of the CIGAR, which need not be merged
    for n, op in cigar:
        if op in runs:
            runs[op] += 1
    md, run, in_del, k = "", 0, False, 0
    elem_of = [e for e, (n, _) in enumerate(cigar) for _ in range(n)]
    for k, (kind, base) in enumerate(cols):
        if kind == "I":
            continue
        new_del = kind == "D" and not (in_del and elem_of[k] == last_del)
        if kind == "=":
            run += 1
            in_del = False
        elif kind == "X":
            md += "%d%c" % (run, base)
            run, in_del = 0, False
        elif new_del:
            md += "%d^%c" % (run, base)
            run, in_del, last_del = 0, True, elem_of[k]
        else:
            md += chr(base)
    md += "%d" % run
    return Description(kinds.count("="), kinds.count("X"), kinds.count("I"), kinds.count("D"), runs["I"], runs["D"], md.encode("latin-1"), xc)
