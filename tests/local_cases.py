"""Adversarial inputs for the local Smith-Waterman kernels (tests/test_gpu_local_edges.py) and, from the textbook alone
(tests/local_textbook.py), the measures that say whether an input is adversarial ENOUGH: tests/test_local_cases.py asserts them on any
machine, so a generator that stops producing ties or seam-crossing gaps fails there instead of making a GPU test vacuous.

Every generator is seeded and takes nothing a test varies at random.  A pair is (t, q, key, o, e): target and query as bytes, the name
of its scoring (scoring()) and the gap penalties."""
import re

import numpy as np

import local_textbook as lt

PROT = np.frombuffer(b"ARNDCQEGHILKMFPSTWYV", np.uint8)


def scoring(key):
    """(code, matrix) of a pair's scoring: 'dna1' = +1 / -1, 'dna23' = +2 / -3 over ACGTN, 'blosum' = BLOSUM62."""
    if key == "dna1":
        return lt.dna_matrix(1, -1)
    if key == "dna23":
        return lt.dna_matrix(2, -3)
    from mgl_amd import protein

    return protein.blosum62()


# ---- ties in the end cell ------------------------------------------------------------------------------------------------------------
def tied_pairs():
    """DNA repeats and homopolymers whose maximum is held by many cells: a short repeat query against a long repeat target (one column,
    many rows, several 64-row strips), a long repeat query against a short target (one row, many columns), a query holding the same
    repeat twice with a stretch of N between (two columns: the copy at the LARGER column ends in a SMALLER row than later ends of the
    first copy), and the homopolymer forms of the first two.  Target lengths on both sides of 64 and 128."""
    rng = np.random.default_rng(101)
    out = []
    for key in ("dna1", "dna23"):
        for n, tl in enumerate((60, 63, 64, 65, 70, 100, 127, 128, 129, 140, 200)):
            unit = [b"ACGT", b"GTACC", b"TGCA", b"CA"][n % 4]
            junk = b"N" * int(rng.integers(0, 4))  # the repeat's phase moves
            t = (junk + unit * (tl // len(unit) + 1))[:tl]
            copy = unit * (12 // len(unit))
            out.append((t, copy, key, 5, 1))                                  # one column, every period's row
            out.append((t[:40], unit * 40, key, 5, 1))                        # one row, many columns
            out.append((t, copy + b"N" * 15 + copy, key, 5, 1))               # two columns x many rows
            out.append((t, copy + b"N" * 15 + copy + b"N" * 15 + copy, key, 7, 2))
            out.append((b"A" * tl, b"A" * 20, key, 5, 1))                     # rows 20 .. tl of column 20
            out.append((b"A" * 30, b"A" * (tl // 2 + 10), key, 5, 1))         # row 30, columns 30 ..
    return out


def end_ties(t, q, code, mat, o, e, rows=64):
    """From the textbook's H: (cells holding the maximum, in two strips of `rows` rows?, in one row at two columns?, in two rows of one
    strip with the smaller row at the larger column?)."""
    H = lt.local_matrices_np(t, q, code, mat, o, e)[0]
    ii, jj = np.nonzero(H[1:, 1:] == H[1:, 1:].max())
    ii, jj = ii + 1, jj + 1
    strip = (ii - 1) // rows
    two_strips = len(set(strip.tolist())) > 1
    one_row = any((ii == r).sum() > 1 for r in set(ii.tolist()))
    crossed = False
    for s in set(strip.tolist()):
        a, b = ii[strip == s], jj[strip == s]
        # cells come in row-major order: a later cell of a larger row at a smaller column than some earlier one
        best = -1
        for r in sorted(set(a.tolist())):
            if best > b[a == r].min():
                crossed = True
            best = max(best, int(b[a == r].max()))
    return len(ii), two_strips, one_row, crossed


# ---- ties in the walk ----------------------------------------------------------------------------------------------------------------
def walk_tie_pairs():
    """Pairs over two- and three-letter alphabets under +1 / -1 and +2 / -3 with o == e and o == 0: gaps cost what mismatches cost, so a
    walk meets cells that the diagonal, F and E reach with one value, and gaps that opening and extending reach with one value."""
    rng = np.random.default_rng(102)
    out = []
    for n in range(160):
        key = ("dna1", "dna23")[n % 2]
        o, e = [(1, 1), (0, 0), (2, 2), (0, 1), (3, 3), (0, 2)][n % 6]
        alpha = np.frombuffer((b"AC", b"ACG", b"AT")[n % 3], np.uint8)
        t = bytearray(alpha[rng.integers(0, len(alpha), int(rng.integers(30, 150)))].tobytes())
        q = bytearray(t[int(rng.integers(0, 10)):])
        for _ in range(int(rng.integers(2, 9))):
            k = int(rng.integers(0, len(q)))
            if rng.random() < 0.5:
                del q[k:k + int(rng.integers(1, 5))]
            else:
                q[k:k] = alpha[rng.integers(0, len(alpha), int(rng.integers(1, 5)))].tobytes()
        out.append((bytes(t), bytes(q or b"A"), key, o, e))
    return out


def walk_ties(t, q, code, mat, o, e):
    """The textbook's walk over the textbook's matrices, counting the cells where its order of preference decides: (H == diagonal == F,
    H == F == E without the diagonal, open == extend in a gap).  Its CIGAR is checked against local_align_np's."""
    o, e = abs(int(o)), abs(int(e))
    H, E, F = lt.local_matrices_np(t, q, code, mat, o, e)
    want = lt.local_align_np(t, q, code, mat, o, e)
    if want[0] == 0:
        return 0, 0, 0
    i, j, state, ops = want[2], want[4], "H", []
    n_df = n_fe = n_oe = 0
    while True:
        if state == "H":
            if i == 0 or j == 0 or H[i, j] == 0:
                break
            diag = H[i - 1, j - 1] + int(mat[code[t[i - 1]]][code[q[j - 1]]])
            if H[i, j] == diag:
                n_df += int(H[i, j] == F[i, j])
                ops.append("M")
                i, j = i - 1, j - 1
            elif H[i, j] == F[i, j]:
                n_fe += int(H[i, j] == E[i, j])
                state = "F"
            else:
                state = "E"
        elif state == "F":
            ops.append("I")
            n_oe += int(F[i, j - 1] - e == H[i, j - 1] - o)
            state = "F" if F[i, j - 1] - e >= H[i, j - 1] - o else "H"
            j -= 1
        else:
            ops.append("D")
            n_oe += int(E[i - 1, j] - e == H[i - 1, j] - o)
            state = "E" if E[i - 1, j] - e >= H[i - 1, j] - o else "H"
            i -= 1
    assert lt.cigar_text("".join(reversed(ops))) == want[5] and (i, j) == (want[1], want[3])
    return n_df, n_fe, n_oe


# ---- long gaps across strip seams ------------------------------------------------------------------------------------------------------
SEAM_GAPS = (20, 33, 63, 64, 65, 70, 100, 130, 160, 200)


def seam_gap_pairs(rows_per_strip):
    """Protein under BLOSUM62, one target of 560 residues per gap model (o in {2, 11} x e in {0, 1}), so that the pairs of a gap model
    also form a shared-target tile.  Deletions: the query is two pieces of the target with g = 20 .. 200 residues cut out between them,
    the cut placed so that rows M and M + 1 (M a multiple of `rows_per_strip`) both lie inside it.  Insertions: the query is the target's
    piece with g random residues put in after row M - 1, M or M + 1 (a run of g columns in the last or first row of a strip; g > 64
    crosses more anti-diagonal steps than a strip of kernel B has lanes).  The flanks are 90 residues or more (an identical flank scores
    about 5 a residue; the dearest gap costs 11 + 199).  Returns (t, q, 'blosum', o, e, kind) with kind 'D' or 'I'."""
    R = rows_per_strip
    rng = np.random.default_rng(103 + R)
    out = []
    for o in (2, 11):
        for e in (0, 1):
            t = PROT[rng.integers(0, 20, 560)].tobytes()
            for n, g in enumerate(SEAM_GAPS + SEAM_GAPS[2:]):
                d = int(rng.integers(1, g))                       # rows of the cut above the seam
                m = -(-(95 + d) // R)                             # the first seam with 95 residues or more above the cut
                la = m * R - d                                    # rows la + 1 .. la + g are cut: M = m R and M + 1 among them
                s0 = la - 95 + n % 5
                out.append((t, t[s0:la] + t[la + g:la + g + 90 + n % 7], "blosum", o, e, "D"))
            for n, g in enumerate(SEAM_GAPS):
                row = (2 + n % 3) * 64 + (-1, 0, 1)[n % 3]  # (a multiple of 64 is one of 32 too)
                s0 = row - 92 - n
                x = PROT[rng.integers(0, 20, g)].tobytes()
                out.append((t, t[s0:row] + x + t[row:row + 95], "blosum", o, e, "I"))
    return out


def cigar_runs(cigar, t_begin):
    """[(op, length, first target row, last target row)] of a text CIGAR that begins at target offset t_begin (rows count from 1; an
    insertion lies in the row before it)."""
    runs, i = [], t_begin
    for n, op in re.findall(r"(\d+)([MID])", cigar):
        n = int(n)
        if op == "I":
            runs.append((op, n, i, i))
        else:
            runs.append((op, n, i + 1, i + n))
            i += n
    return runs


def d_run_straddles(cigar, t_begin, rows_per_strip):
    """A 'D' run holds rows M and M + 1 for a multiple M of rows_per_strip: it begins above a strip seam and ends below it."""
    for op, n, a, b in cigar_runs(cigar, t_begin):
        seam = (b - 1) // rows_per_strip * rows_per_strip  # the largest multiple below the run's last row
        if op == "D" and seam >= a:
            return True
    return False


def longest_i_run(cigar):
    return max([int(n) for n, op in re.findall(r"(\d+)([MID])", cigar) if op == "I"], default=0)


# ---- kernel A's 16-bit guard, at its last length -----------------------------------------------------------------------------------------
GUARD_EDGES = ((-128, 127, 514), (-8, 120, 544))  # smax L + 255 = 65 533 and 65 535: L is the last length local_lane_ok admits
SLOT_LOW, SLOT_HIGH, SLOT_BOTH = 10, 21, 40       # the identical query in a lane's low half, high half, both halves (40, 41)


def guard_edge_tiles():
    """For each (smin, smax, L) of GUARD_EDGES and each length in (L, L + 1, L + 3): (smin, smax, L, length, code, matrix, target,
    queries).  The matrix scores smax on the diagonal and holds smin; the target is `length` residues of codes 0 .. 30, so the identical
    query scores smax * length.  The tile's 128 queries: the identical one in slot 10 with a query of code 31 alone in slot 11 (no
    positive score against the target: exactly 0), the other way round in slots 20 / 21, the identical one in both 40 and 41; the
    others prefixes, suffixes and random residues of mixed lengths, with two holes."""
    out = []
    for n, (smin, smax, L) in enumerate(GUARD_EDGES):
        rng = np.random.default_rng(104 + n)
        mat = rng.integers(-8, 9, size=(32, 32)).astype(np.int8)
        mat[np.arange(32), np.arange(32)] = smax
        mat[31, :31] = mat[:31, 31] = -5      # code 31: the cold query's, absent from the target
        mat[3, 17] = smin
        code = (np.arange(256) % 32).astype(np.uint8)
        for length in (L, L + 1, L + 3):
            t = rng.integers(0, 31, length).astype(np.uint8).tobytes()
            qs = []
            for k in range(128):
                r = k % 4
                if r == 0:
                    q = t[: length - 3 * k]
                elif r == 1:
                    q = t[k:]
                elif r == 2:
                    q = rng.integers(0, 32, int(rng.integers(1, length + 1))).astype(np.uint8).tobytes()
                else:
                    q = t[: length // 2] + rng.integers(0, 32, int(rng.integers(1, length // 2))).astype(np.uint8).tobytes()
                qs.append(q)
            cold = bytes([31]) * length
            qs[SLOT_LOW], qs[SLOT_LOW + 1] = t, cold
            qs[SLOT_HIGH - 1], qs[SLOT_HIGH] = cold, t
            qs[SLOT_BOTH], qs[SLOT_BOTH + 1] = t, t
            qs[60] = qs[99] = b""
            out.append((smin, smax, L, length, code, mat, t, qs))
    return out
