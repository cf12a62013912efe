"""Constructed inputs for the PairHMM kernels (mgl_amd/csrc/pairhmm_kernels.hip), shared by test_pairhmm_cases.py (CPU:
what the cases reach, according to variant()) and test_gpu_pairhmm_edges.py (GPU: the kernels against the restatement).

Everything is plain numpy in the layout of pairhmm.pack_reads / pack_haps, deterministic from SEED.  A Case is two pools
(reads, haplotypes) and a pair list over them; take() reorders or cuts the pair list and remembers where each pair stood
in the list it came from, so one oracle run of the root list serves every order of it.

Why the inputs look as they do:
  * sequences: for R <= H a "prefix" read is a copy of the haplotype's first R bases and a "suffix" read a copy of its
    last R bases (2 % flips); for R > H the haplotype is a copy of the read's first ("prefix") or last ("suffix") H
    bases.  The best alignment then starts in column 1 or ends in column H, so a dropped or doubled border column moves
    the sum far more than the tolerance.
  * tracks: quality, insertion, deletion and GCP bytes differ on every row and use all of 0..255 (the kernel and the
    restatement mask with 127).  Seven rows of eight take a phred of 16..63 with a random top bit, the eighth any byte:
    with uniform bytes a read of a few hundred rows underflows float every time and only the double kernels would be
    tested on long reads.  Rows 1, R and the first and last row of lanes 0, 1, G - 1 and of the lane that owns row R
    get a 0 or a 127 in one track.
  * odd bytes, one kind per grid cell in turn: N in the read at row 1 / row R, N in the haplotype at column 1 / column
    H, lower-case bases, a read byte 0 (the haplotype's LDS padding is zeros) and a read byte 255.
  * rows that have no haplotype base to stand against (R > H) can only be inserted; their GCP is 0 or 1 with a random
    top bit, their other tracks any byte (see _cell).
  * no pair's float sum lies within [1e-30, 1e-26] of MIN_ACCEPTED = 1e-28: a read that comes closer is drawn again, so
    that which pairs are rescued in double cannot depend on rounding.
"""
import collections
import functools

import numpy as np

import pairhmm_oracle_lib as pol

SEED = 20260
BAND = (1e-30, 1e-26)                 # around MIN_ACCEPTED = 1e-28 (pairhmm_kernels.hip:34)
LDS_PLAIN, LDS_MAX = 64 * 1024, 160 * 1024   # above the first a launch sets the function attribute (:663); the second is the CU's LDS
MAX_PAIRS = 300000
ACGT = np.frombuffer(b"ACGT", np.uint8)

# lanes per pair -> read lengths of the seam grid, and the read lengths of each call (split by longest read so that
# every KMAX instantiation is launched; the last call of 21 and 32 is the read that makes the host fall back to 64)
GRID_R = {
    16: (1, 2, 15, 16, 17, 31, 32, 33, 48, 49),
    21: (1, 2, 20, 21, 22, 41, 42, 43, 62, 63, 64, 83, 84, 85, 104, 105, 106),
    32: (1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 159, 160, 161),
    64: (1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 258, 511, 512, 513),
}
GRID_CALL_MAX = {16: (49,), 21: (84, 105, 106), 32: (128, 160, 161), 64: (64, 128, 192, 513)}
KMAX_ROWS = {16: 1, 21: 5, 32: 5, 64: 4}


def grid_h(G):
    return (1, 2, 3, 4, 5, 7, 8, 9, G - 1, G, G + 1, G + 7, G + 8, G + 9, 2 * G + 1)


def grid_call_r(rows, call):
    """Read lengths of one call: everything up to the call's longest read; the fallback read goes alone."""
    top = GRID_CALL_MAX[rows][call]
    if rows in (21, 32) and call == 2:
        return (top,)
    return tuple(r for r in GRID_R[rows] if r <= top)


def lds_bytes(hap_cap, rows, elem_bytes):
    """ph_lds_bytes, pairhmm_kernels.hip:651-657: per group a ring of hap_cap + 2 rows + 16 carries of three elements
    and (hap_cap + 2 rows + 35) & ~7 haplotype bytes; 64 / rows groups per wave, one wave per block."""
    ring_entries = hap_cap + 2 * rows + 16
    hap_bytes = (hap_cap + 2 * rows + 28 + 7) & ~7
    return (64 // rows) * (ring_entries * 3 * elem_bytes + hap_bytes)


def max_fit(rows, elem_bytes, limit):
    """Largest haplotype length whose carve is at most `limit` bytes."""
    lo, hi = 1, 1 << 20
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if lds_bytes(mid, rows, elem_bytes) <= limit:
            lo = mid
        else:
            hi = mid - 1
    return lo


def max_haplotype_len():
    """mgl_pairhmm_max_haplotype_len (pairhmm_capi.cpp:117-128,240-245): the 64-lane double carve bounds both modes."""
    return max_fit(64, 8, LDS_MAX)


Variant = collections.namedtuple("Variant", "float_kernel float_rows float_kmax float_k double_kernel double_rows double_kmax double_k")


def variant(n_pairs, max_read, max_hap, forced_rows, use_double, pair_r=None, flags=None):
    """Which kernels a call launches: mirrors run_device (pairhmm_capi.cpp:167-197), launch_pairhmm_float / _double
    (pairhmm_kernels.hip:675-699) and the K dispatch of pairhmm_wave / pairhmm_wave_multi (:552-560, :586-594).
    Returns the kernel names, their KMAX template argument (0 for the 16-lane kernels, which have none) and, given the
    pairs' read lengths in list order, the rows per lane K each wave takes (float pass: every wave; double pass: every
    pair in double mode, the pairs in `flags` otherwise).  It exists so that the CPU test can assert coverage."""
    rows = forced_rows
    if not rows:
        rows = 64 if (max_read >= 48 and lds_bytes(max_hap, 16, 4) > 12 * 1024) else 16
        if n_pairs > 1024 and 24 <= max_read <= 160:
            slots21, slots32 = 21 * ((max_read + 20) // 21), 32 * ((max_read + 31) // 32)
            ok21 = max_read <= 105 and lds_bytes(max_hap, 21, 4) <= 24 * 1024
            ok32 = lds_bytes(max_hap, 32, 4) <= 24 * 1024
            if ok21 and (slots21 <= slots32 or not ok32):
                rows = 21
            elif ok32:
                rows = 32
            elif max_read > 64:
                rows = 64
    if rows == 32 and (max_read > 160 or lds_bytes(max_hap, 32, 4) > LDS_MAX):
        rows = 64
    if rows == 21 and (max_read > 105 or lds_bytes(max_hap, 21, 4) > LDS_MAX):
        rows = 64
    if lds_bytes(max_hap, rows, 4) > LDS_MAX:
        rows = 64
    rows_d = 16 if (lds_bytes(max_hap, 16, 8) <= LDS_MAX and rows == 16) else 64
    rpl = min(4, (max_read + 63) // 64)
    rpl_f = max(3, (max_read + 31) // 32) if rows == 32 else max(3, (max_read + 20) // 21) if rows == 21 else rpl

    def k64(kmax, r):
        return min(kmax, (r + 63) >> 6)

    fk, fkmax, fks = None, 0, ()
    if not use_double:
        if rows == 16:
            fk, fkmax = "pairhmm_float_kernel", 0
        elif rows == 64:
            fk, fkmax = "pairhmm_float64_kernel", rpl
        else:
            fk, fkmax = "pairhmm_float%d_kernel" % rows, (4 if rpl_f <= 4 else 5)
        if pair_r is not None:
            pw = 64 // rows
            if rows == 16:
                fks = (1,) * ((len(pair_r) + pw - 1) // pw)
            elif rows == 64:
                fks = tuple(k64(fkmax, int(r)) for r in pair_r)
            else:
                ks = []
                for w in range(0, len(pair_r), pw):
                    k = min(fkmax, (int(max(pair_r[w:w + pw])) + rows - 1) // rows)
                    ks.append(2 if k <= 2 else 3 if k == 3 else 4 if (fkmax == 4 or k == 4) else 5)
                fks = tuple(ks)
    dk, dkmax = ("pairhmm_double_kernel", 0) if rows_d == 16 else ("pairhmm_double64_kernel", rpl)
    dks = ()
    if pair_r is not None:
        ran = range(len(pair_r)) if use_double else ([] if flags is None else np.flatnonzero(flags))
        dks = tuple(1 if rows_d == 16 else k64(dkmax, int(pair_r[i])) for i in ran)
    return Variant(fk, rows, fkmax, fks, dk, rows_d, dkmax, dks)


class Case:
    """Packed pools and a pair list.  `root` / `idx`: the list this one was taken from and each pair's place in it."""

    def __init__(self, name, reads, read_off, haps, hap_off, pair_read, pair_hap, kind=None, root=None, idx=None):
        self.name = name
        self.reads, self.read_off, self.haps, self.hap_off = reads, read_off, haps, hap_off
        self.pair_read = np.ascontiguousarray(pair_read, dtype=np.int32)
        self.pair_hap = np.ascontiguousarray(pair_hap, dtype=np.int32)
        self.kind = kind  # per pair: "prefix" / "suffix" where the pair was built for a border column
        self.root = root if root is not None else self
        self.idx = idx if idx is not None else np.arange(len(self.pair_read))
        self.n = len(self.pair_read)
        self.R = np.diff(read_off)[self.pair_read]
        self.H = np.diff(hap_off)[self.pair_hap]
        self.max_read, self.max_hap = int(self.R.max()), int(self.H.max())

    def take(self, sel, name):
        sel = np.asarray(sel)
        kind = None if self.kind is None else [self.kind[i] for i in sel]
        return Case(name, self.reads, self.read_off, self.haps, self.hap_off, self.pair_read[sel], self.pair_hap[sel], kind,
                    self.root, self.idx[sel])

    def compact(self):
        """The same pair list over pools that hold only the reads and haplotypes it uses (the host entries take the
        longest read and haplotype from the pools)."""
        ur, ir = np.unique(self.pair_read, return_inverse=True)
        uh, ih = np.unique(self.pair_hap, return_inverse=True)
        reads = [[np.frombuffer(t, np.uint8) for t in self.read(int(r))] for r in ur]
        haps = [np.frombuffer(self.hap(int(h)), np.uint8) for h in uh]
        return _pack(self.name + "/compact", reads, haps, ir, ih, self.kind)

    def read(self, r):
        """(bases, quals, ins, del, gcp) of pool read r as bytes."""
        n = int(self.read_off[r + 1] - self.read_off[r])
        b = 5 * int(self.read_off[r])
        return tuple(self.reads[b + t * n: b + (t + 1) * n].tobytes() for t in range(5))

    def hap(self, h):
        return self.haps[int(self.hap_off[h]): int(self.hap_off[h + 1])].tobytes()

    def forward_float(self, k):
        rd = self.read(int(self.pair_read[k]))
        hp = self.hap(int(self.pair_hap[k]))
        return float(pol.oracle().pho_forward_float(pol.Read(len(rd[0]), *rd), hp, len(hp)))


def _pack(name, reads, haps, pair_read, pair_hap, kind=None):
    roff = np.zeros(len(reads) + 1, np.int64)
    roff[1:] = np.cumsum([len(r[0]) for r in reads])
    hoff = np.zeros(len(haps) + 1, np.int64)
    hoff[1:] = np.cumsum([len(h) for h in haps])
    rd = np.concatenate([np.asarray(t, np.uint8) for r in reads for t in r])
    hd = np.concatenate([np.asarray(h, np.uint8) for h in haps])
    return Case(name, rd, roff, hd, hoff, pair_read, pair_hap, kind)


def _forward_float(read, hap):
    rd = tuple(np.asarray(t, np.uint8).tobytes() for t in read)
    hp = np.asarray(hap, np.uint8).tobytes()
    return float(pol.oracle().pho_forward_float(pol.Read(len(rd[0]), *rd), hp, len(hp)))


def _forward_double(read, hap):
    rd = tuple(np.asarray(t, np.uint8).tobytes() for t in read)
    hp = np.asarray(hap, np.uint8).tobytes()
    return float(pol.oracle().pho_forward_double(pol.Read(len(rd[0]), *rd), hp, len(hp)))


def in_band(v):
    return BAND[0] <= v <= BAND[1]


def usable(read, hap):
    """The float sum is clear of MIN_ACCEPTED and the double sum is a normal number (its log10 is finite)."""
    return not in_band(_forward_float(read, hap)) and 1e-300 < _forward_double(read, hap) < float("inf")


def border_shift(read, hap, kind):
    """How far log10 moves when the haplotype loses the column the read was built for: its last base (suffix reads)
    or its first (prefix reads).  Cells are drawn until this is more than 1e-3, a hundred times the GPU test's
    tolerance, so no kernel that drops or doubles that column can pass."""
    rd = tuple(np.asarray(t, np.uint8).tobytes() for t in read)
    hp = np.asarray(hap, np.uint8).tobytes()
    full, _ = pol.log10_likelihood(hp, *rd, use_double=True)
    cut, _ = pol.log10_likelihood(hp[:-1] if kind == "suffix" else hp[1:], *rd, use_double=True)
    return abs(full - cut)


def symmetric(bases):
    """A one-row read of N matches every column and one of another odd byte none: its sum is H equal terms of
    INITIAL / H whatever H is, and no column stands out."""
    return len(bases) == 1 and int(bases[0]) not in b"ACGT"


def special_rows(R, G):
    """Rows 1 and R and the first and last row of lanes 0, 1, G - 1 and of the lane that owns row R, under the numbering
    of pairhmm_body_k (pairhmm_kernels.hip:406,462): K rows per lane, pad virtual rows in front."""
    K = min(KMAX_ROWS[G], max(2 if G in (21, 32) else 1, -(-R // G)))
    pad = (K - R % K) % K
    last_lane = ((R + pad) // K - 1) % G
    rows = {1, R}
    for stripe0, L in ((0, 0), (0, 1), (0, G - 1), ((R + pad - 1) // (G * K), last_lane)):
        for j in (0, K - 1):
            rows.add((stripe0 * G + L) * K + j + 1 - pad)
    return sorted(r for r in rows if 1 <= r <= R)


def varied_tracks(rng, R, G, unmatched=None):
    """Four tracks that differ on every row (see the module docstring).  `unmatched`: the rows (0-based slice) that have
    no haplotype base to stand against and can only be inserted."""
    t = (rng.integers(16, 64, size=(4, R)) | (rng.integers(0, 2, size=(4, R)) << 7)).astype(np.uint8)
    wild = rng.random((4, R)) < 0.125
    t[wild] = rng.integers(0, 256, size=int(wild.sum())).astype(np.uint8)
    if unmatched is not None:
        n = len(range(*unmatched.indices(R)))
        t[:3, unmatched] = rng.integers(0, 256, size=(3, n)).astype(np.uint8)
        t[3, unmatched] = ((rng.random(n) < 0.4).astype(np.uint8) | (rng.integers(0, 2, n) << 7)).astype(np.uint8)
    for n, row in enumerate(special_rows(R, G)):
        t[(n // 2) % 4, row - 1] = 127 if n % 2 == 0 else 0
    return [t[0], t[1], t[2], t[3]]


def _other_base(rng, b):
    return ACGT[(int(np.flatnonzero(ACGT == b)[0]) + int(rng.integers(1, 4))) % 4]


def _cell(rng, R, H, G, deco):
    """One grid cell: a haplotype and its prefix and suffix read (module docstring), with odd bytes of kind `deco`."""
    hap = ACGT[rng.integers(0, 4, H)]
    if R <= H:
        pre, suf = hap[:R].copy(), hap[H - R:].copy()
        for i in np.flatnonzero(rng.random(R) < 0.02):
            suf[i] = _other_base(rng, suf[i])
    else:
        pre = np.concatenate([hap, ACGT[rng.integers(0, 4, R - H)]])
        suf = np.concatenate([ACGT[rng.integers(0, 4, R - H)], hap])
    hap = hap.copy()
    if deco == 1:
        pre[0] = suf[0] = ord("N")
    elif deco == 2:
        pre[R - 1] = suf[R - 1] = ord("N")
    elif deco == 3:
        hap[0] = ord("N")
    elif deco == 4:
        hap[H - 1] = ord("N")
    elif deco == 5:
        pre[R // 2] |= 0x20
        suf[R // 3] |= 0x20
        hap[H // 2] |= 0x20
    elif deco == 6:
        pre[0] = suf[R - 1] = 0
    elif deco == 7:
        pre[R - 1] = suf[0] = 255
    # rows without a haplotype base can only be inserted: behind the copy in the prefix read; in the suffix read row 1
    # has to stand in column 1 (row 0 holds no M or X to insert from), so rows 2 .. R - H + 1.  Their GCP is 0 or 1
    # (top bit random): at the usual phreds every inserted row costs 1.6 to 6.3 orders of magnitude and the 384 of a
    # 513-base read against 129 columns would underflow double, let alone float.
    free = (None, None) if R <= H else (slice(H, R), slice(1, R - H + 1))
    out = []
    for bases, unmatched, kind in zip((pre, suf), free, ("prefix", "suffix")):
        for _ in range(64):
            rd = [bases] + varied_tracks(rng, R, G, unmatched)
            if usable(rd, hap) and (border_shift(rd, hap, kind) > 1e-3 or H < 2 or symmetric(bases)):
                break
        else:
            raise AssertionError("no draw of the tracks keeps the float sum off MIN_ACCEPTED")
        out.append(rd)
    return hap, out[0], out[1]


@functools.lru_cache(maxsize=None)
def grid(rows):
    """The whole seam grid of one lane group, R-major: for R, for H, the prefix then the suffix read."""
    reads, haps, pr, ph, kind = [], [], [], [], []
    for ri, R in enumerate(GRID_R[rows]):
        for hi, H in enumerate(grid_h(rows)):
            rng = np.random.default_rng([SEED, rows, R, H])
            hap, pre, suf = _cell(rng, R, H, rows, (ri * 15 + hi) % 8)
            haps.append(hap)
            for rd, kd in ((pre, "prefix"), (suf, "suffix")):
                pr.append(len(reads))
                ph.append(len(haps) - 1)
                kind.append(kd)
                reads.append(rd)
    return _pack("grid%d" % rows, reads, haps, pr, ph, kind)


def grid_call(rows, call):
    g = grid(rows)
    want = set(grid_call_r(rows, call))
    return g.take(np.flatnonzero([int(r) in want for r in g.R]), "grid%d/call%d" % (rows, call))


def permuted(case):
    """A fixed permutation: a wave's groups then differ in R, H and N content."""
    return case.take(np.random.default_rng([SEED, case.n]).permutation(case.n), case.name + "/permuted")


def cuts(case, rows):
    """The list cut to n = 1, 2, ... (mod pairs per wave): a partly filled last wave."""
    pw = 64 // rows
    out = []
    for m in range(1, pw):
        n = case.n - ((case.n - m) % pw)
        out.append(case.take(np.arange(n), "%s/cut%d" % (case.name, m)))
    return out


# ---------------------------------------------------------------------------------------------------------- mixed waves
@functools.lru_cache(maxsize=None)
def mixed(rows):
    """Waves whose groups are at opposite extremes: (R, H) = (1, 1) beside (G Kmax, 330); a haplotype with N beside ones
    without; a read that ends in stripe 0 beside one of three stripes of 16 rows.  Every extreme stands at every group
    position once.  Laid out for `rows` lanes per pair (64 / rows pairs per wave)."""
    rng = np.random.default_rng([SEED, 77, rows])
    pw = 64 // rows
    big_r = rows * KMAX_ROWS[rows] if rows != 16 else 48
    hap330 = ACGT[rng.integers(0, 4, 330)]
    hap40 = ACGT[rng.integers(0, 4, 40)]
    hap40n = hap40.copy()
    hap40n[17] = ord("N")
    haps = [np.frombuffer(b"C", np.uint8), hap330, hap40, hap40n]
    # the one-row read at phred 17: a column counted behind its haplotype's only one (a mismatch against the LDS padding,
    # 0.02 / 3 of INITIAL each) shows at once when the neighbour has 330 of them
    reads = [[np.frombuffer(b"C", np.uint8)] + [np.array([b], np.uint8) for b in (17 | 128, 45, 72 | 128, 10)],
             [hap330[330 - big_r:].copy()] + varied_tracks(rng, big_r, rows),
             [hap40[8:38].copy()] + varied_tracks(rng, 30, rows),
             [hap40[:5].copy()] + varied_tracks(rng, 5, rows),
             [np.concatenate([hap40, ACGT[rng.integers(0, 4, 8)]])] + varied_tracks(rng, 48, rows, slice(40, 48))]
    small, big, plain, with_n, short, three = (0, 0), (1, 1), (2, 2), (2, 3), (3, 2), (4, 2)
    pairs = []
    for a, b in ((small, big), (big, small), (plain, with_n), (short, three)):
        for pos in range(pw):
            wave = [a] * pw
            wave[pos] = b
            pairs += wave
    for r, h in set(pairs):
        assert usable(reads[r], haps[h]), (r, h)
    return _pack("mixed%d" % rows, reads, haps, [p[0] for p in pairs], [p[1] for p in pairs])


# --------------------------------------------------------------------------------------------------------------- rescue
def _mismatched(rng, hap, start, R, n_mis, q):
    bases = hap[start:start + R].copy()
    for i in np.linspace(2, R - 3, n_mis).astype(int) if n_mis else ():
        bases[i] = _other_base(rng, bases[i])
    return [bases, np.full(R, q, np.uint8), np.full(R, 60, np.uint8), np.full(R, 60, np.uint8), np.full(R, 40, np.uint8)]


@functools.lru_cache(maxsize=None)
def _rescue_pool():
    """Reads of 60 bases with 0 .. 16 mismatches at phred 60 (3.3e-7 each, against 2^120 = 1.3e36 at the start; gaps at
    phred 60, continued at 40, are no cheaper way round): the float sum falls on either side of MIN_ACCEPTED.  Only reads
    whose float sum is outside BAND are kept.  The long reads (100, 170 and 300 bases, all flagged) take two, three and
    four rows per lane of the 64-lane rescue; the last one takes two stripes there and nineteen on 16 lanes."""
    rng = np.random.default_rng([SEED, 88])
    hap = ACGT[rng.integers(0, 4, 80)]
    hap_long = ACGT[rng.integers(0, 4, 330)]
    reads, flagged = [], []
    for n_mis in (0, 2, 4, 6, 9, 10, 11, 12, 14, 16):
        rd = _mismatched(rng, hap, 10, 60, n_mis, 60)
        v = _forward_float(rd, hap)
        if not in_band(v):
            reads.append(rd)
            flagged.append(v < 1e-28)
    n_short = len(reads)
    for R in (100, 170, 300):
        for n_mis in (14, 16, 20):
            rd = _mismatched(rng, hap_long, 20, R, n_mis, 60)
            v = _forward_float(rd, hap_long)
            if not in_band(v) and v < 1e-28:
                reads.append(rd)
                flagged.append(True)
                break
        else:
            raise AssertionError("no long read falls clear of MIN_ACCEPTED")
    return reads, [hap, hap_long], np.array(flagged), n_short


def rescue_cases(rows):
    """Pair lists for `rows` lanes per pair: one flagged pair alone in a wave of unflagged ones at each group position,
    the flagged long reads among short unflagged ones, all flagged, none flagged."""
    reads, haps, flagged, n_short = _rescue_pool()
    pw = 64 // rows
    F = [i for i in range(n_short) if flagged[i]]
    U = [i for i in range(n_short) if not flagged[i]]
    assert F and U
    solo = []
    for pos in range(pw):
        wave = [U[(pos + g) % len(U)] for g in range(pw)]
        wave[pos] = F[pos % len(F)]
        solo += wave + [U[g % len(U)] for g in range(pw)]
    long_ = [U[0]] * pw + [U[1 % len(U)], n_short + 2, n_short, U[0], n_short + 1] + [U[0]] * pw
    out = []
    for name, lst in (("solo", solo), ("long", long_), ("all", (F * 9)[:9]), ("none", (U * 9)[:9])):
        out.append(_pack("rescue%d/%s" % (rows, name), reads, haps, lst, [1 if r >= n_short else 0 for r in lst]))
    return out


SWEEP_GRID, SWEEP_N = 4096, 4096 * 64 + 64 + 3   # blocks of the rescue sweep (pairhmm_kernels.hip:669), 64 flags a step


@functools.lru_cache(maxsize=None)
def sweep():
    """More pairs than one turn of the rescue sweep covers (pairhmm_kernels.hip:638): a pool of twelve reads and twelve
    haplotypes of at most 12 bases; flagged pairs at the ends of the first step, of the first turn, of the list, and a
    sprinkle between.  Flagged reads are A's at phred 127 in every track against haplotypes without A: every row costs
    1e-12.7 or more, the float sum underflows; unflagged reads copy the haplotype they come from at phred 20."""
    rng = np.random.default_rng([SEED, 99])
    cgt = np.frombuffer(b"CGT", np.uint8)
    haps = [cgt[rng.integers(0, 3, n)] for n in range(1, 13)]
    reads = []
    for k in range(6):
        n = 2 * k + 1 + (k % 2)
        reads.append([haps[11][:n].copy(), np.full(n, 20, np.uint8), np.full(n, 40, np.uint8), np.full(n, 40, np.uint8), np.full(n, 10, np.uint8)])
    for k in range(6):
        n = 7 + k
        reads.append([np.full(n, ord("A"), np.uint8)] + [np.full(n, 127, np.uint8)] * 4)
    for r, rd in enumerate(reads):
        for hp in haps:
            v = _forward_float(rd, hp)
            assert not in_band(v) and (v < 1e-28) == (r >= 6), (r, v)
    n = SWEEP_N
    turn = SWEEP_GRID * 64
    spots = np.unique(np.concatenate([[0, 63, 64, turn - 1, turn, n - 1], rng.integers(0, n, 300)]))
    pr = rng.integers(0, 6, n)
    pr[spots] = 6 + rng.integers(0, 6, len(spots))
    c = _pack("sweep", reads, haps, pr, rng.integers(0, 12, n))
    c.flagged_at = spots
    return c


# ------------------------------------------------------------------------------------------------------------ LDS edges
LdsCase = collections.namedtuple("LdsCase", "name rows use_double case")
# longest read of the call -> the KMAX instantiation (pairhmm_capi.cpp:196-197, pairhmm_kernels.hip:675-699)
LDS_COMPANION = {16: (0,), 21: (63, 105), 32: (96, 160), 64: (0, 128, 192, 256)}


def _lds_case(name, rows, use_double, H, companion):
    """One haplotype of H bases with a prefix read (37 rows), a suffix read (40 rows) and a read that needs the rescue
    (33 lower-case bases at phred 127); `companion`: a read of that length against a haplotype of 9 bases, which only
    sets the call's longest read and so the KMAX instantiation."""
    rng = np.random.default_rng([SEED, 55, rows, H, companion, int(use_double)])
    G = rows if rows else 16
    hap = ACGT[rng.integers(0, 4, H)]
    reads = [[hap[:37].copy()] + varied_tracks(rng, 37, G), [hap[H - 40:].copy()] + varied_tracks(rng, 40, G),
             [np.full(33, ord("a"), np.uint8)] + [np.full(33, 127, np.uint8)] * 4]
    haps = [hap]
    pr, ph = [0, 1, 2], [0, 0, 0]
    if companion:
        small = ACGT[rng.integers(0, 4, 9)]
        reads.append([np.concatenate([small, ACGT[rng.integers(0, 4, companion - 9)]])] + varied_tracks(rng, companion, G, slice(9, companion)))
        haps.append(small)
        pr.append(3)
        ph.append(1)
    for r, h in zip(pr, ph):
        assert usable(reads[r], haps[h]), (name, r, h)
    return LdsCase(name, rows, use_double, _pack(name, reads, haps, pr, ph))


def lds_specs():
    """(name, rows, use_double, H, companion) of the LDS-edge calls, pure arithmetic: the last haplotype length at which a
    kernel's carve is a plain 64 KiB launch and the first that needs the function attribute, for every instantiation; the
    last length at which four float (double) rings of the 16-lane kernel fit the CU's 160 KiB and the first at which the
    host falls back to 64 lanes; and the longest haplotype the library takes."""
    out = []
    for rows in (16, 21, 32, 64):
        fit = max_fit(rows, 4, LDS_PLAIN)
        for comp in LDS_COMPANION[rows]:
            for H in (fit, fit + 1):
                out.append(("lds/plain/float%d/r%d/h%d" % (rows, comp, H), rows, False, H, comp))
    for rows in (16, 64):
        fit = max_fit(rows, 8, LDS_PLAIN)
        for comp in LDS_COMPANION[rows]:
            for H in (fit, fit + 1):
                out.append(("lds/plain/double%d/r%d/h%d" % (rows, comp, H), rows, True, H, comp))
    for elem, dbl_modes in ((4, (False,)), (8, (False, True))):
        fit = max_fit(16, elem, LDS_MAX)
        for H in (fit, fit + 1):
            for dbl in dbl_modes:
                out.append(("lds/cu/%s16/%s/h%d" % ("float" if elem == 4 else "double", "double" if dbl else "float", H), 16, dbl, H, 0))
    for dbl in (False, True):
        out.append(("lds/longest/%s" % ("double" if dbl else "float"), 0, dbl, max_haplotype_len(), 0))
    return out


@functools.lru_cache(maxsize=None)
def lds_case(name):
    spec = {s[0]: s for s in lds_specs()}[name]
    return _lds_case(*spec)


def lds_cases():
    return tuple(lds_case(s[0]) for s in lds_specs())
