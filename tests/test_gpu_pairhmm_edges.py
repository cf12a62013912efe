"""The PairHMM kernels at their seams (cases: pairhmm_cases.py; what they reach: test_pairhmm_cases.py).  Every case goes
through the device-resident entry with `out` and `used_double` 16 entries longer than the pair list and prefilled, and is
compared with the restatement of the same mode under the tolerances of test_gpu_pairhmm.py: 1e-5 on log10 for pairs
computed in float, 1e-9 relative for pairs computed in double.  Which pairs were rescued is compared element by element.
Between two runs of the same pairs (another order, another lane group) float results agree within 2e-6, the bound
test_two_pairs_per_wave uses between instantiations, and double results within 1e-9 relative."""
import numpy as np
import pytest
import torch

import pairhmm_cases as pc
import pairhmm_oracle_lib as pol
from mgl_amd import pairhmm

pytestmark = pytest.mark.gpu

PAD = 16
CANARY_OUT = -7.25e300
CANARY_USED = 0x5A5A5A5A


@pytest.fixture(scope="module")
def hmm():
    p = pairhmm.MicrosoftPairHmm(0)
    assert p.load(), "libmgl_pairhmm_hip.so could not create a GPU context"
    yield p
    p.done()


_pools = {}
_refs = {}


def _device_pools(case):
    key = id(case.reads)
    if key not in _pools:
        dev = torch.device("cuda", 0)
        _pools[key] = (case.reads, tuple(torch.from_numpy(a).to(dev) for a in (case.reads, case.read_off, case.haps, case.hap_off)))
    return _pools[key][1]


def run(hmm, case, rows, use_double, max_read=None, max_hap=None):
    """One call of mgl_pairhmm_compute_pairs_device; asserts the canaries behind the pair list and, in double mode, what
    include/mgl_pairhmm.h says of d_used_double there: it is not written.  Returns (log10 likelihoods, used_double)."""
    dev = torch.device("cuda", 0)
    hmm.initialize(pairhmm.PairHMMNativeArguments(use_double, 1))
    hmm.set_stripe_rows(rows)
    rd, roff, hd, hoff = _device_pools(case)
    out = torch.full((case.n + PAD,), CANARY_OUT, dtype=torch.float64, device=dev)
    used = torch.full((case.n + PAD,), CANARY_USED, dtype=torch.int32, device=dev)
    try:
        hmm.compute_pairs_device(rd, roff, hd, hoff, torch.from_numpy(case.pair_read).to(dev), torch.from_numpy(case.pair_hap).to(dev),
                                 max_read or case.max_read, max_hap or case.max_hap, out, used)
        torch.cuda.synchronize()
    finally:
        hmm.set_stripe_rows(0)
    o, u = out.cpu().numpy(), used.cpu().numpy()
    assert (o[case.n:] == CANARY_OUT).all(), "out written behind n_pairs"
    assert (u[case.n:] == CANARY_USED).all(), "used_double written behind n_pairs"
    assert (o[:case.n] != CANARY_OUT).all(), "a pair got no result"
    if use_double:
        assert (u == CANARY_USED).all(), "double mode rescues nothing and leaves used_double alone"
    return o[:case.n], u[:case.n]


def ref(case, use_double):
    """The restatement's answers for the case's pairs: one run per root list and mode, shared by every order of it."""
    key = (id(case.root), use_double)
    if key not in _refs:
        r = case.root
        want, used = pol.compute_pairs(r.reads, r.read_off, r.haps, r.hap_off, r.pair_read, r.pair_hap, use_double, nthreads=4)
        assert np.isfinite(want).all()
        want.setflags(write=False)
        used.setflags(write=False)
        _refs[key] = (r, want, used)
    _, want, used = _refs[key]
    return want[case.idx], used[case.idx]


def check(case, got, used, use_double, what=""):
    want, wused = ref(case, use_double)
    assert np.isfinite(got).all(), (case.name, what)
    if not use_double:
        bad = np.flatnonzero(used != wused)
        assert bad.size == 0, (case.name, what, "rescue flags differ at", bad[:8], used[bad[:8]], wused[bad[:8]])
    dbl = (wused != 0) | use_double
    err = np.abs(got - want)
    bad = np.flatnonzero(dbl & ~(err < 1e-9 * np.maximum(1.0, np.abs(want))))
    assert bad.size == 0, (case.name, what, "double", bad[:8], case.R[bad[:8]], case.H[bad[:8]], got[bad[:8]], want[bad[:8]])
    bad = np.flatnonzero(~dbl & ~(err < 1e-5))
    assert bad.size == 0, (case.name, what, "float", bad[:8], case.R[bad[:8]], case.H[bad[:8]], got[bad[:8]], want[bad[:8]])
    return dbl


def agree(a, b, dbl, what):
    d = np.abs(a - b)
    assert (d[dbl] < 1e-9 * np.maximum(1.0, np.abs(a[dbl]))).all(), (what, d[dbl].max())
    assert (d[~dbl] < 2e-6).all(), (what, d[~dbl].max(), int(np.argmax(np.where(dbl, 0, d))))


GRID_CALLS = [(rows, call) for rows in (16, 21, 32, 64) for call in range(len(pc.GRID_CALL_MAX[rows]))]


@pytest.mark.parametrize("use_double", [False, True], ids=["float", "double"])
@pytest.mark.parametrize("rows,call", GRID_CALLS, ids=["rows%d-call%d" % rc for rc in GRID_CALLS])
def test_seam_grid(hmm, rows, call, use_double):
    """One call of a seam grid, R-major (a wave's groups share R), in a fixed permutation (they differ in R, H and N
    content), cut to every remainder of pairs per wave, and with the lane group left to the host.  The last call of the
    21- and 32-lane grids is the read the host has to take on 64 lanes instead."""
    c = pc.grid_call(rows, call)
    p = pc.permuted(c)
    got_c, used_c = run(hmm, c, rows, use_double)
    dbl_c = check(c, got_c, used_c, use_double, "R-major")
    got_p, used_p = run(hmm, p, rows, use_double)
    dbl_p = check(p, got_p, used_p, use_double, "permuted")
    place = {int(r): i for i, r in enumerate(c.idx)}
    back = np.array([place[int(r)] for r in p.idx])
    agree(got_p, got_c[back], dbl_p, "permuted against R-major")
    for cut in pc.cuts(p, rows):
        got, used = run(hmm, cut, rows, use_double)
        check(cut, got, used, use_double, "cut")
        agree(got, got_p[:cut.n], dbl_p[:cut.n], cut.name)
    for lst, forced, dbl in ((c, got_c, dbl_c), (p, got_p, dbl_p)):
        got, used = run(hmm, lst, 0, use_double)
        check(lst, got, used, use_double, "rows 0")
        agree(got, forced, dbl, lst.name + " rows 0 against forced")


@pytest.mark.parametrize("use_double", [False, True], ids=["float", "double"])
@pytest.mark.parametrize("rows", [16, 21, 32, 64])
def test_mixed_waves(hmm, rows, use_double):
    """Neighbouring groups at opposite extremes: the wave-wide stripe count, K, h_min / h_max and any_n are driven by one
    group while another needs the least of each."""
    m = pc.mixed(rows)
    got, used = run(hmm, m, rows, use_double)
    dbl = check(m, got, used, use_double)
    for other in (0, 64):
        again, used2 = run(hmm, m, other, use_double)
        check(m, again, used2, use_double, "rows %d" % other)
        agree(again, got, dbl, "%s rows %d against %d" % (m.name, other, rows))


@pytest.mark.parametrize("rows", [16, 21, 32, 64, 0])
def test_rescue_by_pair(hmm, rows):
    """Which pairs are rescued, not how many: one flagged pair alone in a wave at each group position (the 16-lane rescue
    skips a wave by ballot), flagged reads of two to four rows per lane and two stripes in the 64-lane rescue, all
    flagged, none flagged."""
    for c in pc.rescue_cases(rows or 16):
        got, used = run(hmm, c, rows, False)
        dbl = check(c, got, used, False)
        kind = c.name.split("/")[1]
        assert kind != "all" or dbl.all()
        assert kind != "none" or not dbl.any()
        assert kind not in ("solo", "long") or (dbl.any() and not dbl.all())
        again, unwritten = run(hmm, c, rows, True)
        check(c, again, unwritten, True)
        agree(again[dbl], got[dbl], np.ones(int(dbl.sum()), bool), c.name + " rescued against double mode")


@pytest.mark.parametrize("rows", [64, 16])
def test_rescue_sweep_turns_its_loop(hmm, rows):
    """4096 x 64 + 64 + 3 pairs: the sweep of pairhmm_double64_kernel (4096 blocks, 64 flags a step) takes a second turn,
    with flagged pairs at both ends of the first step, of the first turn and of the list; on 16 lanes the same list is
    the ballot skip with waves of none, one and more flagged pairs."""
    s = pc.sweep()
    got, used = run(hmm, s, rows, False)
    check(s, got, used, False)
    assert (np.flatnonzero(used) == s.flagged_at).all()


LDS_NAMES = [spec[0] for spec in pc.lds_specs()]


@pytest.mark.parametrize("name", LDS_NAMES)
def test_lds_edges(hmm, name):
    """Either side of 64 KiB of dynamic LDS for every instantiation, either side of the 160 KiB at which four rings of 16
    lanes stop fitting (the host falls back to 64 lanes: results, not an error), and the longest haplotype there is."""
    lc = pc.lds_case(name)
    got, used = run(hmm, lc.case, lc.rows, lc.use_double)
    check(lc.case, got, used, lc.use_double)


def test_longest_haplotype_is_the_carve_formula(hmm):
    assert pairhmm.lib().mgl_pairhmm_max_haplotype_len(0) == pc.max_haplotype_len()
    assert pairhmm.lib().mgl_pairhmm_max_haplotype_len(1) == pc.max_haplotype_len()


@pytest.mark.parametrize("rows", [16, 32, 64])
def test_length_bounds_may_exceed_the_batch(hmm, rows):
    """include/mgl_pairhmm.h: max_read_len / max_hap_len "bound the lengths in the batch" -- upper bounds, not the exact
    maxima.  Larger ones size the LDS carve and pick KMAX (64 lanes: a read bound of 200 launches float64<4> for reads of
    at most 128 rows); the answers stay within the tolerances."""
    c = pc.permuted(pc.grid_call(rows, 1 if rows != 16 else 0))
    exact, used = run(hmm, c, rows, False)
    dbl = check(c, exact, used, False)
    # 32 lanes: the batch's longest read is 160 already and a larger bound would leave the lane group
    read_bound = {16: c.max_read + 7, 32: c.max_read, 64: 200}[rows]
    assert c.max_read <= read_bound and (rows != 64 or c.max_read == 128)
    got, used = run(hmm, c, rows, False, read_bound, c.max_hap + 13)
    check(c, got, used, False, "larger bounds")
    agree(got, exact, dbl, "larger bounds against exact")


def test_host_and_jni_entries_equal_the_device_entry(hmm):
    """The permuted 32-lane grid through mgl_pairhmm_compute_pairs, and a region of its reads and haplotypes through
    mgl_pairhmm_compute_likelihoods: bit for bit what the device entry gives (test_device_resident_entry)."""
    c = pc.permuted(pc.grid_call(32, 1)).compact()
    dev, used = run(hmm, c, 32, False)
    check(c, dev, used, False)
    hmm.initialize(pairhmm.PairHMMNativeArguments(False, 1))
    hmm.set_stripe_rows(32)
    try:
        host = hmm.compute_pairs(c.reads, c.read_off, c.haps, c.hap_off, c.pair_read, c.pair_hap)
        assert hmm.timing().rescued == int(used.sum())
        # a region: 60 reads x 40 haplotypes in the order the permuted list meets them
        rs = list(dict.fromkeys(c.pair_read.tolist()))[:60]
        hs = list(dict.fromkeys(c.pair_hap.tolist()))[:40]
        reads = [pairhmm.ReadDataHolder(*c.read(r)) for r in rs]
        haps = [pairhmm.HaplotypeDataHolder(c.hap(h)) for h in hs]
        jni = np.zeros(len(rs) * len(hs))
        hmm.computeLikelihoods(reads, haps, jni)
    finally:
        hmm.set_stripe_rows(0)
    assert (host == dev).all()
    # the same pairs in the same order through the device entry (compact() renumbers the pools, the pair order stays)
    region = pc.Case("region", c.reads, c.read_off, c.haps, c.hap_off, np.repeat(np.array(rs, np.int32), len(hs)),
                     np.tile(np.array(hs, np.int32), len(rs))).compact()
    dev_region, used_region = run(hmm, region, 32, False)
    check(region, dev_region, used_region, False)
    assert (jni == dev_region).all()
