"""scripts/lane_ck_waits.py on a hand-written listing: the two readings it is trusted for.  A wait at a loop's header whose count is
smaller than the stores issued behind the newest load (what pass 1's group loops had) is marked `<< STORE`, a counted one is not;
and a wait that stands between two sets of loads issued behind branches (what ck_block's byte-compare round loop had) is marked
`<< BETWEEN LOADS`."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
import lane_ck_waits as w  # noqa: E402


def _listing(header_wait, masked_wait):
    body = ["kernel_a:", ".LBB0_1:"]
    body += [f"\ts_waitcnt vmcnt({header_wait})", "\tv_mov_b32_e32 v1, v2"]
    body += ["\tglobal_load_dwordx4 v[4:7], v3, s[0:1]", "\tglobal_load_dword v8, v3, s[0:1]"]
    body += ["\tv_pk_add_u16 v9, v9, v10"] * 3
    # two sets of loads, each behind a branch
    body += ["\ts_cbranch_execz .LBB0_2", "\tglobal_load_dwordx4 v[12:15], v3, s[2:3]", ".LBB0_2:"]
    body += ["\ts_cbranch_execz .LBB0_3"]
    if masked_wait is not None:
        body += [f"\ts_waitcnt vmcnt({masked_wait})"]
    body += ["\tglobal_load_dwordx4 v[16:19], v3, s[2:3]", ".LBB0_3:"]
    body += ["\tglobal_store_dwordx4 v3, v[4:7], s[4:5]", "\tglobal_store_dwordx2 v3, v[8:9], s[4:5]"]
    body += ["\ts_cbranch_scc1 .LBB0_1", "\ts_endpgm"]
    return body


def _read(lines):
    out = []
    for name, lo, hi in w.kernels(lines):
        assert name == "kernel_a"
        for a, b in w.loops(lines, lo, hi):
            out += w.describe(lines, a, b, min_pk=2)
    return out


def test_a_header_wait_that_covers_the_trip_s_stores_is_marked():
    out = _read(_listing(0, None))
    assert "2 loads, 2 stores a trip" in out[0]
    waits = [ln for ln in out if "s_waitcnt" in ln]
    assert len(waits) == 1 and "<< STORE: waits for 2 store(s)" in waits[0]


def test_a_counted_header_wait_is_not():
    waits = [ln for ln in _read(_listing(2, None)) if "s_waitcnt" in ln]
    assert len(waits) == 1 and "<<" not in waits[0] and "global_load_dword at" in waits[0]


def test_a_wait_between_loads_behind_branches_is_marked():
    out = _read(_listing(2, 0))
    marked = [ln for ln in out if "BETWEEN LOADS" in ln]
    assert len(marked) == 1 and "(skipped)" in marked[0]
    assert sum("(skipped)" in ln and "global_load" in ln and "s_waitcnt" not in ln for ln in out) == 2
    assert not [ln for ln in _read(_listing(2, None)) if "BETWEEN LOADS" in ln]
