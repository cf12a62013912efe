"""The waits of the lane kernel's column loops, read from a `-S` build (no GPU):
  hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S -o lane_ck.s mgl_amd/csrc/sw_dp16_lane_ck.hip
  python scripts/lane_ck_waits.py lane_ck.s [kernel-name-substring]
Every kernel is cut into loops at its backward branches (a branch to a label that stands above it); the innermost loops with
more than 200 v_pk_* are the column loops of pass 1 and of ck_block.  For each of them: its instructions, v_pk_*, v_mov_b32 and
scratch accesses, then its loads, stores and vmcnt waits in program order.

A `vmcnt(N)` lets the N newest memory operations stay in flight and waits for every older one.  Beside each wait stands what it
leaves in flight and the newest operation it waits for, counted back along the loop's own back edge on the trip that takes no
block the body branches around (the checkpoint's stores every 32 columns: listed, marked `skipped`, not counted -- they are issued
in front of the trip's loads, so they stand behind no load).  A wait in a loop serves a load.  Where the newest operation it waits
for is a STORE with no load between it and the wait's window, the count is smaller than any load needs and the wave waits for that
store's acknowledgement: marked `<< STORE`.  The count goes back over this trip and the one before it, no further (a count that
reaches beyond two trips' operations shows no newest awaited operation).

The blocks the body branches around get a reading of their own: ck_block's round loop loads pair A's and pair B's kept-row groups
under the lanes' masks, each behind a branch.  A wait inside such a block that stands BETWEEN loads -- the memory operation in front
of it a load of a branched-around block, the one behind it a load of the wait's own block -- makes the second set of loads wait for
the first: marked `<< BETWEEN LOADS`.  A wait outside those blocks is counted a second time on the trip that takes EVERY block,
and where that changes the newest awaited operation it is shown in brackets: a `<< STORE` whose bracket names a load waits for the
store only in a wave none of whose lanes takes the block.  Blocks that the compiler lays out behind the loop's backward branch are
not read.  It reads waits, loads and stores only."""
import re
import sys

MEM = re.compile(r"^\s+((?:global|buffer|flat|scratch)_(?:load|store|atomic)\w*)")
VMCNT = re.compile(r"^\s+s_waitcnt\b.*vmcnt\((\d+)\)")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BRANCH = re.compile(r"^\s+s_c?branch\w*\s+(\.LBB\d+_\d+)")
FUNC = re.compile(r"^(\w+):")
INSN = re.compile(r"^\s+[a-z]\w+")


def kernels(lines):
    """(name, first line, last line) of every function of the listing"""
    out, name, start = [], None, 0
    for k, ln in enumerate(lines):
        m = FUNC.match(ln)
        if m:
            name, start = m.group(1), k
        elif ln.startswith("\ts_endpgm") and name:
            out.append((name, start, k))
            name = None
    return out


def loops(lines, lo, hi):
    """innermost (label line, branch line) spans of the function"""
    at, spans = {}, []
    for k in range(lo, hi + 1):
        m = LABEL.match(lines[k])
        if m:
            at[m.group(1)] = k
            continue
        m = BRANCH.match(lines[k])
        if m and m.group(1) in at:
            spans.append((at[m.group(1)], k))
    return [s for s in spans if not any(o != s and s[0] <= o[0] and o[1] <= s[1] for o in spans)]


def describe(lines, a, b, min_pk=200):
    span = lines[a:b + 1]
    if sum("v_pk_" in ln for ln in span) <= min_pk:
        return []
    labels = {LABEL.match(ln).group(1): k for k, ln in enumerate(span) if LABEL.match(ln)}
    regions = []  # (first line, line of the target) of every forward branch inside the loop: the lines it can skip
    for k, ln in enumerate(span):
        m = BRANCH.match(ln)
        if m and labels.get(m.group(1), -1) > k:
            regions.append((k + 1, labels[m.group(1)]))
    skipped = {k for a_, b_ in regions for k in range(a_, b_)}

    def region(k):  # the innermost such block that holds line k
        inside = [r for r in regions if r[0] <= k < r[1]]
        return min(inside, key=lambda r: r[1] - r[0]) if inside else None
    n = pk = mov = scr = 0
    events = []  # (instruction number, kind, text, skipped)
    for k, ln in enumerate(span):
        if not INSN.match(ln) or ln.lstrip().startswith("."):
            continue
        n += 1
        word = ln.split()[0]
        pk += word.startswith("v_pk_")
        mov += word == "v_mov_b32_e32" or word == "v_mov_b32"
        scr += word.startswith("scratch_")
        m = MEM.match(ln)
        if m:
            events.append((n, "store" if "_store" in word else "load", word, k in skipped, region(k)))
        elif VMCNT.match(ln):
            events.append((n, "wait", int(VMCNT.match(ln).group(1)), k in skipped, region(k)))
    ops = [e for e in events if e[1] != "wait" and not e[3]]
    out = [f"  loop at line {a + 1}: {n} instructions, {pk} v_pk_*, {mov} v_mov_b32, {scr} scratch accesses, "
           f"{sum(e[1] == 'load' for e in ops)} loads, {sum(e[1] == 'store' for e in ops)} stores a trip"]
    for x, e in enumerate(events):
        if e[1] != "wait":
            out.append(f"    {e[0]:5d}  {e[2]}{'  (skipped)' if e[3] else ''}")
            continue
        # the operations in front of the wait, newest first: this trip's, then the trip's before it
        before = [(o, "") for o in reversed(ops) if o[0] < e[0]] + [(o, " of the trip before") for o in reversed(ops) if o[0] > e[0]]
        flying, rest = before[:e[2]], before[e[2]:]
        note = f"leaves {sum(o[1] == 'load' for o, _ in flying)} loads + {sum(o[1] == 'store' for o, _ in flying)} stores in flight"
        if e[3]:
            note += " (skipped)"
            mem = [m for m in events if m[1] != "wait"]
            front = [m for m in mem if m[0] < e[0]][-1:]
            behind = [m for m in mem if m[0] > e[0]][:1]
            if front and behind and front[0][1] == "load" and front[0][3] and behind[0][1] == "load" and behind[0][4] == e[4]:
                note += f"  << BETWEEN LOADS: {behind[0][2]} at {behind[0][0]} waits for {front[0][2]} at {front[0][0]}"
        elif rest:
            # the same count on the trip that takes EVERY block (ck_block's masked loads stand in such blocks)
            every = [m for m in events if m[1] != "wait"]
            taken = ([m for m in reversed(every) if m[0] < e[0]] + [m for m in reversed(every) if m[0] > e[0]])[e[2]:e[2] + 1]
            o, trip = rest[0]
            note += f"; the newest it waits for: {o[2]} at {o[0]}{trip}"
            if o[1] == "store":
                extra = 0
                for p, _ in rest:
                    if p[1] == "load":
                        break
                    extra += 1
                note += f"  << STORE: waits for {extra} store(s) issued behind the newest load it can serve"
            if taken and taken[0] is not o:
                note += f"  [every block taken: {taken[0][2]} at {taken[0][0]}]"
        out.append(f"    {e[0]:5d}  s_waitcnt vmcnt({e[2]})  {note}")
    return out


def main():
    lines = open(sys.argv[1]).read().splitlines()
    pat = sys.argv[2] if len(sys.argv) > 2 else ""
    for name, lo, hi in kernels(lines):
        if pat not in name:
            continue
        print(name)
        for a, b in loops(lines, lo, hi):
            for ln in describe(lines, a, b):
                print(ln)


if __name__ == "__main__":
    main()
