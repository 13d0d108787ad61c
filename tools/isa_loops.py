#!/usr/bin/env python3
"""Per-loop instruction mix of one kernel in a hipcc -save-temps .s file.

usage: tools/isa_loops.py [--waits | --lds] FILE.s KERNEL_SUBSTRING
For every innermost loop (a label that a later branch jumps back to) prints its length and how many
scratch loads/stores, LDS reads, VALU, AGPR moves and s_waitcnt it holds - the quick check that a
sweep's row loop is free of register spills.

--waits: what the loops wait for on vmcnt, the one counter of vector-memory loads and stores.  Loops are taken from the
compiler's own block comments here ("Inner Loop Header" / "in Loop: Header="), so that blocks it placed behind the loop's
closing branch count too.  For every innermost loop: its instructions, the s_waitcnt that name vmcnt outside the block(s)
that issue plain (not nt) global loads - the L2 fallback of a degenerate residue code, which completes its own loads - and
for each of them the distance in instructions back to the nearest nt load of the loop (row_waits below).

--lds: the twin for lgkmcnt, the counter of LDS accesses, which return in order.  For every innermost loop: the s_waitcnt that
name lgkmcnt outside the fallback blocks, for each the distance in instructions back to the nearest LDS instruction before it
along the same canonical row (round the back edge where needed), and which LDS accesses each wait is the first to cover, with
the distance from their issue (lds_waits below).
"""
import re
import sys


def function_body(lines, key):
    """The lines of the first function whose mangled name holds <key>, its label line to .Lfunc_end."""
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and key in l and re.match(r"^\S+:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[start:end + 1]


def _is_insn(l):
    return l.startswith("\t") and not l.strip().startswith((";", "."))


def inner_loops(body, fine=False):
    """Innermost loops as the compiler's comments name them: {header label: [(label, [instruction, ...]), ...]}, the
    labelled blocks of each loop in an order in which the row executes them: the layout's order, a block placed out of line
    (behind the loop's closing branch) moved to where the loop's own control flow first reaches it.
    fine: the compiler's unlabelled blocks ("; %bb.N:", reached by falling through only) are blocks of their own, named "%bb.N":
    a fallback block that follows the loop's header without a label is then told from the header."""
    blocks, cur = [], None                     # (label, annotation, instructions), layout order
    for l in body:
        m = re.match(r"^(\.LBB\d+_\d+):(.*)$", l) or (fine and re.match(r"^; (%bb\.\d+):(.*)$", l))
        if m:
            cur = [m.group(1), m.group(2), []]
            blocks.append(cur)
        elif cur is not None:
            if _is_insn(l):
                cur[2].append(l.split(";")[0].strip())
            elif l.strip().startswith(";") and not cur[2]:
                cur[1] += " " + l.strip()      # (a header's annotation runs over several comment lines)
    loops = {}
    for label, note, _ in blocks:
        if "Inner Loop Header" in note:
            loops[label] = []
    for label, note, insns in blocks:
        m = re.search(r"in Loop: Header=(BB\d+_\d+)", note)
        hdr = label if label in loops else ".L" + m.group(1) if m else None
        if hdr in loops:
            loops[hdr].append((label, insns))
    for hdr, members in loops.items():
        loops[hdr] = _execution_order(hdr, members)
    return loops                               # (row_waits and lds_waits take the members of one loop)


def _execution_order(hdr, members):
    names = [m[0] for m in members]
    succ = {}
    for n, (label, insns) in enumerate(members):
        out = []
        for ins in insns:
            m = re.match(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", ins)
            if m and m.group(1) in names and m.group(1) != hdr:
                out.append(m.group(1))
        falls = not insns or not re.match(r"s_branch|s_setpc|s_endpgm", insns[-1])
        if falls and n + 1 < len(members) and names[n + 1] != hdr:
            out.append(names[n + 1])           # (members are in layout order; a gap between two of them ends in a branch)
        succ[label] = out
    npred = {n: 0 for n in names}
    for outs in succ.values():
        for t in set(outs):
            npred[t] += 1
    order, ready = [], [hdr]
    while ready:
        ready.sort(key=names.index)
        label = ready.pop(0)
        order.append(label)
        for t in set(succ[label]):
            npred[t] -= 1
            if npred[t] == 0:
                ready.append(t)
    order += [n for n in names if n not in order]      # (unreached by this simple walk: kept, at the end)
    by = dict(members)
    return [(n, by[n]) for n in order]


def row_waits(members):
    """(instructions of the loop without its fallback blocks, [distance of each vmcnt wait outside them], fallback blocks).
    A fallback block issues plain global loads (the emission row of a degenerate code from L2).  The distance of a wait is
    the number of instructions from the nearest nt load before it to the wait, along the row as _execution_order lists it
    (every other block counted as executed, the way a row's instruction count is quoted), round the loop's back edge if
    the load sits behind the wait; None if the loop has no nt load."""
    fallback = [label for label, insns in members if any(re.match(r"(global|buffer|flat)_load", i) and not i.endswith(" nt") for i in insns)]
    pos, loads, waits = 0, [], []
    for label, insns in members:
        if label in fallback:
            continue
        for ins in insns:
            if re.match(r"(global|buffer|flat)_load", ins) and ins.endswith(" nt"):
                loads.append(pos)
            if ins.startswith("s_waitcnt") and "vmcnt" in ins:
                waits.append(pos)
            pos += 1
    dist = [min((w - p) % pos for p in loads) if loads else None for w in waits]
    return pos, dist, fallback


def lds_waits(members):
    """(instructions of the loop without its fallback blocks, [(position, n, distance, covered)] for every s_waitcnt lgkmcnt(n)
    outside them, fallback blocks).  <distance>: instructions from the nearest LDS instruction before the wait to the wait, along
    the canonical row of row_waits, round the back edge if need be (None: the loop has no LDS instruction).  <covered>: the LDS
    accesses this wait is the first to cover, as (mnemonic, instructions since their issue).  LDS accesses return in order, so
    lgkmcnt(n) covers all but the n youngest; the row is walked twice and the second walk is reported, so that an access issued
    behind its wait is found round the back edge.  (A loop whose row also issues scalar loads would need lgkmcnt(0) for them:
    none of the sweeps' row loops does, and such a wait is simply reported with what it covers.)"""
    fallback = [label for label, insns in members if any(re.match(r"(global|buffer|flat)_load", i) and not i.endswith(" nt") for i in insns)]
    row = [ins for label, insns in members if label not in fallback for ins in insns]
    n_row = len(row)
    lds = [p for p, ins in enumerate(row) if ins.startswith("ds_")]
    out, queue = [], []
    for walk in range(2):
        for p, ins in enumerate(row):
            if ins.startswith("ds_"):
                queue.append((ins.split()[0], walk * n_row + p))
            m = re.match(r"s_waitcnt\b.*lgkmcnt\((\d+)\)", ins)
            if m:
                n = int(m.group(1))
                done = queue[:max(len(queue) - n, 0)]
                queue = queue[len(done):]
                if walk == 1:
                    dist = min(((p - q - 1) % n_row) + 1 for q in lds) if lds else None
                    out.append((p, n, dist, [(name, walk * n_row + p - at) for name, at in done]))
    return n_row, out, fallback


def main():
    args = [a for a in sys.argv[1:] if a not in ("--waits", "--lds")]
    path, key = args[0], args[1]
    lines = open(path).read().splitlines()
    body = function_body(lines, key)
    if "--lds" in sys.argv[1:]:
        for hdr, members in inner_loops(body, fine=True).items():
            n, waits, fallback = lds_waits(members)
            print("%s loop %s: n=%4d without %d fallback block(s); lgkmcnt waits outside them: %d" % (key, hdr, n, len(fallback), len(waits)))
            for p, cnt, dist, done in waits:
                print("    at %4d lgkmcnt(%d): %s instructions after the nearest LDS instruction; first to cover: %s"
                      % (p, cnt, dist, ", ".join("%s (+%d)" % d for d in done) or "nothing"))
        return
    if "--waits" in sys.argv[1:]:
        for hdr, members in inner_loops(body).items():
            n, dist, fallback = row_waits(members)
            print("%s loop %s: n=%4d without %d fallback block(s); vmcnt waits outside them: %d, instructions after the nearest nt load: %s"
                  % (key, hdr, n, len(fallback), len(dist), dist))
        return
    labels = {}
    for i, l in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            labels[m.group(1)] = i
    loops = []
    for i, l in enumerate(body):
        m = re.search(r"s_cbranch_\w+\s+(\.LBB\d+_\d+)|s_branch\s+(\.LBB\d+_\d+)", l)
        if m:
            t = m.group(1) or m.group(2)
            if t in labels and labels[t] < i:
                loops.append((labels[t], i))
    inner = [lp for lp in loops if not any(o != lp and lp[0] <= o[0] and o[1] <= lp[1] for o in loops)]
    print("%s: %d instructions, %d loops (%d innermost)" % (key, len(body), len(loops), len(inner)))
    for a, b in sorted(set(loops)):
        seg = [l.strip() for l in body[a:b + 1] if l.startswith("\t") and not l.strip().startswith((";", "."))]
        c = lambda pat: sum(1 for l in seg if re.match(pat, l))
        tag = "inner" if (a, b) in inner else "outer"
        print("  %-5s lines %5d-%5d  n=%5d  scratch_ld=%3d scratch_st=%3d ds_read=%3d ds_write=%2d global=%3d valu=%4d accvgpr=%3d waitcnt=%3d nop=%2d"
              % (tag, a, b, len(seg), c(r"scratch_load"), c(r"scratch_store"), c(r"ds_read|ds_load"), c(r"ds_write|ds_store"),
                 c(r"global_|buffer_|flat_"), c(r"v_(?!accvgpr)"), c(r"v_accvgpr"), c(r"s_waitcnt"), c(r"s_nop")))


if __name__ == "__main__":
    main()
