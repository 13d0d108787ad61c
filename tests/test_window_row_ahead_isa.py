"""What the row loops of the two node-window sweeps wait for on lgkmcnt (WH_ROW_AHEAD, wh_score7.hip): the compiled code, no GPU.

A window lane owns four cells, so a row is one dependent chain and an LDS round trip at its head is exposed in full.  The
parent's rows had two: the residue byte (ds_read_u8, waited for 2 instructions later) and the emission piece (ds_read_b128,
waited for 1 instruction later); the multihit window row also waited for lane 0's posterior writes at its back edge.  With
WH_ROW_AHEAD the byte is read two rows ahead and the piece one row ahead.  Asserted here, on the canonical path of each row loop
(tools/isa_loops.py's lds_waits: every block but the L2 fallback of a degenerate code):
(a) the lgkmcnt wait that is the first to cover a ds_read_u8 or a ds_read_b128 stands at least 64 instructions behind it.  At
    5 or more cycles of single-wave issue per instruction that is 320 cycles or more, over twice the unloaded return of a
    ds_read_b128;
(b) the multihit window loop has no lgkmcnt wait between the posterior ds_write_b32 and the loop's closing branch;
(c) neither loop touches scratch.
One -S compile with the Makefile's flags for the default object; every register class of 8 to 24 cells per lane, both thread
counts, 256-node windows (QB = 4) and the 512-node windows of the 16- and 24-cell classes (QB = 8), the multihit sweep also in its
in-place form.  No instantiation keeps the parent's form."""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "witch_amd", "csrc")
CELLS = (8, 12, 16, 20, 24)
THREADS = (512, 768)
MIN_DISTANCE = 64
KEPT_BACK = {}      # (function, QB, Q, TH) -> reason: instantiations that keep the parent's rows.  None.


def _isa_loops():
    spec = importlib.util.spec_from_file_location("isa_loops", os.path.join(ROOT, "tools", "isa_loops.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _default_object_flags():
    """K7A_FLAGS of the Makefile: K7_FLAGS and the layout of the default object."""
    text = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^K7_FLAGS\s*\?=\s*(.*)$", text, re.M).group(1).split()
    layout = re.search(r"^K7_LAYOUT\s*\?=\s*(\d+)", text, re.M).group(1)
    assert re.search(r"^K7A_FLAGS\s*\?=\s*\$\(K7_FLAGS\) -DWH_SPEC_ROWS=\$\(K7_LAYOUT\)\s*$", text, re.M), "K7A_FLAGS changed: restate it here"
    assert re.search(r"^K7B_FLAGS\s*\?=.*-DWH_ROW_AHEAD=0\b", text, re.M), "the A/B slot must keep the parent's window rows"
    return flags + ["-DWH_SPEC_ROWS=" + layout]


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("isa") / "wh_score7.s")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
                       + _default_object_flags() + ["--cuda-device-only", "-S", os.path.join(CSRC, "wh_score7.hip"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(out).read().splitlines()


def _row_loop(il, asm, key):
    """The row loop of a window sweep: the innermost loop that reads a residue byte."""
    loops = il.inner_loops(il.function_body(asm, key), fine=True)
    rows = [m for m in loops.values() if any(i.startswith("ds_read_u8") for _, ins in m for i in ins)]
    rows = [m for m in rows if any(i.startswith("ds_read_b128") for _, ins in m for i in ins)]
    assert len(rows) == 1, (key, len(rows))
    return rows[0]


def _check(il, asm, name, key, qb, q, th, posterior_writes):
    members = _row_loop(il, asm, key)
    n, waits, fallback = il.lds_waits(members)
    assert len(fallback) >= 1, (name, qb, q, th)                     # (the L2 branch of a degenerate code is still there)
    row = [ins for label, insns in members if label not in fallback for ins in insns]
    covered = [(op, d) for _, _, _, done in waits for op, d in done if op in ("ds_read_u8", "ds_read_b128")]
    print("%s<%d, %d, %d>: row of %d instructions, %d lgkmcnt waits; first cover of the residue byte / emission piece after %s instructions"
          % (name, qb, q, th, n, len(waits), sorted(covered)))
    bad = []
    # every such read of the row is covered by some wait of the row (qb / 4 pieces and one byte)
    if sorted(op for op, _ in covered) != ["ds_read_b128"] * (qb // 4) + ["ds_read_u8"]:
        bad.append(("reads covered", covered))
    if any(d < MIN_DISTANCE for _, d in covered):
        bad.append(("(a)", covered))
    if posterior_writes:
        writes = [p for p, ins in enumerate(row) if ins.startswith("ds_write")]      # (in place, two of the three words share one write)
        assert 1 <= len(writes) <= 3, (name, qb, q, th, writes)
        late = [p for p, _, _, _ in waits if p > writes[0]]
        if late:
            bad.append(("(b)", late))
    scratch = [ins for _, insns in members for ins in insns if ins.startswith("scratch_")]
    if scratch:
        bad.append(("(c)", scratch[:4]))
    return bad


def test_multihit_window_rows(asm):
    il = _isa_loops()
    bad, seen = [], set()
    for qb, cells in ((4, CELLS), (8, (16, 24))):
        for q in cells:
            for th in THREADS:
                for inpl in (0, 1):              # (1: the posteriors overwrite rows E, B and N in place - the 20- and 24-cell classes)
                    key = "sweep_backward_decode_winILi%dELi%dELi%dELb%dELb0ELb0E" % (qb, q, th, inpl)
                    if ("decode", qb, q, th) in KEPT_BACK or not any(l.startswith("_Z") and key in l for l in asm):
                        continue
                    seen.add((qb, q, th))
                    bad += [(qb, q, th, inpl) + b for b in _check(il, asm, "sweep_backward_decode_win", key, qb, q, th, True)]
    assert seen >= {(4, q, th) for q in CELLS for th in THREADS}, seen      # (every class has its 256-node window)
    assert not bad, bad


def test_envelope_window_rows(asm):
    il = _isa_loops()
    bad = []
    for qb, cells in ((4, CELLS), (8, (16, 24))):
        for q in cells:
            for th in THREADS:
                if ("null2", qb, q, th) in KEPT_BACK:
                    continue
                key = "sweep_backward_null2_winILi%dELi%dELi%dELb0ELb0E" % (qb, q, th)
                bad += [(qb, q, th) + b for b in _check(il, asm, "sweep_backward_null2_win", key, qb, q, th, False)]
    assert not bad, bad
