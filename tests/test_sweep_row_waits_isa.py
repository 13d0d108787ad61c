"""What the row loops of the default scoring object wait for on vmcnt (WH_ROW_WAITS, wh_score7.hip): the compiled code, no GPU.

gfx950 counts vector-memory loads and stores on one counter.  A row of the stored Forward sweep must not wait on it at all
outside the block that issues the emission loads of a degenerate residue code - its own row stores stay in flight until the
sweep's closing wait - and a row of the envelope window sweep may wait on it only for the Forward cells it requested almost
a row earlier: at least 150 instructions after the nearest nt load of the loop (the parent's rows waited 23 to 33 instructions
after the request; the distance is tools/isa_loops.py's row_waits).  One -S compile with the Makefile's flags for the
default object; every register class of 8 to 24 cells per lane, both thread counts, the LDS instantiations.  No
instantiation keeps the parent's form."""
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
MIN_DISTANCE = 150


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


def test_stored_forward_rows_do_not_wait_on_vmcnt(asm):
    il = _isa_loops()
    bad = []
    for q in CELLS:
        for th in THREADS:
            loops = il.inner_loops(il.function_body(asm, "sweep_forwardILi%dELb1ELi%dELb0E" % (q, th)))
            members = max(loops.values(), key=lambda m: sum(len(i) for _, i in m))      # the row loop
            n, dist, fallback = il.row_waits(members)
            stores = sum(i.startswith("global_store") for _, ins in members for i in ins)
            print("sweep_forward<%d, true, %d, false>: row of %d instructions, %d row stores, %d fallback block(s), vmcnt waits outside: %d" % (q, th, n, stores, len(fallback), len(dist)))
            assert stores == 2 * (q // 4) and len(fallback) == 1, (q, th, stores, fallback)        # (it IS the storing row loop)
            if dist:
                bad.append((q, th, dist))
    assert not bad, bad


def test_window_rows_wait_for_their_request_a_row_later(asm):
    il = _isa_loops()
    bad = []
    for qb, cells in ((4, CELLS), (8, (16, 24))):
        for q in cells:
            for th in THREADS:
                loops = il.inner_loops(il.function_body(asm, "sweep_backward_null2_winILi%dELi%dELi%dELb0ELb0E" % (qb, q, th)))
                rows = [m for m in loops.values() if any(i.endswith(" nt") for _, ins in m for i in ins)]
                assert rows, (qb, q, th)
                for members in rows:
                    n, dist, fallback = il.row_waits(members)
                    print("sweep_backward_null2_win<%d, %d, %d, false>: loop of %d instructions, vmcnt waits %s instructions after the nearest nt load" % (qb, q, th, n, dist))
                    assert len(fallback) >= 1, (qb, q, th)
                    if any(d is None or d < MIN_DISTANCE for d in dist):
                        bad.append((qb, q, th, dist))
    assert not bad, bad
