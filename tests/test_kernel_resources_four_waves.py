"""Static resources of the four-waves-per-SIMD scoring object (wh_score7w.o: wh::k7w::score_kernel7<Q, 1024, false>): the
compiler's own report and the compiled row loops, no GPU.

The object is wh_score7.hip compiled with the default object's flags plus WH_K7W for workgroups of 1 024 threads, which leaves
a wave 128 vector registers.  Pinned here, for Q = 8, 12 and 16:
 - exactly these three kernels exist in the namespace, each at four waves per SIMD, its scratch per lane at most the cap stored
   here (the finished build's value rounded up to 16 B; the unchanged source, compiled for 1 024 threads, gave 564 B at Q = 16);
 - the row loops of the sweeps that run in volume - the two dense Forward sweeps, the in-place multihit window sweep and the
   envelope window sweep on 256 nodes - hold no scratch store and no more scratch loads than stored here: one (two in the storing
   sweep) per dense Forward row at Q = 16, a loop-invariant 64-bit value that the register allocator keeps in scratch and
   reloads once per row of 450 instructions; none anywhere else.  (The 512-node windows of the 16-cell class do spill at 128
   registers; they serve 0.4 % of the headline's envelopes and are left as they are: DESIGN.md section 9.12.)"""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "witch_amd", "csrc")
CELLS = (8, 12, 16)
SCRATCH_CAPS = {8: 288, 12: 304, 16: 576}          # B per lane; measured 288, 304, 564 (564 for the source before this object existed)
# (scratch loads, scratch stores) per row loop
ROW_LOOPS = {
    "sweep_forwardILi%dELb0ELi1024ELb0E": {8: (0, 0), 12: (0, 0), 16: (1, 0)},
    "sweep_forwardILi%dELb1ELi1024ELb0E": {8: (0, 0), 12: (0, 0), 16: (2, 0)},
    "sweep_backward_decode_winILi4ELi%dELi1024ELb1ELb0ELb0E": {8: (0, 0), 12: (0, 0), 16: (0, 0)},
    "sweep_backward_null2_winILi4ELi%dELi1024ELb0ELb0E": {8: (0, 0), 12: (0, 0), 16: (0, 0)},
}


def _isa_loops():
    spec = importlib.util.spec_from_file_location("isa_loops", os.path.join(ROOT, "tools", "isa_loops.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _object_flags():
    """The flags of the Makefile's wh_score7w.o rule: K7A_FLAGS (K7_FLAGS and the default object's layout) and the object's own."""
    text = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^K7_FLAGS\s*\?=\s*(.*)$", text, re.M).group(1).split()
    layout = re.search(r"^K7_LAYOUT\s*\?=\s*(\d+)", text, re.M).group(1)
    assert re.search(r"^K7A_FLAGS\s*\?=\s*\$\(K7_FLAGS\) -DWH_SPEC_ROWS=\$\(K7_LAYOUT\)\s*$", text, re.M), "K7A_FLAGS changed: restate it here"
    rule = re.search(r"^wh_score7w\.o: wh_score7\.hip\n\t(.*)$", text, re.M).group(1)
    assert "$(K7A_FLAGS)" in rule, rule
    own = [w for w in rule.split() if w.startswith("-DWH_K7")]
    assert sorted(own) == ["-DWH_K7LAUNCH=launch_score7w", "-DWH_K7NS=k7w", "-DWH_K7W=1"], own
    return flags + ["-DWH_SPEC_ROWS=" + layout] + own


def _hipcc():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    return [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC] + _object_flags()


def test_kernels_scratch_and_occupancy():
    r = subprocess.run(_hipcc() + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "wh_score7.hip"), "-o", os.devnull],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    seen, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            k = re.match(r"_ZN2wh3k7w13score_kernel7ILi(\d+)ELi(\d+)ELb([01])EEE", m.group(1))
            assert k or "score_kernel7" not in m.group(1), m.group(1)      # no kernel of another namespace, no four-envelope kernel
            cur = (int(k.group(1)), int(k.group(2)), k.group(3) == "1") if k else None
            if cur:
                seen[cur] = {}
            continue
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs): (\d+)", line)
        if m and cur:
            seen[cur][m.group(1).split()[0]] = int(m.group(2))
    assert set(seen) == {(q, 1024, False) for q in CELLS}, sorted(seen)
    bad = []
    for q in CELLS:
        s = seen[(q, 1024, False)]
        print("k7w::score_kernel7<%d, 1024, false>: %d VGPRs, scratch %d B/lane (cap %d), %d waves per SIMD" % (q, s["VGPRs"], s["ScratchSize"], SCRATCH_CAPS[q], s["Occupancy"]))
        if s["Occupancy"] != 4 or s["ScratchSize"] > SCRATCH_CAPS[q]:
            bad.append((q, s))
    assert not bad, bad


def _row_loop(il, asm, key):
    body = il.function_body(asm, key)
    if "_win" in key:      # the innermost loop that reads a residue byte and an emission piece (tests/test_window_row_ahead_isa.py)
        rows = [m for m in il.inner_loops(body, fine=True).values()
                if any(i.startswith("ds_read_u8") for _, ins in m for i in ins) and any(i.startswith("ds_read_b128") for _, ins in m for i in ins)]
        assert len(rows) == 1, (key, len(rows))
        return rows[0]
    return max(il.inner_loops(body).values(), key=lambda m: sum(len(i) for _, i in m))      # (tests/test_sweep_row_waits_isa.py)


def test_row_loops_stay_out_of_scratch(tmp_path):
    il = _isa_loops()
    out = str(tmp_path / "wh_score7w.s")
    r = subprocess.run(_hipcc() + ["--cuda-device-only", "-S", os.path.join(CSRC, "wh_score7.hip"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = open(out).read().splitlines()
    bad = []
    for pattern, per_q in ROW_LOOPS.items():
        for q, (max_loads, max_stores) in per_q.items():
            ins = [i for _, block in _row_loop(il, asm, pattern % q) for i in block]
            loads = sum(i.startswith("scratch_load") for i in ins)
            stores = sum(i.startswith("scratch_store") for i in ins)
            valu = sum(bool(re.match(r"v_(?!accvgpr)", i)) for i in ins)
            reads = sum(bool(re.match(r"ds_read|ds_load", i)) for i in ins)
            print("%s: %d instructions / %d VALU / %d ds_read / %d scratch loads / %d scratch stores" % (pattern % q, len(ins), valu, reads, loads, stores))
            assert len(ins) > 150 and valu > 100, (pattern % q, len(ins))      # (it IS a row loop)
            if loads > max_loads or stores > max_stores:
                bad.append((pattern % q, loads, stores))
    assert not bad, bad
