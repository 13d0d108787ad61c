"""Static resources of the phase-call scoring kernels (wh_score7.hip): the compiler's own report, no GPU.

The sweeps of a pair are non-inlined functions without spills; what the kernel body itself keeps in scratch is the
per-pair glue.  This pins it: for every score_kernel7<Q, TH, SG> instantiation the waves per SIMD the
register allocation admits must not fall below what the launch shape needs (3 at 768 threads, 2 at 512), and the
scratch bytes per lane must not exceed the cap stored here (the finished build's value, rounded up to 16 B)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "witch_amd", "csrc")

# (Q, threads, long-query mode): (cap B/lane, B/lane before the glue was moved to scalar registers)
CAPS = {
    (4, 512, True): (64, 64), (4, 512, False): (64, 64),
    (8, 512, True): (80, 192), (8, 512, False): (80, 144),
    (12, 512, True): (80, 240), (12, 512, False): (80, 256),
    (16, 512, True): (192, 448), (16, 512, False): (96, 336),
    (20, 512, True): (272, 528), (20, 512, False): (208, 464),
    (24, 512, True): (368, 624), (24, 512, False): (336, 592),
    (4, 768, True): (64, 272), (4, 768, False): (64, 208),
    (8, 768, True): (176, 432), (8, 768, False): (144, 416),
    (12, 768, True): (352, 608), (12, 768, False): (176, 432),
    (16, 768, True): (480, 736), (16, 768, False): (448, 696),
    (20, 768, True): (432, 676), (20, 768, False): (448, 700),
    (24, 768, True): (560, 788), (24, 768, False): (544, 792),
}


def _k7_flags():
    for line in open(os.path.join(CSRC, "Makefile")):
        m = re.match(r"K7_FLAGS\s*\?=\s*(.*)$", line)
        if m:
            return m.group(1).split()
    raise AssertionError("K7_FLAGS not found in the Makefile")


def test_scoring_kernel_scratch_and_occupancy():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
                       + _k7_flags() + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "wh_score7.hip"), "-o", os.devnull],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    seen, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: _ZN2wh2k713score_kernel7ILi(\d+)ELi(\d+)ELb([01])EEE", line)
        if m:
            cur = (int(m.group(1)), int(m.group(2)), m.group(3) == "1")
            seen[cur] = {}
            continue
        if "Function Name:" in line:
            cur = None
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and cur:
            seen[cur][m.group(1).split()[0]] = int(m.group(2))
    assert set(seen) == set(CAPS), sorted(set(seen) ^ set(CAPS))
    bad = []
    for key in sorted(CAPS):
        cap, before = CAPS[key]
        scratch, occ = seen[key]["ScratchSize"], seen[key]["Occupancy"]
        print("score_kernel7<%d, %d, %s>: scratch %d B/lane (cap %d, before %d), %d waves per SIMD" % (key + (scratch, cap, before, occ)))
        if scratch > cap or occ < (3 if key[1] == 768 else 2):
            bad.append((key, scratch, occ))
    assert not bad, bad
