"""wh_hmmbuild_batch on the host (device = -1): all models of an eHMM in one call, calibrated in one batch.

The batch builds every model exactly as wh_hmmbuild2 does and, with WH_BUILD_STATS, calibrates them with the host's
sweeps (witch_amd/csrc/wh_calibrate.h: the same functions the device kernel is compiled from), so every text must be
byte for byte hmmbuild_text's, and the three STATS LOCAL lines hmmbuild's own (the golden files').  No GPU and no HIP
call is involved.
"""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from witch_amd import _lib, synth
from witch_amd.gcmm import hmmbuild_text_batch          # noqa: F401  (the re-export is part of the interface)
from witch_amd.gcmm.hmmbuild import hmmbuild_text, hmmbuild_text_batch, build_ehmm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CASES = sorted(f[:-4] for f in os.listdir(os.path.join(GOLD, "hmmbuild_cases")) if f.endswith(".afa"))


def stats_lines(text):
    return [l.rstrip() for l in text.splitlines() if l.startswith("STATS")]


def case_rows(case):
    d = os.path.join(GOLD, "hmmbuild_cases")
    rows = [l.strip() for l in open(os.path.join(d, case + ".afa")) if not l.startswith(">")]
    gold = open(os.path.join(d, case + ".hmm")).read()
    mol = {"DNA": "dna", "RNA": "rna", "amino": "amino"}[[l.split()[1] for l in gold.splitlines() if l.startswith("ALPH")][0]]
    return rows, gold, mol


def cases_by_molecule():
    by = {}
    for case in CASES:
        rows, gold, mol = case_rows(case)
        by.setdefault(mol, []).append((case, rows, gold))
    return by


def family_rows(alphabet, seed, root_len, n_leaves, n_sub, sub_rate, indel_rate):
    """The alignments tests/golden/make_golden.py::family_case handed to hmmbuild (seeded, reproducible)."""
    import numpy as np
    fam = synth.make_family(seed, root_len, n_leaves, alphabet, sub_rate, indel_rate)
    sym = synth.symbols(alphabet) + "-"
    rows = []
    for i in range(n_leaves):
        r = fam.msa[i].astype(np.int64).copy()
        r[r < 0] = len(sym) - 1
        rows.append("".join(sym[int(x)] for x in r))
    return rows, synth.bfs_subsets(n_leaves, n_sub)


def printed(sv):
    """out_stats as wh_build.cpp prints them: float32, %8.4f for the locations and %8.5f for lambda."""
    f32 = lambda v: C.c_float(v).value
    lam, mmu, vmu, tau = sv
    return ["STATS LOCAL MSV      %8.4f %8.5f" % (f32(mmu), f32(lam)),
            "STATS LOCAL VITERBI  %8.4f %8.5f" % (f32(vmu), f32(lam)),
            "STATS LOCAL FORWARD  %8.4f %8.5f" % (f32(tau), f32(lam))]


def test_batch_texts_and_stats_values():
    """The 20 golden cases, one batch per molecule, without flags and with WH_BUILD_STATS: byte for byte the texts of
    hmmbuild_text; with stats the three lines are the golden files', and out_stats printed as the builder prints them
    gives those lines."""
    by = cases_by_molecule()
    assert sum(len(v) for v in by.values()) == 20 and set(by) == {"dna", "rna", "amino"}
    for mol, items in by.items():
        names = [c for c, _, _ in items]
        lists = [r for _, r, _ in items]
        plain = hmmbuild_text_batch(lists, mol, names, device=-1)
        cal = hmmbuild_text_batch(lists, mol, names, stats=True, device=-1, want_stats_values=True)
        assert len(plain) == len(cal) == len(items)
        for (case, rows, gold), p, c in zip(items, plain, cal):
            assert p == hmmbuild_text(rows, mol, case), case
            assert c[:3] == hmmbuild_text(rows, mol, case, stats=True), case
            assert stats_lines(c[0]) == stats_lines(gold) and len(stats_lines(gold)) == 3, case
            assert printed(c[3]) == stats_lines(gold), (case, c[3])


def _raw_call(lists, n, device=-1, flags=0):
    L = _lib.lib()
    keep = [[r.encode() for r in rows] for rows in lists]
    arrs = [(C.c_char_p * len(rows))(*rows) for rows in keep]
    cnt = max(len(lists), 1)
    rows_pp = (C.POINTER(C.c_char_p) * cnt)(*[C.cast(a, C.POINTER(C.c_char_p)) for a in arrs])
    nseq = (C.c_int32 * cnt)(*[len(r) for r in keep])
    alen = (C.c_int64 * cnt)(*[len(r[0]) for r in keep])
    text = (C.c_void_p * cnt)(*([0xdead] * cnt))         # poisoned: the call must clear every entry
    tlen = (C.c_int64 * cnt)()
    rc = L.wh_hmmbuild_batch(device, b"dna", n, nseq, alen, rows_pp, None, 0.59, 0.0, 0.5, flags, text, tlen, None, None, None)
    return rc, text, tlen


def test_argument_handling():
    rc, _, _ = _raw_call([], 0)
    assert rc == _lib.WH_OK
    # a ragged alignment as model 1 of 3: refused, the message names the model, nothing is returned
    good = ["ACGTACGT", "ACGAACGT", "ACG-ACGT"]
    rc, text, tlen = _raw_call([good, ["ACGTACGT", "ACG"], good], 3)
    assert rc == _lib.WH_EINVAL
    msg = _lib.lib().wh_last_error().decode()
    assert "model 1" in msg and "row 1" in msg, msg
    assert all(text[i] is None for i in range(3)) and all(tlen[i] == 0 for i in range(3))
    # the same three, well-formed: three texts, each released by the caller
    rc, text, tlen = _raw_call([good, good[:2], good], 3)
    assert rc == _lib.WH_OK and all(text[i] for i in range(3))
    assert C.string_at(text[1], tlen[1]).decode() == hmmbuild_text(good[:2], "dna", "sub")[0]
    for i in range(3):
        _lib.lib().wh_free_text(text[i])
    with pytest.raises(ValueError):
        hmmbuild_text_batch([good, ["ACGT", "ACG"]], "dna", device=-1)
    with pytest.raises(ValueError):
        hmmbuild_text_batch([good], "protein", device=-1)


def test_build_ehmm_with_stats_on_the_host(tmp_path):
    """The dna_hmmbuild family (8 models of ~120 nodes): with stats=True the model files carry the golden STATS lines,
    everything else in them and the returned tuples are those of stats=False."""
    rows, subs = family_rows("dna", 11, 120, 32, 8, 0.04, 0.004)
    names = ["t%d" % i for i in range(len(rows))]
    subsets = [("A_0_%d" % i, list(range(lo, hi))) for i, (lo, hi) in enumerate(subs)]
    plain = build_ehmm(names, rows, subsets, "dna", str(tmp_path / "plain"))
    cal = build_ehmm(names, rows, subsets, "dna", str(tmp_path / "cal"), stats=True, device=-1)
    assert len(plain) == len(cal) == 8
    for idx, (p, c) in enumerate(zip(plain, cal)):
        assert p[1:] == c[1:] and os.path.relpath(p[0], tmp_path / "plain") == os.path.relpath(c[0], tmp_path / "cal")
        gold = open(os.path.join(GOLD, "dna_hmmbuild", "hmms", "A_0_%d.hmm" % idx)).read()
        tp, tc = open(p[0]).read(), open(c[0]).read()
        assert stats_lines(tc) == stats_lines(gold) and len(stats_lines(tc)) == 3 and not stats_lines(tp)
        assert [l for l in tc.splitlines() if not l.startswith("STATS")] == tp.splitlines()
        inp = os.path.join(os.path.dirname(c[0]), "hmmbuild.input.A_0_%d.fasta" % idx)
        assert open(inp).read() == open(os.path.join(os.path.dirname(p[0]), "hmmbuild.input.A_0_%d.fasta" % idx)).read()


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ on this machine")
def test_gpu_free_executable_still_builds_with_plain_gxx(tmp_path):
    """witch_amd/shim/bin/hmmbuild is wh_build.cpp + wh_calibrate.h under plain g++ (no HIP): it still builds after the
    sweeps became host/device functions, and still prints hmmbuild's lines."""
    shim = os.path.join(ROOT, "witch_amd", "shim")
    subprocess.run(["make", "-B", "-C", shim, "bin/hmmbuild", "CXX=g++"], check=True, stdout=subprocess.DEVNULL)
    exe = os.path.join(shim, "bin", "hmmbuild")
    case = "dna_fragments"
    out = tmp_path / "model.hmm"
    subprocess.run([str(exe), "--cpu", "1", "--dna", "--ere", "0.59", "--symfrac", "0.0", "--informat", "afa", "-o", "/dev/null", str(out),
                    os.path.join(GOLD, "hmmbuild_cases", case + ".afa")], check=True)
    gold = open(os.path.join(GOLD, "hmmbuild_cases", case + ".hmm")).read()
    skip = ("NAME", "DATE")
    assert [l for l in out.read_text().splitlines() if not l.startswith(skip)] == [l for l in gold.splitlines() if not l.startswith(skip)]
    assert len(stats_lines(out.read_text())) == 3
