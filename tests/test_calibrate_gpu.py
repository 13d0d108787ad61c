"""E-value calibration of a whole batch of models on the device (witch_amd/csrc/wh_calibrate.hip through
wh_hmmbuild_batch with WH_BUILD_STATS).

The kernel runs the host's own sweeps (wh_calibrate.h) with one lane per (model, random sequence): the two integer
filters and the contraction-free float64 Forward recurrence must give the host's values bit for bit, and hmmbuild's
printed digits wherever a golden file exists.  The reference is the host path, which the golden files pin - never the
kernel itself.

Sizes at which the device code takes another path, all covered below:
  * 1, 2, 3 nodes (the first / last node have no D-state / no outgoing transitions);
  * 7, 8, 9, 15, 16, 17 nodes: kCalibChunk = 8, the sweeps read row i-1 eight nodes at a time (whole chunks, then a tail);
  * 63 .. 129 nodes: wave-width neighbours (no code path depends on them; asked for by the issue);
  * amino 1 169 / 1 170 nodes: the last model whose filter tables fit the 64 KiB of LDS (56 (M+1) bytes), and the first
    that reads them from global memory; WH_BUILD_CALIB_NO_LDS forces the latter for every model;
  * the example backbone's 1 278 .. 2 574-node DNA models: up to 62 KB of LDS.
"""
import gzip
import os
import re

import numpy as np
import pytest

from witch_amd import _lib, synth
from witch_amd.gcmm.hmmbuild import hmmbuild_text, hmmbuild_text_batch, build_ehmm

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(f[:-4] for f in os.listdir(os.path.join(GOLD, "hmmbuild_cases")) if f.endswith(".afa"))
MIB = 1 << 20


def stats_lines(text):
    return [l.rstrip() for l in text.splitlines() if l.startswith("STATS")]


def no_stats(text):
    return "".join(l for l in text.splitlines(True) if not l.startswith("STATS"))


def read(path):
    return (gzip.open(path, "rt") if path.endswith(".gz") else open(path)).read()


def family_rows(alphabet, seed, root_len, n_leaves, n_sub, sub_rate, indel_rate):
    """The alignments tests/golden/make_golden.py::family_case handed to hmmbuild (seeded, reproducible)."""
    fam = synth.make_family(seed, root_len, n_leaves, alphabet, sub_rate, indel_rate)
    sym = synth.symbols(alphabet) + "-"
    rows = []
    for i in range(n_leaves):
        r = fam.msa[i].astype(np.int64).copy()
        r[r < 0] = len(sym) - 1
        rows.append("".join(sym[int(x)] for x in r))
    return rows, synth.bfs_subsets(n_leaves, n_sub)


def family_models(case, args):
    rows, subs = family_rows(*args)
    return [(rows[lo:hi], read(os.path.join(GOLD, case, "hmms", "A_0_%d.hmm" % idx))) for idx, (lo, hi) in enumerate(subs)]


DNA_FAMILY = ("dna_hmmbuild", ("dna", 11, 120, 32, 8, 0.04, 0.004))
AMINO_FAMILY = ("amino_hmmbuild", ("amino", 13, 90, 16, 4, 0.08, 0.004))


def example_models(which):
    rows = []
    with gzip.open(os.path.join(GOLD, "example_e2e", "backbone.fasta.gz"), "rt") as fh:
        for line in fh:
            line = line.strip()
            if line.startswith(">"):
                rows.append("")
            elif line:
                rows[-1] += line
    subs = synth.bfs_subsets(len(rows), 15)
    return [([r.upper() for r in rows[subs[i][0]:subs[i][1]]], read(os.path.join(GOLD, "example_e2e", "hmms", "A_0_%d.hmm.gz" % i)))
            for i in which]


def check_against_golden(models, mol):
    """One batch on the device: the STATS lines are the golden files', the rest of each text is the stats-free text."""
    out = hmmbuild_text_batch([rows for rows, _ in models], mol, stats=True, device=0)
    assert len(out) == len(models)
    for i, ((rows, gold), (text, M, _)) in enumerate(zip(models, out)):
        assert stats_lines(text) == stats_lines(gold) and len(stats_lines(gold)) == 3, (i, M, stats_lines(text), stats_lines(gold))
        assert no_stats(text) == hmmbuild_text(rows, mol, "sub")[0], (i, M)


def test_golden_digits_small_models():
    """All 20 hmmbuild_cases (13 .. 80 nodes; DNA, RNA, amino), one batch per molecule."""
    by = {}
    for case in CASES:
        d = os.path.join(GOLD, "hmmbuild_cases")
        rows = [l.strip() for l in open(os.path.join(d, case + ".afa")) if not l.startswith(">")]
        gold = read(os.path.join(d, case + ".hmm"))
        mol = {"DNA": "dna", "RNA": "rna", "amino": "amino"}[[l.split()[1] for l in gold.splitlines() if l.startswith("ALPH")][0]]
        by.setdefault(mol, []).append((rows, gold))
    assert sum(len(v) for v in by.values()) == 20 and set(by) == {"dna", "rna", "amino"}
    for mol, models in by.items():
        check_against_golden(models, mol)


def test_golden_digits_families():
    """The 8 dna_hmmbuild and the 4 amino_hmmbuild models."""
    dna, amino = family_models(*DNA_FAMILY), family_models(*AMINO_FAMILY)
    assert len(dna) == 8 and len(amino) == 4
    check_against_golden(dna, "dna")
    check_against_golden(amino, "amino")


def test_golden_digits_real_sizes():
    """All 15 example-backbone models (1 278 .. 2 574 nodes: filter tables of up to 62 KB in LDS) in one batch."""
    models = example_models(range(15))
    out = hmmbuild_text_batch([rows for rows, _ in models], "dna", stats=True, device=0)
    golds = [g for _, g in models]
    assert sorted(M for _, M, _ in out)[0] == 1278 and sorted(M for _, M, _ in out)[-1] == 2574
    for i, ((text, M, _), gold) in enumerate(zip(out, golds)):
        assert stats_lines(text) == stats_lines(gold) and len(stats_lines(gold)) == 3, (i, M, stats_lines(text), stats_lines(gold))


DNA_M = (1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129)
AMINO_M = (64, 65, 1169, 1170)


def synthetic(alphabet, M, seed):
    """Four related sequences of exactly M columns without gaps: an M-node model under --symfrac 0.0."""
    fam = synth.make_family(seed, M, 4, alphabet, 0.1, 0.0)
    sym = synth.symbols(alphabet)
    assert fam.msa.shape == (4, M) and (fam.msa >= 0).all()
    return ["".join(sym[int(x)] for x in fam.msa[i]) for i in range(4)]


def bits(sv):
    return np.asarray(sv, np.float64).view(np.uint64).tolist()


@pytest.mark.parametrize("alphabet,sizes", [("dna", DNA_M), ("amino", AMINO_M)])
def test_device_equals_host_where_no_golden_exists(alphabet, sizes):
    """lambda, MSV mu, Viterbi mu (integer sweeps, the host's fit) and tau (float64 multiplies and adds in the host's
    order, never fused) are bit-identical to the host path's."""
    lists = [synthetic(alphabet, M, 100 + M) for M in sizes]
    host = hmmbuild_text_batch(lists, alphabet, stats=True, device=-1, want_stats_values=True)
    dev = hmmbuild_text_batch(lists, alphabet, stats=True, device=0, want_stats_values=True)
    assert [h[1] for h in host] == list(sizes)
    for M, h, d in zip(sizes, host, dev):
        print(alphabet, M, "host", h[3], "device", d[3])
        assert bits(d[3]) == bits(h[3]), (alphabet, M, h[3], d[3])
        assert d[0] == h[0], (alphabet, M)


@pytest.fixture(scope="module")
def schedule_models():
    """The 8 DNA family models and 3 of the example models (1 278, 1 286 and 1 291 nodes), and their default run.  (The 4
    amino family models run beside them in their own batch: one call takes one molecule.)"""
    dna = [rows for rows, _ in family_models(*DNA_FAMILY)] + [rows for rows, _ in example_models((11, 7, 8))]
    amino = [rows for rows, _ in family_models(*AMINO_FAMILY)]
    ref = {"dna": hmmbuild_text_batch(dna, "dna", stats=True, device=0, want_stats_values=True),
           "amino": hmmbuild_text_batch(amino, "amino", stats=True, device=0, want_stats_values=True)}
    return {"dna": dna, "amino": amino}, ref


def rows_bytes(M):
    """The row workspace of one model (include/witch_hip.h: wh_hmmbuild_batch), without its tables."""
    return 200 * 62 * (M + 1)


def test_schedule_tables_from_global_memory(schedule_models):
    lists, ref = schedule_models
    for mol in ("dna", "amino"):
        out = hmmbuild_text_batch(lists[mol], mol, stats=True, device=0, want_stats_values=True, flags=_lib.WH_BUILD_CALIB_NO_LDS)
        assert [bits(o[3]) for o in out] == [bits(r[3]) for r in ref[mol]]
        assert [o[0] for o in out] == [r[0] for r in ref[mol]]


def test_schedule_several_groups(schedule_models, monkeypatch):
    """A budget that holds any one of the three large models but no two of them: at least three groups."""
    lists, ref = schedule_models
    Ms = [r[1] for r in ref["dna"]][-3:]
    assert sorted(Ms) == [1278, 1286, 1291]
    budget_mb = (rows_bytes(max(Ms)) + MIB - 1) // MIB + 2          # + 2 MiB: its tables (124 (M+1) bytes) and rounding
    assert 2 * rows_bytes(min(Ms)) > budget_mb * MIB
    monkeypatch.setenv("WH_CALIB_WS_MB", str(budget_mb))
    out = hmmbuild_text_batch(lists["dna"], "dna", stats=True, device=0, want_stats_values=True)
    assert [bits(o[3]) for o in out] == [bits(r[3]) for r in ref["dna"]]
    assert [o[0] for o in out] == [r[0] for r in ref["dna"]]


def test_budget_below_one_model_is_refused(schedule_models, monkeypatch):
    lists, ref = schedule_models
    monkeypatch.setenv("WH_CALIB_WS_MB", "8")                     # the 1 278-node model's rows alone are 15.9 MB
    with pytest.raises(_lib.WitchHipError) as ei:
        hmmbuild_text_batch(lists["dna"], "dna", stats=True, device=0)
    msg = str(ei.value)
    assert "(%d)" % _lib.WH_ENOMEM in msg and "model 8 (1278 nodes)" in msg, msg
    figures = [int(x) for x in re.findall(r"(\d+) bytes", msg)]
    assert figures[0] >= rows_bytes(1278) and (8 * MIB) in figures, msg
    # the small models alone fit the same budget
    out = hmmbuild_text_batch(lists["dna"][:4], "dna", stats=True, device=0, want_stats_values=True)
    assert [bits(o[3]) for o in out] == [bits(r[3]) for r in ref["dna"][:4]]


def test_build_ehmm_on_the_device_equals_the_host(tmp_path):
    rows, subs = family_rows(*DNA_FAMILY[1])
    names = ["t%d" % i for i in range(len(rows))]
    subsets = [("A_0_%d" % i, list(range(lo, hi))) for i, (lo, hi) in enumerate(subs)]
    host = build_ehmm(names, rows, subsets, "dna", str(tmp_path / "host"), stats=True, device=-1)
    dev = build_ehmm(names, rows, subsets, "dna", str(tmp_path / "dev"), stats=True)        # device=None: the current device
    assert [h[1:] for h in host] == [d[1:] for d in dev]
    for h, d in zip(host, dev):
        assert open(h[0]).read() == open(d[0]).read() and len(stats_lines(open(d[0]).read())) == 3
        assert sorted(os.listdir(os.path.dirname(h[0]))) == sorted(os.listdir(os.path.dirname(d[0])))
