#!/usr/bin/env python3
"""Stage outcomes of hmmsearch's acceleration pipeline WITH the bias filter (no --nobias) per (model, query), for the bias
stage of wh_filter / wh_score_filtered (tests/test_filters_bias_host.py, tests/test_filters_bias_gpu.py).

RUNS ONLY IN THE BUILD CONTAINER (needs /root/reference), like make_golden_filters.py, whose runner, bisection and query
makers it uses.  Every bracket bisects one threshold with the other two at 1.0, over the same ln-F range and iteration count:
  T1   --nobias, bisect --F1, "Passed MSV":   P_MSV
  Tb   bisect --F1, "Passed bias":            max(P_MSV, P_bias)
  T2b  bisect --F2, "Passed Vit":             min(P_bias, P_Vit), both against the bias filter's score
  T3b  bisect --F3, "Passed Fwd":             P_Fwd against the bias filter's score

Stored under tests/golden/filters_bias/<case>.json.gz:
  "queries"      [name, sequence]
  "thresholds"   {"default": [F1, F2, F3], "alt": [...]}
  per model: "golden_case", "position" (whose model file it is), "hmm_text" (only where the file the binary read is not a
             golden case's: a model with its COMPO line removed), "mu_lambda", "counts" - the four "Passed" numbers of a
             run over ALL queries, "counts_nobias" the same with --nobias
  per model and query: "out" {"default": [4 x 0/1], "alt": [...]}, "T1", "Tb", "T2b", "T3b"
Only program output and these settings are stored.

classes_dna, classes_amino: the seeded models and the queries of make_golden_filters.py's fixtures of these names (one
model per size class of wh_filter.hip, tests/filters_classes_common.py), with the same records per pair.
"""
import gzip
import json
import math
import os
import random
import sys
import tempfile
from multiprocessing import Pool

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from tests.conftest import load_case  # noqa: E402
from make_golden_filters import ALT, DEFAULT, LN_LO, MAX_SKIP, bisect, classes_setup, degenerate_copies, low_complexity, run, stats_of, write_fasta  # noqa: E402
from tests.filters_classes_common import CLASSES  # noqa: E402

OUT = os.path.join(HERE, "filters_bias")


def one_pair(job):
    hmm, seq = job
    with tempfile.NamedTemporaryFile("w", suffix=".fa", delete=False) as f:
        f.write(">q\n%s\n" % seq)
        fa = f.name
    try:
        return {"out": {"default": run(hmm, fa, DEFAULT, nobias=False), "alt": run(hmm, fa, ALT, nobias=False)},
                "T1": bisect(hmm, fa, 0, 0), "Tb": bisect(hmm, fa, 0, 1, nobias=False),
                "T2b": bisect(hmm, fa, 1, 2, nobias=False), "T3b": bisect(hmm, fa, 2, 3, nobias=False)}
    finally:
        os.unlink(fa)


def dna_low_complexity(n=300, seed=20240608):
    """seeded low-complexity reads: 80 % of the residues from one or two letters, lengths 60 - 400"""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        L = rng.randint(60, 400)
        short = rng.sample("ACGT", rng.randint(1, 2))
        out.append(("dlc%03d" % i, "".join(rng.choice(short) if rng.random() < 0.8 else rng.choice("ACGT") for _ in range(L))))
    return out


def case_queries(cname):
    case = load_case(cname)
    names, seqs = case.qnames[:50], case.qseqs[:50]
    return list(zip(names, seqs)) + degenerate_copies(names, seqs, case.alphabet in (2, "amino"))


def dna_queries():
    q = dna_low_complexity()
    return q + degenerate_copies([n for n, _ in q], [s for _, s in q], False)


def strip_compo(path):
    return "".join(ln for ln in open(path) if not ln.split()[:1] == ["COMPO"])


# fixture -> (queries, [(golden case, model position, remove the COMPO line)], the two runs' counts must differ)
CASES = {
    "lowcomplexity": (low_complexity, [("amino_hmmbuild", 0, False), ("amino_hmmbuild", 1, False)], False),
    "amino_hmmbuild": (lambda: case_queries("amino_hmmbuild"), [("amino_hmmbuild", m, False) for m in range(4)], False),
    "dna_lowcomplexity": (dna_queries, [("dna_synth", 0, False), ("dna_synth", 1, False), ("dna_hmmbuild", 0, False), ("dna_hmmbuild", 1, False)], True),
    "nocompo": (lambda: low_complexity() + case_queries("amino_hmmbuild"), [("amino_hmmbuild", 0, True)], False),
}


def main_classes(fname, tmp):
    """classes_dna, classes_amino: the models and queries of make_golden_filters.py's fixtures of these names, with the
    bias filter on"""
    alphabet, shared, todo = classes_setup(fname, tmp)
    with Pool(8) as pool:
        flat = pool.map(one_pair, [(hp, s) for _, hp, queries in todo for _, s in queries], chunksize=1)
    models = []
    fa_all = os.path.join(tmp, fname + ".fa")
    for rec, hp, queries in todo:
        pairs, flat = flat[:len(queries)], flat[len(queries):]
        write_fasta(fa_all, queries)
        rec.update({"mu_lambda": stats_of(hp),
                    "counts": {"default": run(hp, fa_all, DEFAULT, nobias=False), "alt": run(hp, fa_all, ALT, nobias=False)},
                    "counts_nobias": {"default": run(hp, fa_all, DEFAULT), "alt": run(hp, fa_all, ALT)}, "pairs": pairs})
        for key in ("default", "alt"):
            assert [sum(p["out"][key][s] for p in pairs) for s in range(4)] == rec["counts"][key], (fname, rec["M"], rec["variant"], key)
        models.append(rec)
    allp = [p for m in models for p in m["pairs"]]
    for key, F in (("default", DEFAULT), ("alt", ALT)):
        near = sum(1 for p in allp if any(p[t][0] <= math.log(F[i]) <= p[t][1] and p[t][1] > LN_LO for i, t in enumerate(("Tb", "T2b", "T3b"))))
        assert near <= MAX_SKIP * len(allp), (fname, key, near)
    decided = sum(1 for p in allp if p["Tb"][0] > p["T1"][1])
    path = os.path.join(OUT, fname + ".json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps({"fixture": fname, "alphabet": alphabet, "shared_queries": shared, "thresholds": {"default": DEFAULT, "alt": ALT},
                            "ln_lo": LN_LO, "models": models}, separators=(",", ":")).encode())
    print("%s: %d models, %d pairs, the bias stage's P above the MSV stage's on %d, %d bytes" % (fname, len(models), len(allp), decided, os.path.getsize(path)), flush=True)


def main():
    os.makedirs(OUT, exist_ok=True)
    tmp = tempfile.mkdtemp(prefix="golden_filters_bias_")
    only = sys.argv[1:]
    for fname in CLASSES:
        if not only or fname in only:
            main_classes(fname, tmp)
    for fname, (qmake, mlist, must_differ) in CASES.items():
        if only and fname not in only:
            continue
        queries = qmake()
        fa_all = os.path.join(tmp, fname + ".fa")
        with open(fa_all, "w") as f:
            for n, s in queries:
                f.write(">%s\n%s\n" % (n, s))
        models = []
        for cname, m, nocompo in mlist:
            case = load_case(cname)
            hp = case.hmm_paths[m]
            rec = {"golden_case": cname, "position": m, "hmm_file": case.hmm_files[m]}
            if nocompo:
                rec["hmm_text"] = strip_compo(hp)
                assert "COMPO" not in rec["hmm_text"] and rec["hmm_text"] != open(hp).read()
                hp = os.path.join(tmp, "%s_%s_%d_nocompo.hmm" % (fname, cname, m))
                with open(hp, "w") as f:
                    f.write(rec["hmm_text"])
            with Pool(8) as pool:
                pairs = pool.map(one_pair, [(hp, s) for _, s in queries], chunksize=1)
            rec.update({"mu_lambda": stats_of(hp),
                        "counts": {"default": run(hp, fa_all, DEFAULT, nobias=False), "alt": run(hp, fa_all, ALT, nobias=False)},
                        "counts_nobias": {"default": run(hp, fa_all, DEFAULT), "alt": run(hp, fa_all, ALT)},
                        "pairs": pairs})
            for key in ("default", "alt"):
                assert [sum(p["out"][key][s] for p in pairs) for s in range(4)] == rec["counts"][key], (fname, cname, m, key)
                if must_differ:
                    assert rec["counts"][key] != rec["counts_nobias"][key], (fname, cname, m, key)
            for key, F in (("default", DEFAULT), ("alt", ALT)):
                near = sum(1 for p in pairs if any(p[t][0] <= math.log(F[i]) <= p[t][1] and p[t][1] > LN_LO for i, t in enumerate(("Tb", "T2b", "T3b"))))
                assert near <= MAX_SKIP * len(pairs), (fname, cname, m, key, near)
            models.append(rec)
            print("%s %s model %d: default %s alt %s; --nobias default %s alt %s" % (fname, cname, m, rec["counts"]["default"], rec["counts"]["alt"],
                                                                                   rec["counts_nobias"]["default"], rec["counts_nobias"]["alt"]), flush=True)
        path = os.path.join(OUT, fname + ".json.gz")
        with gzip.GzipFile(path, "wb", mtime=0) as f:
            f.write(json.dumps({"fixture": fname, "queries": [list(q) for q in queries], "thresholds": {"default": DEFAULT, "alt": ALT},
                                "ln_lo": LN_LO, "models": models}, separators=(",", ":")).encode())
        print("%s: %d models x %d queries, %d bytes" % (fname, len(models), len(queries), os.path.getsize(path)), flush=True)


if __name__ == "__main__":
    main()
