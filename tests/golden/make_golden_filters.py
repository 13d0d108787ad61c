#!/usr/bin/env python3
"""Stage outcomes of hmmsearch's acceleration pipeline (MSV -> bias -> Viterbi -> Forward) per (model, query), for the
filters of wh_filter / wh_score_filtered (tests/test_filters_host.py, tests/test_filters_gpu.py).

RUNS ONLY IN THE BUILD CONTAINER (needs /root/reference): the reference's bundled hmmsearch on ONE-SEQUENCE FASTA files,

    hmmsearch --cpu 1 --noali [--nobias] --F1 a --F2 b --F3 c HMM ONE.fasta

whose "Internal pipeline statistics summary" then says with 0 or 1 which of the four stages the pair passed.  Bisecting one
threshold with the others at 1.0 finds the smallest F at which the pair passes a stage: that F is the stage's P-value.
  T1  --nobias --F2 1 --F3 1, bisect --F1, "Passed MSV":  P_MSV
  Tb  (no --nobias) --F2 1 --F3 1, bisect --F1, "Passed bias":  max(P_MSV, P_bias)      [cases with "bias": true]
  T2  --nobias --F1 1 --F3 1, bisect --F2, "Passed Vit":  min(P_MSV, P_Vit)  (the Viterbi stage is skipped below F2)
  T3  --nobias --F1 1 --F2 1, bisect --F3, "Passed Fwd":  P_Fwd
The bisection runs on ln F over [-700, 0]; a bracket is [lo, hi] in ln F with "fails at lo, passes at hi" (hi = -700: passes
everywhere - the filter overflowed or P underflows; lo = 0 does not occur, every pair passes at F = 1).

Stored under tests/golden/filters/<case>.json.gz:
  "golden_case", "models"   the golden case whose model files are used, and which of them (positions)
  "queries"                 [name, sequence] - the case's own queries plus copies with degenerate residues (X / N and one
                            IUPAC pair code), or a seeded low-complexity set
  "thresholds"              {"default": [F1, F2, F3], "alt": [...]}
  per model: "mu_lambda" (the six STATS numbers as printed), "counts" {"default": [4], "alt": [4]} - the four "Passed"
             numbers of a run over ALL queries with --nobias, "counts_bias" the same without --nobias
  per model and query: "out" {"default": [4 x 0/1], "alt": [...]} (with --nobias), "T1", "T2", "T3" (and "Tb") brackets,
             "msv_int": round((usc + 3) scale) = xJ - tjb - base recovered from T1 by inverting the Gumbel (null where
             1 - P is below 1e-9 or the filter overflowed), "msv_resid": its distance from the integer,
             "bias_nats": filtersc - null1 from Tb where P_bias > P_MSV decides (else null)
Only program output and these settings are stored.
"""
import gzip
import json
import math
import os
import random
import re
import subprocess
import sys
import tempfile
from multiprocessing import Pool

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests.conftest import load_case  # noqa: E402

HMMSEARCH = "/root/reference/witch_msa/tools/magus/tools/hmmer/hmmsearch"
OUT = os.path.join(HERE, "filters")
DEFAULT = [0.02, 1e-3, 1e-5]
ALT = [0.3, 0.05, 1e-3]
LN_LO, ITER = -700.0, 40
LOG2 = 0.69314718055994529
MAX_SKIP = 0.01
PASSED = [r"Passed MSV filter:\s+(\d+)", r"Passed bias filter:\s+(\d+)", r"Passed Vit filter:\s+(\d+)", r"Passed Fwd filter:\s+(\d+)"]


def run(hmm, fa, F, nobias=True):
    cmd = [HMMSEARCH, "--cpu", "1", "--noali"] + (["--nobias"] if nobias else []) + \
          ["--F1", repr(F[0]), "--F2", repr(F[1]), "--F3", repr(F[2]), hmm, fa]
    text = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True).stdout
    return [int(re.search(p, text).group(1)) for p in PASSED]


def bisect(hmm, fa, which, stage, nobias=True):
    """[lo, hi] in ln F: the pair fails <stage> at exp(lo) and passes at exp(hi)."""
    def passes(lnF):
        F = [1.0, 1.0, 1.0]
        F[which] = math.exp(lnF)
        return run(hmm, fa, F, nobias)[stage] == 1
    if passes(LN_LO):
        return [LN_LO, LN_LO]
    lo, hi = LN_LO, 0.0
    for _ in range(ITER):
        mid = 0.5 * (lo + hi)
        if passes(mid):
            hi = mid
        else:
            lo = mid
    return [lo, hi]


def stats_of(hmm_path):
    ev = {}
    for line in open(hmm_path):
        w = line.split()
        if len(w) >= 5 and w[0] == "STATS" and w[1] == "LOCAL":
            ev[w[2]] = (float(w[3]), float(w[4]))
        if w and w[0] == "HMM":
            break
    return ev


def nullone(L):
    return L * math.log(L / (L + 1.0)) + math.log(1.0 / (L + 1.0))


def gumbel_inv(P, mu, lam):
    """score in bits with gumbel_surv(score) = P"""
    return mu - math.log(-math.log1p(-P)) / lam


def one_pair(job):
    hmm, seq, ev, want_bias = job
    L = len(seq)
    with tempfile.NamedTemporaryFile("w", suffix=".fa", delete=False) as f:
        f.write(">q\n%s\n" % seq)
        fa = f.name
    try:
        rec = {"out": {"default": run(hmm, fa, DEFAULT), "alt": run(hmm, fa, ALT)},
               "T1": bisect(hmm, fa, 0, 0), "T2": bisect(hmm, fa, 1, 2), "T3": bisect(hmm, fa, 2, 3)}
        mu, lam = ev["MSV"]
        scale = 3.0 / LOG2
        rec["msv_int"], rec["msv_resid"], rec["bias_nats"] = None, None, None
        P1 = math.exp(rec["T1"][1])
        if rec["T1"][1] > LN_LO and 1.0 - P1 > 1e-9:
            usc = gumbel_inv(P1, mu, lam) * LOG2 + nullone(L)
            v = (usc + 3.0) * scale
            rec["msv_int"], rec["msv_resid"] = int(round(v)), abs(v - round(v))
        if want_bias:
            rec["Tb"] = bisect(hmm, fa, 0, 1, nobias=False)
            Pb = math.exp(rec["Tb"][1])
            # the bias stage decides where its P is above the MSV stage's by more than the brackets
            if rec["msv_int"] is not None and rec["Tb"][0] > rec["T1"][1] and 1.0 - Pb > 1e-9:
                usc = rec["msv_int"] / scale - 3.0
                rec["bias_nats"] = usc - gumbel_inv(Pb, mu, lam) * LOG2 - nullone(L)
        return rec
    finally:
        os.unlink(fa)


def degenerate_copies(names, seqs, amino):
    """three of the case's queries with degenerate residues: every 7th an X / N, every 11th a pair code (B / R)"""
    any_c, pair_c = ("X", "B") if amino else ("N", "R")
    out = []
    for n, s in list(zip(names, seqs))[:3]:
        t = list(s)
        for i in range(3, len(t), 7):
            t[i] = any_c
        for i in range(5, len(t), 11):
            t[i] = pair_c
        out.append((n + "_degen", "".join(t)))
    return out


def low_complexity(n=300, seed=20240607):
    """seeded low-complexity protein sequences: 80 % of the residues from a short set, lengths 80 - 500"""
    rng = random.Random(seed)
    aa = "ACDEFGHIKLMNPQRSTVWY"
    out = []
    for i in range(n):
        L = rng.randint(80, 500)
        short = rng.sample(aa, rng.randint(2, 4))
        out.append(("lc%03d" % i, "".join(rng.choice(short) if rng.random() < 0.8 else rng.choice(aa) for _ in range(L))))
    return out


# fixture -> (golden case, model positions, queries: None = the case's own + degenerate copies, bias thresholds as well)
CASES = {
    "amino_hmmbuild": ("amino_hmmbuild", None, None, True),
    "dna_hmmbuild": ("dna_hmmbuild", None, None, False),
    "dna_synth": ("dna_synth", None, None, False),
    "amino_multidomain": ("amino_multidomain", [0, 1], None, False),
    "lowcomplexity": ("amino_hmmbuild", [0, 1], "lc", True),
}


def main():
    os.makedirs(OUT, exist_ok=True)
    tmp = tempfile.mkdtemp(prefix="golden_filters_")
    only = sys.argv[1:]
    for fname, (cname, mpos, qsrc, want_bias) in CASES.items():
        if only and fname not in only:
            continue
        case = load_case(cname)
        amino = case.alphabet in (2, "amino")
        if qsrc == "lc":
            queries = low_complexity()
        else:
            names, seqs = case.qnames[:50], case.qseqs[:50]
            queries = list(zip(names, seqs)) + degenerate_copies(names, seqs, amino)
        mpos = list(range(len(case.hmm_paths))) if mpos is None else mpos
        fa_all = os.path.join(tmp, fname + ".fa")
        with open(fa_all, "w") as f:
            for n, s in queries:
                f.write(">%s\n%s\n" % (n, s))
        models = []
        for m in mpos:
            hp = case.hmm_paths[m]
            ev = stats_of(hp)
            with Pool(8) as pool:
                pairs = pool.map(one_pair, [(hp, s, ev, want_bias) for _, s in queries], chunksize=1)
            rec = {"hmm_file": case.hmm_files[m], "position": m, "mu_lambda": ev,
                   "counts": {"default": run(hp, fa_all, DEFAULT), "alt": run(hp, fa_all, ALT)},
                   "counts_bias": {"default": run(hp, fa_all, DEFAULT, nobias=False), "alt": run(hp, fa_all, ALT, nobias=False)},
                   "pairs": pairs}
            # the per-pair runs and the whole-file run are the same pipeline
            for key in ("default", "alt"):
                assert [sum(p["out"][key][s] for p in pairs) for s in range(4)] == rec["counts"][key], (fname, m, key)
            # a pair whose threshold lies within its own bracket of the F in use cannot be tested: at most 1 % of a case
            for key, F in (("default", DEFAULT), ("alt", ALT)):
                near = sum(1 for p in pairs if any(p[t][0] <= math.log(F[i]) <= p[t][1] and p[t][1] > LN_LO for i, t in enumerate(("T1", "T2", "T3"))))
                assert near <= MAX_SKIP * len(pairs), (fname, m, key, near)
            models.append(rec)
            print("%s model %d: default %s alt %s bias-default %s" % (fname, m, rec["counts"]["default"], rec["counts"]["alt"], rec["counts_bias"]["default"]), flush=True)
        path = os.path.join(OUT, fname + ".json.gz")
        with gzip.GzipFile(path, "wb", mtime=0) as f:
            f.write(json.dumps({"fixture": fname, "golden_case": cname, "queries": [list(q) for q in queries],
                                "thresholds": {"default": DEFAULT, "alt": ALT}, "ln_lo": LN_LO, "models": models},
                               separators=(",", ":")).encode())
        print("%s: %d models x %d queries, %d bytes" % (fname, len(models), len(queries), os.path.getsize(path)), flush=True)


if __name__ == "__main__":
    main()
