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

classes_dna, classes_amino (tests/filters_classes_common.py): one seeded model per size class of wh_filter.hip, made here
as the tests make it - "models" hold M, the seed, the variant ("mu40": the MSV mu at -40) and the sha256 of the text the
binary read, their own "queries" and "pairs" (own queries first, then "shared_queries"); no model text is stored.  The
conditions the fixture must meet are asserted in main_classes.
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
import numpy as np  # noqa: E402

from tests.conftest import load_case  # noqa: E402
from tests.filters_common import msv_tjb  # noqa: E402
from tests.filters_classes_common import CLASSES, LIMIT_LENGTHS, LIMIT_MODEL, MU40, model_file, model_list, model_text, sha256  # noqa: E402
from witch_amd import synth  # noqa: E402

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


# ---- classes_dna, classes_amino: one seeded model per size class of wh_filter.hip (tests/filters_classes_common.py) -----------
SYMS = {"dna": "ACGT", "amino": "ACDEFGHIKLMNPQRSTVWY"}
DEGEN = {"dna": ("N", "R"), "amino": ("X", "B")}
# The MSV filter cannot overflow on the 5-node DNA model, whatever the query: a hit scores at most 5 nodes x 6 units, pays
# tbm = 12 and tjb(L) to enter and tec = 3 to go on, and overflows 65 - bias units above the base; over n tiled copies
# (L = 5 n) the best total stays below 30 units.  The generator asserts that the binary shows none there.
NO_MSV_OVERFLOW = {("dna", 5)}
# (length, substitution rate) of a model's fragments.  A protein residue scores about twice a DNA residue's bits, and the MSV
# filter overflows 65 units above its base: longer or cleaner protein fragments all overflow and resolve nothing
FRAGMENTS = {"dna": ((8, 0.0), (12, 0.1), (20, 0.2), (30, 0.3), (45, 0.4), (60, 0.5), (24, 0.0), (40, 0.15)),
             "amino": ((8, 0.0), (8, 0.25), (10, 0.2), (10, 0.4), (12, 0.3), (14, 0.4), (16, 0.5), (20, 0.5))}


def _text(alphabet, codes):
    return "".join(SYMS[alphabet][int(c)] for c in codes)


def _substitute(rng, s, rate, K):
    s = np.array(s, copy=True)
    mut = rng.random(len(s)) < rate
    s[mut] = rng.integers(0, K, size=int(mut.sum()))
    return s


def _window(rng, cons, n):
    """n residues of the consensus from a seeded start; a model shorter than n is tiled"""
    M = len(cons)
    if M >= n:
        a = int(rng.integers(0, M - n + 1))
        return cons[a:a + n].copy()
    return np.tile(cons, -(-n // M))[:n]


def model_queries(alphabet, M, h):
    """a model's own queries [name, text] from its consensus (seed 7000 + M)"""
    K = len(SYMS[alphabet])
    rng = np.random.default_rng(7000 + M)
    cons = np.argmax(h.mat[1:], axis=1)
    any_c, pair_c = DEGEN[alphabet]
    out = []
    # fragments of 8 - 60 residues at 0 - 50 % substitution: scores in the discriminating range
    for n, rate in FRAGMENTS[alphabet]:
        out.append(("frag%d_%d" % (n, int(100 * rate)), _text(alphabet, _substitute(rng, _window(rng, cons, n), rate, K))))
    # consensus copies with one residue deleted every 6 - 14: the Viterbi filter follows them, the MSV filter does not
    for step in (6, 8, 14):
        s = _window(rng, cons, min(max(M, 40), 240))
        keep = np.ones(len(s), bool)
        keep[step - 1::step] = False
        out.append(("del%d" % step, _text(alphabet, s[keep])))
    # a long exact copy overflows the MSV filter
    out.append(("exact", _text(alphabet, _window(rng, cons, min(max(M, 30), 400)))))
    # a fragment between unrelated flanks
    f = _substitute(rng, _window(rng, cons, 40), 0.1, K)
    out.append(("flank", _text(alphabet, np.concatenate([rng.integers(0, K, 20), f, rng.integers(0, K, 20)]))))
    # degenerate codes at the first and last positions
    t = _text(alphabet, _substitute(rng, _window(rng, cons, 30), 0.1, K))
    out.append(("ends_degen", any_c + t[1:-1] + pair_c))
    # lengths around the 64-residue fetch, from the model's own consensus
    for n in (63, 65, 128):
        out.append(("len%d" % n, _text(alphabet, _substitute(rng, _window(rng, cons, n), 0.25, K))))
    if M in MU40[alphabet]:
        # queries that no node scores well: residues whose best log-odds over the nodes is negative, else the 'any' code
        best = np.log(h.mat[1:] / synth.background(alphabet)[None, :]).max(axis=0)
        poor = [SYMS[alphabet][a] for a in np.argsort(best) if best[a] < -0.25][:3] or [any_c]
        for i, n in enumerate((1, 2, 4, 7)):
            out.append(("poor%d" % n, "".join(poor[(i + j) % len(poor)] for j in range(n))))
    return [list(q) for q in out]


def limit_queries(alphabet):
    """runs of the 'any' code so long that the MSV filter's tjb + tbm + tec + bias passes 127 between the two lengths"""
    return [["limit%d" % n, DEGEN[alphabet][0] * n] for n in LIMIT_LENGTHS]


def shared_queries(alphabet):
    """the queries every model of a fixture is run on: unrelated, low-complexity and degenerate ones at the lengths
    around the 64-residue fetch"""
    K = len(SYMS[alphabet])
    rng = np.random.default_rng(20240901 + K)
    any_c, pair_c = DEGEN[alphabet]
    out = [("rand%d" % n, _text(alphabet, rng.integers(0, K, n))) for n in (1, 2, 64, 127, 129)]
    for n, k in ((100, 1), (300, 2)):
        short = rng.choice(K, size=k, replace=False)
        out.append(("lowc%d" % n, _text(alphabet, [rng.choice(short) if rng.random() < 0.8 else rng.integers(0, K) for _ in range(n)])))
    t = list(_text(alphabet, rng.integers(0, K, 150)))
    for i in range(3, 150, 7):
        t[i] = any_c
    for i in range(5, 150, 11):
        t[i] = pair_c
    t[0], t[-1] = pair_c, any_c
    out.append(("rand150_degen", "".join(t)))
    return [list(q) for q in out]


def resolvable(br):
    return LN_LO < br[1] < -1e-6


def classes_setup(fname, tmp):
    """(alphabet, shared queries, [(model record without results, path, queries)])"""
    alphabet = CLASSES[fname]
    shared = shared_queries(alphabet)
    models = []
    for M, variant in model_list(alphabet):
        h, text = model_text(alphabet, M, variant)
        own = model_queries(alphabet, M, h) + (limit_queries(alphabet) if variant == "mu40" and M == LIMIT_MODEL.get(alphabet) else [])
        rec = {"M": M, "seed": 1000 + M, "variant": variant, "sha256": sha256(text), "queries": own}
        models.append((rec, model_file(alphabet, M, variant, text, tmp), own + shared))
    return alphabet, shared, models


def write_fasta(path, queries):
    with open(path, "w") as f:
        for n, s in queries:
            f.write(">%s\n%s\n" % (n, s))


def main_classes(fname, tmp):
    alphabet, shared, todo = classes_setup(fname, tmp)
    models, vit_only = [], 0
    fa_all = os.path.join(tmp, fname + ".fa")
    with Pool(8) as pool:      # one pool over every pair of the fixture
        flat = pool.map(one_pair, [(hp, s, stats_of(hp), False) for _, hp, queries in todo for _, s in queries], chunksize=1)
    for rec, hp, queries in todo:
        ev = stats_of(hp)
        pairs, flat = flat[:len(queries)], flat[len(queries):]
        write_fasta(fa_all, queries)
        rec.update({"mu_lambda": ev, "counts": {"default": run(hp, fa_all, DEFAULT), "alt": run(hp, fa_all, ALT)}, "pairs": pairs})
        M, tag = rec["M"], (fname, rec["M"], rec["variant"])
        for key in ("default", "alt"):
            assert [sum(p["out"][key][s] for p in pairs) for s in range(4)] == rec["counts"][key], (tag, key)
        msv_over = sum(1 for p in pairs if p["T1"][1] == LN_LO)
        vit_only += sum(1 for p in pairs if p["T2"][1] == LN_LO and p["T1"][1] > LN_LO)
        if M >= 5:
            n1 = sum(1 for p in pairs if resolvable(p["T1"]))
            n2 = sum(1 for p in pairs if resolvable(p["T2"]) and p["T2"][1] < p["T1"][0])
            n3 = sum(1 for p in pairs if resolvable(p["T3"]))
            print("%s M %d %s: resolvable T1 %d, T2 decided by Viterbi %d, T3 %d, MSV overflows %d" % (fname, M, rec["variant"], n1, n2, n3, msv_over), flush=True)
            # (with the MSV mu at -40 the MSV stage's P is the smaller one wherever both resolve: T2 repeats T1 there)
            assert n1 >= 6 and n3 >= 4 and (n2 >= 4 or rec["variant"] == "mu40"), (tag, n1, n2, n3)
            assert (msv_over == 0) if (alphabet, M) in NO_MSV_OVERFLOW else (msv_over >= 1), (tag, msv_over)
        if rec["variant"] == "mu40":
            poor = [p for (n, _), p in zip(queries, pairs) if n.startswith("poor")]
            assert sum(1 for p in poor if resolvable(p["T1"])) >= 3, (tag, [p["T1"] for p in poor])
        # the "limit" queries: at the first length the binary's integer is the empty diagonal's, -(2 tjb + tbm + tec); at the
        # second it lies below it - the pre-filter stood aside, and the MSV filter paid for a residue
        lim = [(len(s), p["msv_int"]) for (n, s), p in zip(queries, pairs) if n.startswith("limit")]
        if lim:
            empty = [-(2 * msv_tjb(L) + int(-round(3.0 / LOG2 * math.log(2.0 / (M * (M + 1.0))))) + 3) for L, _ in lim]
            print("%s M %d: limit queries %s, the empty diagonal %s" % (fname, M, lim, empty), flush=True)
            assert len(lim) == 2 and lim[0][1] == empty[0] and lim[1][1] < empty[1], (tag, lim, empty)
        models.append(rec)
    # a pair whose threshold lies within its own bracket of the F in use cannot be tested: at most 1 % of the fixture
    allp = [p for m in models for p in m["pairs"]]
    for key, F in (("default", DEFAULT), ("alt", ALT)):
        near = sum(1 for p in allp if any(p[t][0] <= math.log(F[i]) <= p[t][1] and p[t][1] > LN_LO for i, t in enumerate(("T1", "T2", "T3"))))
        assert near <= MAX_SKIP * len(allp), (fname, key, near)
    assert vit_only >= 1, (fname, "no Viterbi overflow without an MSV overflow")
    path = os.path.join(OUT, fname + ".json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps({"fixture": fname, "alphabet": alphabet, "shared_queries": shared, "thresholds": {"default": DEFAULT, "alt": ALT},
                            "ln_lo": LN_LO, "models": models}, separators=(",", ":")).encode())
    print("%s: %d models, %d pairs, %d Viterbi overflows without an MSV overflow, %d bytes" % (fname, len(models), len(allp), vit_only, os.path.getsize(path)), flush=True)


def main():
    os.makedirs(OUT, exist_ok=True)
    tmp = tempfile.mkdtemp(prefix="golden_filters_")
    only = sys.argv[1:]
    for fname in CLASSES:
        if not only or fname in only:
            main_classes(fname, tmp)
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
