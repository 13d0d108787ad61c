#!/usr/bin/env python3
"""A model beyond 16 384 nodes, recorded from HMMER itself (tests/test_long_model_golden.py).

RUNS ONLY IN THE BUILD CONTAINER (needs /root/reference): a seeded witch_amd.synth DNA family whose alignment has ~17 000
columns goes through the reference's bundled hmmbuild 3.1b2 with the reference's command line
(witch_msa/gcmm/algorithm.py:463-470); twelve seeded queries (fragments, fragments in random flanks, one query with two
copies of the family) through hmmsearch --max (algorithm.py:526-532) and hmmalign (aligner.py:98).  Stored under
tests/golden/long_model/: the seeds, the sha256 of hmmbuild's file without its NAME, DATE and STATS lines, the printed
scores, the match columns of every query residue (hmmalign's Stockholm output, RF line: -1 for an insert) and the
queries themselves.  The alignment is NOT stored: the tests regenerate it from the seed.
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests.refparse import evalHMMSearchOutput  # noqa: E402
from witch_amd import synth  # noqa: E402

HMMER = "/root/reference/witch_msa/tools/magus/tools/hmmer"
OUT = os.path.join(HERE, "long_model")
FAMILY = {"seed": 17017, "root_len": 17000, "n_leaves": 8, "alphabet": "dna", "sub_rate": 0.03, "indel_rate": 1e-4}
QUERY_SEED = 1717
SKIP = ("NAME", "DATE", "STATS")


def family_rows(p):
    """The alignment handed to hmmbuild (also tests/test_long_model_golden.py)."""
    fam = synth.make_family(p["seed"], p["root_len"], p["n_leaves"], p["alphabet"], p["sub_rate"], p["indel_rate"])
    sym = synth.symbols(p["alphabet"]) + "-"
    rows = []
    for i in range(p["n_leaves"]):
        r = fam.msa[i].astype(np.int64).copy()
        r[r < 0] = len(sym) - 1
        rows.append("".join(sym[int(x)] for x in r))
    return fam, rows


def body_sha256(text):
    return hashlib.sha256("".join(l + "\n" for l in text.splitlines() if not l.startswith(SKIP)).encode()).hexdigest()


def queries(fam):
    rng = np.random.default_rng(QUERY_SEED)
    bg = synth.background(fam.alphabet)
    K = len(bg)
    _, frag = synth.make_queries(fam, QUERY_SEED, 8, 150)
    _, longer = synth.make_queries(fam, QUERY_SEED + 1, 1, 400)
    _, mid = synth.make_queries(fam, QUERY_SEED + 2, 2, 200)
    seqs = list(frag[:6]) + [longer[0]]
    for m in mid:
        a = int(rng.integers(10, 90))
        seqs.append(np.concatenate([rng.choice(K, size=a, p=bg), m, rng.choice(K, size=100 - a, p=bg)]))
    seqs.append(np.concatenate([frag[6], rng.choice(K, size=80, p=bg), frag[7]]))         # two copies of the family
    seqs.append(rng.choice(K, size=200, p=bg))                                             # background only
    seqs.append(np.concatenate([rng.choice(K, size=60, p=bg), frag[0][:90]]))              # a short fragment at the end
    names = ["long_q%02d" % i for i in range(len(seqs))]
    return names, [synth.to_text(s.astype(np.int64), fam.alphabet) for s in seqs]


def hmmalign_cols(hmm, names, texts, tmp):
    q, o = os.path.join(tmp, "q.fa"), os.path.join(tmp, "o.sto")
    open(q, "w").write("".join(">%s\n%s\n" % (n, t) for n, t in zip(names, texts)))
    subprocess.run([HMMER + "/hmmalign", "-o", o, hmm, q], check=True, stdout=subprocess.DEVNULL)
    rows, rf = {}, ""
    for line in open(o):
        if line.startswith("#=GC RF"):
            rf += line.split()[2]
        elif line.strip() and not line.startswith(("#", "//")):
            n, s = line.split()
            rows[n] = rows.get(n, "") + s
    out = {}
    for n in names:
        cols, k = [], -1
        for c, r in zip(rows[n], rf):
            if r == "x":
                k += 1
            if c not in "-.":
                cols.append(k if r == "x" else -1)
        out[n] = cols
    return out


def main():
    os.makedirs(OUT, exist_ok=True)
    tmp = tempfile.mkdtemp(prefix="golden_long_")
    fam, rows = family_rows(FAMILY)
    afa, hmm = os.path.join(tmp, "long.afa"), os.path.join(tmp, "long.hmm")
    open(afa, "w").write("".join(">s%d\n%s\n" % (i, r) for i, r in enumerate(rows)))
    subprocess.run([HMMER + "/hmmbuild", "--cpu", "1", "--dna", "--ere", "0.59", "--symfrac", "0.0", "--informat", "afa",
                    "-o", "/dev/null", hmm, afa], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(hmm).read()
    M = int(next(l.split()[1] for l in text.splitlines() if l.startswith("LENG")))
    names, texts = queries(fam)
    synth.write_fasta(os.path.join(OUT, "queries.fasta"), names, texts, fam.alphabet)
    out = os.path.join(tmp, "s.out")
    subprocess.run([HMMER + "/hmmsearch", "--cpu", "1", "--noali", "-E", "99999999", "-o", out, "--max", hmm,
                    os.path.join(OUT, "queries.fasta")], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    scores = {q: sc for q, (ev, sc) in evalHMMSearchOutput(out).items()}
    cols = hmmalign_cols(hmm, names, texts, tmp)
    g = {"family": FAMILY, "query_seed": QUERY_SEED, "M": M, "hmmbuild_sha256": body_sha256(text),
         "hmmsearch_scores": scores, "hmmalign_cols": cols, "two_copy": [names[9]]}
    json.dump(g, open(os.path.join(OUT, "golden.json"), "w"), separators=(",", ":"))
    print("M %d, %d of %d queries reported, sha256 %s" % (M, len(scores), len(names), g["hmmbuild_sha256"]))


if __name__ == "__main__":
    main()
