#!/usr/bin/env python3
"""hmmalign's output for FILES of several sequences (one alignment per model), for the alignment assembly of wh_msa
(tests/test_msa_host.py, tests/test_msa_gpu.py, tests/msa_reference.py).

RUNS ONLY IN THE BUILD CONTAINER (needs /root/reference): the reference's bundled `hmmalign [options] HMM FASTA`, four
calls per case - default Stockholm, --trim, --outformat Pfam, --outformat afa.  Stored under
tests/golden/msa/<case>.json.gz: {"hmm": model file below tests/golden, "names", "seqs", "out": {"sto", "trim", "pfam",
"afa"}}.  Cases:
  dna_synth      dna_synth/A_0_0 (156 nodes) with the case's 40 queries
  dna_planted    the same model; the column-wise consensus of those queries with runs of 1, 2, 3, 5 and 7 residues planted at
                 one node (both halves of the split rule), N and C flanks of 0 to 5 residues, and an insert right behind node
                 M - 1 next to a C flank
  amino          amino_hmmbuild/A_0_0 with the case's queries (degenerate residues among them)
  dna_65         dna_hmmbuild/A_0_0 with the case's 50 queries and 15 clipped copies: more than one wavefront of rows
  sub30_two      two queries on example_sub30/A_0_0 (1 211 nodes, 1 429 columns): eight Stockholm blocks, a wide N flank
"""
import gzip
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests.conftest import load_case  # noqa: E402

HMMALIGN = "/root/reference/witch_msa/tools/magus/tools/hmmer/hmmalign"
OUT = os.path.join(HERE, "msa")
OPTIONS = {"sto": [], "trim": ["--trim"], "pfam": ["--outformat", "Pfam"], "afa": ["--outformat", "afa"]}


def hmmalign(hmm, names, seqs, extra, tmp):
    fa = os.path.join(tmp, "in.fa")
    with open(fa, "w") as f:
        for n, s in zip(names, seqs):
            f.write(">%s\n%s\n" % (n, s))
    return subprocess.run([HMMALIGN] + extra + [hmm, fa], check=True, stdout=subprocess.PIPE, text=True).stdout


def dump(name, hmm_rel, names, seqs, tmp):
    hmm = os.path.join(HERE, hmm_rel)
    obj = {"hmm": hmm_rel, "names": names, "seqs": seqs, "out": {k: hmmalign(hmm, names, seqs, v, tmp) for k, v in OPTIONS.items()}}
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(obj, separators=(",", ":")).encode())
    print("%s: %d sequences, %d bytes" % (name, len(names), os.path.getsize(path)))
    return obj


def rows_of(sto):
    rows = {}
    for line in sto.splitlines():
        if line.strip() and not line.startswith(("#", "//")):
            n, s = line.split()
            rows[n] = rows.get(n, "") + s
    return rows


def gc_of(sto, tag):
    return "".join(line.split()[2] for line in sto.splitlines() if line.startswith("#=GC " + tag))


def consensus(sto):
    """The most frequent residue of every match column."""
    rf, rows = gc_of(sto, "RF"), list(rows_of(sto).values())
    out = []
    for c, r in enumerate(rf):
        if r == "x":
            col = [row[c] for row in rows if row[c] != "-"]
            out.append(max(sorted(set(col)), key=col.count) if col else "A")
    return "".join(out)


def main():
    tmp = tempfile.mkdtemp(prefix="golden_msa_")
    rng = np.random.default_rng(20240607)
    rnd = lambda n: "".join("ACGT"[i] for i in rng.integers(0, 4, size=n))      # noqa: E731
    syn = load_case("dna_synth")
    hmm_rel = "dna_synth/hmms/A_0_0.hmm"
    base = dump("dna_synth", hmm_rel, syn.qnames, syn.qseqs, tmp)
    cons = consensus(base["out"]["sto"])
    M = len(cons)
    names, seqs = [], []
    for n in (1, 2, 3, 5, 7, 0):                            # runs at one node
        names.append("run%d" % n)
        seqs.append(cons[:80] + rnd(n) + cons[80:])
    for a, b in ((0, 5), (5, 0), (1, 4), (3, 3), (2, 0), (0, 1), (4, 2), (5, 5)):     # flanks
        names.append("flank%d_%d" % (a, b))
        seqs.append(rnd(a) + cons + rnd(b))
    names.append("tail_insert")                           # an insert right behind node M - 1, next to a C flank
    seqs.append(cons[:M - 1] + rnd(3) + cons[M - 1:] + rnd(4))
    names.append("fragment")
    seqs.append(cons[30:120])
    obj = dump("dna_planted", hmm_rel, names, seqs, tmp)
    rf = gc_of(obj["out"]["sto"], "RF")
    blocks = [len(b) for b in rf.split("x")]
    print("dna_planted: insert blocks (node: width):", {k: w for k, w in enumerate(blocks) if w})
    am = load_case("amino_hmmbuild")
    dump("amino", "amino_hmmbuild/hmms/A_0_0.hmm", am.qnames, am.qseqs, tmp)
    dh = load_case("dna_hmmbuild")
    names, seqs = list(dh.qnames), list(dh.qseqs)
    for t in range(15):
        s = dh.qseqs[t]
        names.append("clip%02d" % t)
        seqs.append(s[t:len(s) - 2 * t])
    dump("dna_65", "dna_hmmbuild/hmms/A_0_0.hmm", names, seqs, tmp)
    sub = load_case("example_sub30")
    # (SB: an N flank of 146 residues; SDCG: 294 residues in match states.  Two of their 604 residues lie in the guard band of
    # tests/test_align_pp.py; the case's first two queries have 11 of 512 there, above the cap of 1 %)
    pick = [sub.qnames.index(n) for n in ("SB", "SDCG")]
    dump("sub30_two", "example_sub30/hmms/A_0_0.hmm", [sub.qnames[t] for t in pick], [sub.qseqs[t] for t in pick], tmp)


if __name__ == "__main__":
    main()
