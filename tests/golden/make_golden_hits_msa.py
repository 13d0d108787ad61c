#!/usr/bin/env python3
"""hmmsearch -A: the bundled binary's alignment of all hits that satisfy the inclusion thresholds, for wh_hits_msa
(tests/hits_msa_reference.py, tests/test_hits_msa_host.py, tests/test_hits_msa_gpu.py).

RUNS ONLY IN THE BUILD CONTAINER (needs /root/reference): the reference's bundled hmmsearch,

    hmmsearch --cpu 1 --noali -E 99999999 --max -o OUT -A ALI [more] HMM QUERIES

for amino_hmmbuild models 0-3, dna_hmmbuild models 0-2 and amino_multidomain model 0 (the queries of the domains fixture).
Stored under tests/golden/hits_msa/<case>.json.gz, per model its "runs", each {"args", "queries", "desc", "sto", "trailer"}
(the -A file and the line behind "//" of the main output; "desc": the FASTA descriptions given):
  "a"        the case's queries
  "b"        the same without the chim* records; the second record carries a FASTA description
  "inc", "notextw", "none"   (first model only, the queries of "b") --incE 1e-10 --incdomE 1e-10; --notextw; thresholds of
             1e-200, which nothing satisfies
and "ref_mismatch" / "ref_mismatch_b": the row names of "a" / "b" on which the CPU reference
(tests/hits_msa_reference.reference) and the binary differ - a name only one of them has (an alignment that ends a residue
earlier or later), or a row whose residues or PP characters differ.  All of them are weak domains;
tests/test_hits_msa_host.py checks that.  Only program output and these settings are stored.
"""
import gzip
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import domains_reference as dr  # noqa: E402
from tests import hits_msa_reference as hr  # noqa: E402
from tests import msa_reference as mr  # noqa: E402
from tests.conftest import load_case  # noqa: E402

HMMSEARCH = "/root/reference/witch_msa/tools/magus/tools/hmmer/hmmsearch"
OUT = os.path.join(HERE, "hits_msa")
DESCRIPTION = "a record with a description of its own"


def run(hmm, names, seqs, desc, extra, tmp):
    fa, o, ali = os.path.join(tmp, "q.fa"), os.path.join(tmp, "o.txt"), os.path.join(tmp, "a.sto")
    with open(fa, "w") as f:
        for n, s in zip(names, seqs):
            f.write(">%s%s\n%s\n" % (n, " " + desc[n] if n in desc else "", s))
    subprocess.run([HMMSEARCH, "--cpu", "1", "--noali", "-E", "99999999", "--max", "-o", o, "-A", ali] + extra + [hmm, fa],
                   check=True, stdout=subprocess.DEVNULL)
    lines = open(o).read().splitlines()
    trailer = lines[lines.index("//") + 1].replace(ali, "ALI")
    return {"args": extra, "queries": names, "desc": desc, "sto": open(ali).read(), "trailer": trailer}


def mismatch(sto, ref_text):
    """Row names on which the two files differ: a name only one has, or a row whose match columns or insert residues differ."""
    out = []
    a, b = mr.parse_msa(sto), mr.parse_msa(ref_text)
    for n in sorted(set(a[0]) | set(b[0])):
        if n not in a[0] or n not in b[0]:
            out.append(n)
        elif (hr.match_and_inserts(a[0][n], a[3]) != hr.match_and_inserts(b[0][n], b[3]) or
              hr.match_and_inserts(a[1][n], a[3]) != hr.match_and_inserts(b[1][n], b[3])):
            out.append(n)
    return out


def main():
    tmp = tempfile.mkdtemp(prefix="golden_hits_")
    os.makedirs(OUT, exist_ok=True)
    for cname, hs in hr.MODELS.items():
        case = load_case(cname)
        nq = len(dr.load_fixture(cname)["queries"])
        names, seqs = case.qnames[:nq], case.qseqs[:nq]
        keep = [q for q in range(nq) if not names[q].startswith("chim")]
        kn, ks = [names[q] for q in keep], [seqs[q] for q in keep]
        desc = {kn[1]: DESCRIPTION}
        models = []
        for h in hs:
            hp = case.hmm_paths[h]
            runs = {"a": run(hp, names, seqs, {}, [], tmp), "b": run(hp, kn, ks, desc, [], tmp)}
            if h == hs[0]:
                runs["inc"] = run(hp, kn, ks, desc, ["--incE", "1e-10", "--incdomE", "1e-10"], tmp)
                runs["notextw"] = run(hp, kn, ks, desc, ["--notextw"], tmp)
                runs["none"] = run(hp, kn, ks, desc, ["--incE", "1e-200", "--incdomE", "1e-200"], tmp)
            ref_a = hr.reference(cname, h)[0]
            ref_b, mb, _ = hr.reference(cname, h, keep=keep, descriptions=desc)
            mm = mismatch(runs["a"]["sto"], ref_a)
            whole = ref_b == runs["b"]["sto"]
            cons_b = mr.parse_msa(runs["b"]["sto"])[2]
            ties = hr.tie_columns(mb["W"] and len(mb["matmap"]), mb["cols"], mb["pps"])
            ncons = sum(1 for x, y in zip(cons_b, mb["pp_cons"].tobytes().decode()) if x != y) if len(cons_b) == mb["W"] else -1
            print("%s model %d: a %d rows, mismatch %s; b %d rows, W %d, whole file equal: %s, PP_cons characters that differ: %d, tie columns %d" %
                  (cname, h, len(hr.parse_gs(runs["a"]["sto"])[0]), mm, len(mb["row_recs"]), mb["W"], whole, ncons, len(ties)))
            mm_b = mismatch(runs["b"]["sto"], ref_b)
            print("    b mismatch %s" % mm_b)
            models.append({"h": h, "hmm_file": case.hmm_files[h], "runs": runs, "ref_mismatch": mm, "ref_mismatch_b": mm_b})
        path = os.path.join(OUT, cname + ".json.gz")
        with gzip.GzipFile(path, "wb", mtime=0) as f:
            f.write(json.dumps({"case": cname, "queries": names, "models": models}, separators=(",", ":")).encode())
        print("%s: %d bytes" % (cname, os.path.getsize(path)))


if __name__ == "__main__":
    main()
