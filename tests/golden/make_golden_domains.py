#!/usr/bin/env python3
"""hmmsearch's per-domain results (its --domtblout file and the ">> name" domain tables of its -o text) per model, for
the domain records of wh_domains (tests/domains_reference.py, tests/test_domains_host.py, tests/test_domains.py).

RUNS ONLY IN THE BUILD CONTAINER (needs /root/reference): the reference's bundled hmmsearch with the command line of
make_golden.py (witch_msa/gcmm/algorithm.py:526-532 plus --domtblout),

    hmmsearch --cpu 1 --noali -E 99999999 --max -o OUT --domtblout D HMM QUERIES

on dna_hmmbuild (8 models x 50 queries), amino_hmmbuild (4 x 44: all its queries) and the first three models x first ten queries of
amino_multidomain.  Stored under tests/golden/domains/<case>.json.gz, per model:
  "lines"   every domtblout line: its 22 columns (numbers as printed, kept as strings) and the raw line
  "header" / "trailer"   the file's comment lines in front of and behind them
  "Z", "domZ"   from the -o text's summary ("Target sequences", "Domain search space (domZ)")
  "tables"  per sequence name the lines of its ">> name" section
Only program output and these settings are stored.
"""
import gzip
import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests.conftest import load_case  # noqa: E402

HMMSEARCH = "/root/reference/witch_msa/tools/magus/tools/hmmer/hmmsearch"
OUT = os.path.join(HERE, "domains")
CASES = {"dna_hmmbuild": (None, None), "amino_hmmbuild": (None, None), "amino_multidomain": (3, 10)}    # (models, queries) kept
COLUMNS = ["target", "tacc", "tlen", "query", "qacc", "qlen", "evalue", "score", "bias", "num", "of", "c_evalue", "i_evalue",
           "dom_score", "dom_bias", "hmm_from", "hmm_to", "ali_from", "ali_to", "env_from", "env_to", "acc"]


def parse_output(text):
    """(Z, domZ, {name: lines of its ">> name" section})."""
    Z = int(re.search(r"^Target sequences:\s+(\d+)", text, re.M).group(1))
    domZ = int(re.search(r"^Domain search space  \(domZ\):\s+(\d+)", text, re.M).group(1))
    tables, name = {}, None
    for line in text.splitlines():
        if line.startswith(">> "):
            name = line[3:].split()[0]
            tables[name] = [line]
        elif name is not None:
            if line.startswith("Internal pipeline statistics"):
                name = None
            else:
                tables[name].append(line)
    for k, v in tables.items():
        while v and not v[-1].strip():
            v.pop()
    return Z, domZ, tables


def main():
    tmp = tempfile.mkdtemp(prefix="golden_dom_")
    os.makedirs(OUT, exist_ok=True)
    for cname, (nh, nq) in CASES.items():
        case = load_case(cname)
        names, seqs = case.qnames[:nq], case.qseqs[:nq]
        fa = os.path.join(tmp, "q.fa")
        with open(fa, "w") as f:
            for n, s in zip(names, seqs):
                f.write(">%s\n%s\n" % (n, s))
        models, ndom = [], 0
        for hf, hp in list(zip(case.hmm_files, case.hmm_paths))[:nh]:
            o, d = os.path.join(tmp, "o.txt"), os.path.join(tmp, "d.tbl")
            subprocess.run([HMMSEARCH, "--cpu", "1", "--noali", "-E", "99999999", "--max", "-o", o, "--domtblout", d, hp, fa],
                           check=True, stdout=subprocess.DEVNULL)
            Z, domZ, tables = parse_output(open(o).read())
            header, trailer, lines = [], [], []
            for line in open(d).read().splitlines():
                if line.startswith("#"):
                    (trailer if lines else header).append(line)
                    continue
                w = line.split()
                rec = dict(zip(COLUMNS, w[:22]))
                rec["raw"] = line
                lines.append(rec)
            # (the trailer names the program, the files and the date of the run: kept out, the tests need its layout only)
            trailer = [t for t in trailer if not re.match(r"# (Date|Current dir|Option settings|Target file|Query file)", t)]
            models.append({"hmm_file": hf, "Z": Z, "domZ": domZ, "header": header, "trailer": trailer, "lines": lines,
                           "tables": tables})
            ndom += len(lines)
        path = os.path.join(OUT, cname + ".json.gz")
        with gzip.GzipFile(path, "wb", mtime=0) as f:
            f.write(json.dumps({"case": cname, "queries": names, "models": models}, separators=(",", ":")).encode())
        print("%s: %d models x %d queries, %d domain lines, %d bytes" % (cname, len(models), len(names), ndom, os.path.getsize(path)))


if __name__ == "__main__":
    main()
