#!/usr/bin/env python3
"""hmmsearch's alignment display: the bundled binary's "Domain annotation for each sequence (and alignments)" section, for
wh_domain_display (tests/display_reference.py, tests/test_display_host.py, tests/test_display_gpu.py).

RUNS ONLY IN THE BUILD CONTAINER (needs /root/reference): the reference's bundled hmmsearch,

    hmmsearch --cpu 1 --max -E 99999999 -o OUT [more] HMM QUERIES

for amino_hmmbuild models 0-3, dna_hmmbuild models 0-2 and amino_multidomain model 0 (the queries of the domains fixture).
Stored under tests/golden/display/<case>.json.gz, per model its "runs", each {"args", "section"} (the lines of the main
output from the section's title up to the pipeline summary):
  "default"                       no further option
  "notextw", "textw150", "domE"   (first model only) --notextw; --textw 150; --domE 1e-10
and "ref_mismatch": {run: [[sequence, domain number]]} - the domains on which the CPU reference
(tests/display_reference.case_section) and the binary differ in any line under the "== domain" header, or that only one of
them prints - with "weak": per such domain HMMER's acc (all of them must be below 0.95: DESIGN.md section 4.10;
tests/test_display_host.py checks that).  Only program output and these settings are stored.
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
from tests import display_reference as ref  # noqa: E402
from tests import domains_reference as dr  # noqa: E402
from tests.conftest import load_case  # noqa: E402

HMMSEARCH = "/root/reference/witch_msa/tools/magus/tools/hmmer/hmmsearch"
OUT = os.path.join(HERE, "display")
RUN_KW = {"default": {}, "notextw": {"textw": None}, "textw150": {"textw": 150}, "domE": {"domE": 1e-10}}


def run(hmm, names, seqs, extra, tmp):
    fa, o = os.path.join(tmp, "q.fa"), os.path.join(tmp, "o.txt")
    with open(fa, "w") as f:
        for n, s in zip(names, seqs):
            f.write(">%s\n%s\n" % (n, s))
    subprocess.run([HMMSEARCH, "--cpu", "1", "--max", "-E", "99999999", "-o", o] + extra + [hmm, fa], check=True, stdout=subprocess.DEVNULL)
    return {"args": extra, "section": ref.section(open(o).read())}


def main():
    tmp = tempfile.mkdtemp(prefix="golden_display_")
    os.makedirs(OUT, exist_ok=True)
    for cname, hs in ref.MODELS.items():
        case = load_case(cname)
        nq = len(dr.load_fixture(cname)["queries"])
        names, seqs = case.qnames[:nq], case.qseqs[:nq]
        models = []
        for h in hs:
            hp = case.hmm_paths[h]
            runs = {"default": run(hp, names, seqs, [], tmp)}
            if h == hs[0]:
                for k, extra in ref.EXTRA_RUNS.items():
                    runs[k] = run(hp, names, seqs, extra, tmp)
            mismatch, weak = {}, {}
            for k, r in runs.items():
                mine = ref.case_section(cname, h, **RUN_KW[k])
                mm = ref.differing_domains(mine, r["section"])
                _, parsed, _ = ref.parse_section(r["section"])
                _, pmine, _ = ref.parse_section(mine)
                accs = [parsed.get(n, {"acc": {}})["acc"].get(d) for n, d in mm]
                ndom = sum(len(v["domains"]) for v in parsed.values())
                heads = sum(1 for n, v in parsed.items() for d, ln in v["domains"].items()
                            if [n, d] not in mm and pmine[n]["domains"][d][0] != ln[0])
                print("%s model %d %s: %d domains displayed, reference differs on %s (HMMER acc %s); headers that differ elsewhere: %d; "
                      "title equal: %s" % (cname, h, k, ndom, mm, accs, heads, mine[0] == r["section"][0]))
                mismatch[k], weak[k] = mm, accs
            models.append({"h": h, "hmm_file": case.hmm_files[h], "runs": runs, "ref_mismatch": mismatch, "weak": weak})
        path = os.path.join(OUT, cname + ".json.gz")
        with gzip.GzipFile(path, "wb", mtime=0) as f:
            f.write(json.dumps({"case": cname, "queries": names, "models": models}, separators=(",", ":")).encode())
        print("%s: %d bytes" % (cname, os.path.getsize(path)))


if __name__ == "__main__":
    main()
