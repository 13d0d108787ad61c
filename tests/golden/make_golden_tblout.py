#!/usr/bin/env python3
"""hmmsearch's per-sequence table (--tblout) per model, for wh_seq_expect / wh_seq_table and the shim's --tblout
(tests/tblout_common.py, tests/test_tblout_host.py, tests/test_tblout_gpu.py).

RUNS ONLY IN THE BUILD CONTAINER (needs /root/reference): the reference's bundled hmmsearch 3.1b2 on the CPU,

    hmmsearch --cpu 1 --max --noali -E 99999999 -o OUT --tblout T HMM QUERIES

on every model and every query of dna_hmmbuild, amino_hmmbuild, amino_multidomain and example_sub30, stored under
tests/golden/tblout/<case>.json.gz, per model:
  "rows"      every table line: its 18 columns (as printed, kept as strings), the description and the raw line
  "header" / "trailer"   the file's comment lines in front of and behind them (the trailer without the lines that name
                         the run: option settings, directory, date, the two files)
  "Z", "domZ" from the -o text's summary
and tests/golden/tblout/classes.json.gz: the same for the seeded models of tests/tblout_common.py (both alphabets; the node
counts at the class edges of the counting sweep), each on its own queries.  No model text is stored: "M", the seed, the
sha256 of the text the binary read, and the queries' names (the tests make both again from the seeds).
Only program output and these settings are stored.

Asserted here, because the tests rely on it: over the case files, clu > 0 on at least 20 rows, among them rows with
env == reg; ov > 0 on at least 10 rows; at least 10 rows with a fractional exp; at least 5 rows with rep < dom; and per file
the exp column of the float64 host replica (wh_seq_expect_host; the library must be built) under the rule of
tests/tblout_common.py with at most 2 % exempt rows, reg and clu equal on every row.
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
import numpy as np  # noqa: E402

from tests import tblout_common as tc  # noqa: E402
from tests.conftest import load_case  # noqa: E402
from tests.filters_common import digitize, pack  # noqa: E402

HMMSEARCH = "/root/reference/witch_msa/tools/magus/tools/hmmer/hmmsearch"
OUT = tc.GOLDEN_TBL


def run(hmm, fa, tmp):
    o, t = os.path.join(tmp, "o.txt"), os.path.join(tmp, "t.tbl")
    subprocess.run([HMMSEARCH, "--cpu", "1", "--max", "--noali", "-E", "99999999", "-o", o, "--tblout", t, hmm, fa], check=True,
                   stdout=subprocess.DEVNULL)
    text = open(o).read()
    Z = int(re.search(r"^Target sequences:\s+(\d+)", text, re.M).group(1))
    m = re.search(r"^Domain search space  \(domZ\):\s+(\d+)", text, re.M)
    header, rows, trailer = tc.parse_tblout(open(t).read())
    trailer = [x for x in trailer if not re.match(r"# (Date|Current dir|Option settings|Target file|Query file)", x)]
    return {"Z": Z, "domZ": int(m.group(1)) if m else 0, "header": header, "trailer": trailer, "rows": rows}


def check_host(fname, paths, res, off, model_rows):
    """model_rows: [(h, [(q, row)])].  The host replica against the rows: reg, clu equal, exp under the rule; the exempt count."""
    from witch_amd.ehmm import seq_expect_host
    H = len(paths)
    pairs, rows = [], []
    for h, lst in model_rows:
        for q, r in lst:
            pairs.append(q * H + h)
            rows.append(r)
    got = seq_expect_host(paths, res, off, np.asarray(pairs, dtype=np.int64))
    exempt = 0
    for g, r in zip(got, rows):
        assert (int(g["reg"]), int(g["clu"])) == (int(r["reg"]), int(r["clu"])), (fname, r["raw"], g)
        ok, ex = tc.exp_ok(float(g["exp"]), r["exp"])
        assert ok, (fname, r["raw"], g)
        exempt += ex
    assert exempt <= tc.EXEMPT_CAP * max(len(rows), 1), (fname, exempt, len(rows))
    return len(rows), exempt


def write(fname, obj):
    path = os.path.join(OUT, fname + ".json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(obj, separators=(",", ":")).encode())
    return os.path.getsize(path)


def main_cases(tmp, only):
    stats = {"clu": 0, "clu_env_eq_reg": 0, "ov": 0, "frac": 0, "rep_lt_dom": 0}
    for cname in tc.CASES:
        if only and cname not in only:
            continue
        case = load_case(cname)
        alph = {"dna": 0, "rna": 1, "amino": 2}.get(case.alphabet, case.alphabet)
        fa = os.path.join(tmp, "q.fa")
        with open(fa, "w") as f:
            for n, s in zip(case.qnames, case.qseqs):
                f.write(">%s\n%s\n" % (n, s))
        res, off = pack([digitize(alph, s.upper()) for s in case.qseqs])
        qi = {n: i for i, n in enumerate(case.qnames)}
        models, model_rows = [], []
        for h, (hf, hp) in enumerate(zip(case.hmm_files, case.hmm_paths)):
            rec = run(hp, fa, tmp)
            rec["hmm_file"] = hf
            models.append(rec)
            model_rows.append((h, [(qi[r["target"]], r) for r in rec["rows"]]))
            for r in rec["rows"]:
                stats["clu"] += int(r["clu"]) > 0
                stats["clu_env_eq_reg"] += int(r["clu"]) > 0 and r["env"] == r["reg"]
                stats["ov"] += int(r["ov"]) > 0
                stats["frac"] += not r["exp"].endswith(".0")
                stats["rep_lt_dom"] += int(r["rep"]) < int(r["dom"])
        n, exempt = check_host(cname, case.hmm_paths, res, off, model_rows)
        size = write(cname, {"case": cname, "queries": case.qnames, "models": models})
        print("%s: %d models x %d queries, %d rows, %d exempt exp fields, %d bytes" % (cname, len(models), len(case.qnames), n, exempt, size), flush=True)
    if not only:
        print("rows with clu > 0: %(clu)d (env == reg on %(clu_env_eq_reg)d), ov > 0: %(ov)d, fractional exp: %(frac)d, rep < dom: %(rep_lt_dom)d" % stats)
        assert stats["clu"] >= 20 and stats["clu_env_eq_reg"] >= 1 and stats["ov"] >= 10 and stats["frac"] >= 10 and stats["rep_lt_dom"] >= 5, stats


def main_classes(tmp):
    out = {"fixture": "classes", "nodes": tc.CLASS_NODES, "alphabets": {}}
    for alphabet in tc.CLASS_ALPHABETS:
        models = tc.class_models(alphabet)
        paths, res, off, pairs, names = tc.class_call(alphabet)
        H = len(models)
        recs, model_rows, q0 = [], [], 0
        for h, (M, path, digest, queries) in enumerate(models):
            fa = os.path.join(tmp, "c.fa")
            with open(fa, "w") as f:
                for n, s in queries:
                    f.write(">%s\n%s\n" % (n, tc.codes_text(alphabet, s)))
            rec = run(path, fa, tmp)
            rec.update({"M": M, "seed": 1000 + M, "sha256": digest, "queries": [n for n, _ in queries]})
            recs.append(rec)
            qi = {n: q0 + i for i, (n, _) in enumerate(queries)}
            model_rows.append((h, [(qi[r["target"]], r) for r in rec["rows"]]))
            q0 += len(queries)
        n, exempt = check_host("classes_" + alphabet, paths, res, off, model_rows)
        out["alphabets"][alphabet] = recs
        print("classes %s: %d models, %d rows, %d exempt exp fields" % (alphabet, H, n, exempt), flush=True)
    print("classes: %d bytes" % write("classes", out))


def main():
    os.makedirs(OUT, exist_ok=True)
    tmp = tempfile.mkdtemp(prefix="golden_tblout_")
    only = sys.argv[1:]
    if only != ["classes"]:
        main_cases(tmp, [x for x in only if x != "classes"])
    if not only or "classes" in only:
        main_classes(tmp)


if __name__ == "__main__":
    main()
