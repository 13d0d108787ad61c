#!/usr/bin/env python3
"""hmmalign's complete Stockholm output (sequence, PP, PP_cons and RF lines) per pair, for the per-residue posterior
probabilities of wh_align_pp (tests/test_align_pp_host.py, tests/test_align_pp.py, tests/pp_reference.py).

RUNS ONLY IN THE BUILD CONTAINER (needs /root/reference): the reference's bundled `hmmalign -o OUT HMM QUERY`
(witch_msa/gcmm/aligner.py:98), one call per pair, on
  * dna_hmmbuild in full (50 queries x 8 models) and amino_hmmbuild in full (40 x 4), and
  * LONG: one seeded 1 900-node witch_amd.synth DNA model (the recipe of
    test_multihit_queries_on_a_long_model_align_like_hmmalign) with two fragment queries and two multi-copy queries that
    leave float32 range on the device.  The model and the queries are NOT stored: the tests regenerate them from the seeds
    kept in the fixture (tests/pp_reference.py: long_model / long_queries), and
  * WINDOW: two seeded 700-node models per alphabet with 36 fragment queries (pp_reference.window_case): the node-window path,
    which the golden models are too short for.
Stored under tests/golden/align_pp/<case>.json.gz: {"pairs": [{"q", "h", "sto"}]}.  The LONG fixture also keeps, per
query class, the share of residues on which hmmalign's own PP character differs from the float64 reference's
(tests/pp_reference.py), measured here on the CPU: the log-space pairs' cap in the GPU test derives from it.
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
from tests import pp_reference as ppr  # noqa: E402
from tests.conftest import load_case  # noqa: E402
from witch_amd import synth  # noqa: E402
from witch_amd.shim.formats import pp_char  # noqa: E402

HMMALIGN = "/root/reference/witch_msa/tools/magus/tools/hmmer/hmmalign"
OUT = os.path.join(HERE, "align_pp")
LONG = {"family": {"seed": 4242 + 1900, "root_len": 1900, "n_leaves": 16, "alphabet": "dna", "sub_rate": 0.03, "indel_rate": 1e-4},
        "n_subsets": 2, "model": 0,
        "fragments": {"seed": 23, "n": 2, "length": [150, 400]},
        # (seed, number drawn, which of them are kept): multi-copy queries as in the parity test, the shortest that the
        # device still redoes in log space
        "multicopy": {"seed": 17, "n": 4, "length": [2100, 4200], "flank_frac": 0.3, "keep": [1, 2]}}


def hmmalign_text(hmm, name, text, tmp):
    q, o = os.path.join(tmp, "q.fa"), os.path.join(tmp, "o.sto")
    with open(q, "w") as f:
        f.write(">%s\n%s\n" % (name, text))
    subprocess.run([HMMALIGN, "-o", o, hmm, q], check=True, stdout=subprocess.DEVNULL)
    with open(o) as f:
        return f.read()


def dump(name, obj):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(obj, separators=(",", ":")).encode())
    print("%s: %d pairs, %d bytes" % (name, len(obj["pairs"]), os.path.getsize(path)))


def main():
    tmp = tempfile.mkdtemp(prefix="golden_pp_")
    for cname in ("dna_hmmbuild", "amino_hmmbuild"):
        case = load_case(cname)
        pairs = []
        for q, (qn, qs) in enumerate(zip(case.qnames, case.qseqs)):
            for h, hp in enumerate(case.hmm_paths):
                pairs.append({"q": q, "h": h, "sto": hmmalign_text(hp, qn, qs, tmp)})
        dump(cname, {"pairs": pairs})
    # the node-window cases
    for alphabet in ("dna", "amino"):
        paths, names, seqs = ppr.window_case(alphabet, os.path.join(tmp, "window_" + alphabet))
        pairs = []
        for q, (n, sq) in enumerate(zip(names, seqs)):
            for h, hp in enumerate(paths):
                pairs.append({"q": q, "h": h, "sto": hmmalign_text(hp, n, synth.to_text(sq.astype(np.int64), alphabet), tmp)})
        dump("window_" + alphabet, {"pairs": pairs})
    # the long model
    from oracle import oracle as orc
    fam, hp = ppr.long_model(LONG, os.path.join(tmp, "long"))
    names, seqs, kinds = ppr.long_queries(LONG, fam)
    model = ppr.Model(orc.OracleHMM(hp))
    pairs, differ, total = [], {}, {}
    for q, (n, s, kind) in enumerate(zip(names, seqs, kinds)):
        sto = hmmalign_text(hp, n, synth.to_text(s.astype(np.int64), "dna"), tmp)
        _, row, pp, _, rf = ppr.parse_stockholm(sto)
        cols, digits = ppr.row_cols_digits(row, pp, rf)
        ref = ppr.path_posteriors(model, s, cols)
        nd = sum(1 for a, b in zip(digits, ref) if a != pp_char(b))
        differ[kind] = differ.get(kind, 0) + nd
        total[kind] = total.get(kind, 0) + len(s)
        pairs.append({"q": q, "h": 0, "sto": sto, "kind": kind, "L": len(s)})
        print("long %s (%s, %d residues): hmmalign's digit differs from the reference's on %d" % (n, kind, len(s), nd))
    dump("long_model", {"spec": LONG, "pairs": pairs,
                        "hmmalign_vs_reference_share": {k: differ[k] / total[k] for k in total}})


if __name__ == "__main__":
    main()
