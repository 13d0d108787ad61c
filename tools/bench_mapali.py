#!/usr/bin/env python3
"""Time hmmalign --mapali (wh_msa_mapali): the mapping of the model's own alignment and the assembly against the alignment
launch they accompany.

A backbone of 10 000 rows as wide as the family bench.py builds for its headline workload (dna_100k_x200: the family's 1 024
aligned leaves, repeated), the model wh_hmmbuild makes of it (symfrac 0.5: the model whose MAP and CKSUM lines are this
alignment's), and 20 000 headline-shaped queries (150 nt).  One wh_msa_mapali call aligns the queries (wh_align_pp_dev), maps
the backbone's rows (count and map kernels) and assembles hmmalign's alignment of 30 000 rows; the parts are timed with HIP
events through wh_last_kernel_ms - slot 7 the mapping (with the host's one wait for the counts), slot 6 the assembly, slot 2
the alignment launches - and the whole call by the wall clock, after a warm-up pass, median of three.  The same queries
through wh_msa (no backbone) are timed beside it.  Writes one JSON file (default profiles/mapali_mi355x.json).

    python tools/bench_mapali.py [--out FILE] [--nq 20000] [--rows 10000] [--repeats 3]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from witch_amd import synth                                    # noqa: E402
from witch_amd.ehmm import EHMM, pack_queries                   # noqa: E402
from witch_amd.gcmm.hmmbuild import hmmbuild_text               # noqa: E402

HEADLINE = ("dna", 20251205, 900, 1024, 0.03, 1e-4, 150)       # bench.py: WORKLOADS["dna_100k_x200"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mapali_mi355x.json"))
    ap.add_argument("--nq", type=int, default=20000)
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_mapali.py needs a GPU: no figure is taken without one")
    alph, seed, root_len, leaves, sub, indel, qlen = HEADLINE
    fam = synth.make_family(seed, root_len, leaves, alph, sub, indel)
    sym = synth.symbols(alph)
    leaf_rows = ["".join(sym[x] if x >= 0 else "-" for x in row) for row in fam.msa]
    rows = [leaf_rows[i % len(leaf_rows)] for i in range(args.rows)]
    names = ["bb%05d" % i for i in range(args.rows)]
    t0 = time.perf_counter()
    text_hmm, M, _ = hmmbuild_text(rows, alph, "backbone", symfrac=0.5)
    build_s = time.perf_counter() - t0
    _, seqs = synth.make_queries(fam, seed + 1, args.nq, qlen)
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "backbone.hmm")
        with open(path, "w") as f:
            f.write(text_hmm)
        e = EHMM([path])
    seqs = [s.astype(np.uint8) for s in seqs]
    res, offs = pack_queries(seqs)
    text = "".join(synth.to_text(s.astype(np.int64), alph) for s in seqs)
    e.set_timing(True)
    runs, plain = [], []
    for r in range(args.repeats + 1):                            # the first pass loads the code objects: reported apart
        t0 = time.perf_counter()
        m = e.msa(res, offs, text, mapali=(names, rows))
        wall = (time.perf_counter() - t0) * 1e3
        map_ms, map_launches = e.last_kernel_ms(7)
        asm_ms, launches = e.last_kernel_ms(6)
        align_ms, align_launches = e.last_kernel_ms(2)
        runs.append({"mapping_ms": map_ms, "assembly_ms": asm_ms, "align_ms": align_ms, "call_wall_ms": wall, "mapping_launches": map_launches,
                     "assembly_launches": launches, "align_launches": align_launches})
        print(json.dumps(runs[-1]), flush=True)
        t0 = time.perf_counter()
        m0 = e.msa(res, offs, text)
        wall = (time.perf_counter() - t0) * 1e3
        plain.append({"assembly_ms": e.last_kernel_ms(6)[0], "align_ms": e.last_kernel_ms(2)[0], "call_wall_ms": wall})
    e.close()
    timed = runs[1:]
    med = {k: statistics.median(r[k] for r in timed) for k in ("mapping_ms", "assembly_ms", "align_ms", "call_wall_ms")}
    med_plain = {k: statistics.median(r[k] for r in plain[1:]) for k in ("assembly_ms", "align_ms", "call_wall_ms")}
    W, alen = int(m["W"]), len(rows[0])
    out = {"tool": "tools/bench_mapali.py", "device": torch.cuda.get_device_name(0), "queries": args.nq, "backbone_rows": args.rows,
           "backbone_columns": alen, "model_nodes": M, "hmmbuild_host_s": build_s, "residues": int(offs[-1]), "W": W, "W_without_backbone": int(m0["W"]),
           "alignment_bytes": (args.rows + 2 * args.nq) * W, "pathless": int(m["pathless"]),
           "first_pass": runs[0], "runs": timed, "median": med, "without_backbone": {"runs": plain[1:], "median": med_plain},
           "mapping_plus_assembly_over_align": (med["mapping_ms"] + med["assembly_ms"]) / med["align_ms"] if med["align_ms"] else None,
           "mapping_gb_per_s": 2 * args.rows * alen / med["mapping_ms"] / 1e6 if med["mapping_ms"] else None}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
