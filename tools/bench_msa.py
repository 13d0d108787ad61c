#!/usr/bin/env python3
"""Time the multi-sequence alignment assembly (wh_msa) against the alignment launch it follows.

20 000 headline-shaped queries (150 nt) against ONE model of the eHMM bench.py builds for its headline workload (the
dna_100k_x200 family and query recipe).  One wh_msa call aligns them (wh_align_pp_dev) and assembles hmmalign's alignment
(wh_msa_dev); both parts are timed with HIP events through wh_last_kernel_ms - slot 2 the alignment launches, slot 6 the
assembly (widths, layout, render and PP_cons kernels, with the host's one wait for W between them) - after a warm-up pass,
median of three.  The yardstick is the cheapest rendering the host could do from the same columns: formats.stockholm_row
once per sequence (one row each, without the shared insert columns, the PP rows or PP_cons).  Writes one JSON file
(default profiles/msa_mi355x.json).

    python tools/bench_msa.py [--out FILE] [--nq 20000] [--nh 200] [--repeats 3]
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
from witch_amd.shim import formats                              # noqa: E402

HEADLINE = ("dna", 20251205, 900, 1024, 0.03, 1e-4, 150)       # bench.py: WORKLOADS["dna_100k_x200"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msa_mi355x.json"))
    ap.add_argument("--nq", type=int, default=20000)
    ap.add_argument("--nh", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_msa.py needs a GPU: no figure is taken without one")
    alph, seed, root_len, leaves, sub, indel, qlen = HEADLINE
    fam = synth.make_family(seed, root_len, leaves, alph, sub, indel)
    with tempfile.TemporaryDirectory() as td:
        eh = synth.make_ehmm(fam, args.nh, td)
        _, seqs = synth.make_queries(fam, seed + 1, args.nq, qlen)
        e = EHMM([eh.paths[0]])
    seqs = [s.astype(np.uint8) for s in seqs]
    res, offs = pack_queries(seqs)
    texts = [synth.to_text(s.astype(np.int64), alph) for s in seqs]
    text = "".join(texts)
    M = int(e.M[0])
    e.set_timing(True)
    runs = []
    for r in range(args.repeats + 1):                            # the first pass loads the code objects: reported apart
        t0 = time.perf_counter()
        m = e.msa(res, offs, text)
        wall = (time.perf_counter() - t0) * 1e3
        asm_ms, launches = e.last_kernel_ms(6)
        align_ms, align_launches = e.last_kernel_ms(2)
        runs.append({"assembly_ms": asm_ms, "align_ms": align_ms, "call_wall_ms": wall, "assembly_launches": launches,
                     "align_launches": align_launches})
        print(json.dumps(runs[-1]), flush=True)
    cols, co, pp = e.align(res, offs, np.arange(args.nq), np.zeros(args.nq, dtype=np.int32), want_pp=True)
    e.close()
    host = []
    for r in range(args.repeats):
        t0 = time.perf_counter()
        for q in range(args.nq):
            formats.stockholm_row(texts[q], cols[co[q]:co[q + 1]], M, flank_at_end=True)
        host.append((time.perf_counter() - t0) * 1e3)
    timed = runs[1:]
    med = {k: statistics.median(r[k] for r in timed) for k in ("assembly_ms", "align_ms", "call_wall_ms")}
    med["host_stockholm_row_ms"] = statistics.median(host)
    W = int(m["W"])
    out = {"tool": "tools/bench_msa.py", "device": torch.cuda.get_device_name(0), "queries": args.nq, "model_nodes": M,
           "residues": int(offs[-1]), "W": W, "alignment_bytes": 2 * args.nq * W, "pathless": int(m["pathless"]),
           "first_pass": runs[0], "runs": timed, "host_runs_ms": host, "median": med,
           "assembly_over_align": med["assembly_ms"] / med["align_ms"] if med["align_ms"] else None,
           "host_over_assembly": med["host_stockholm_row_ms"] / med["assembly_ms"] if med["assembly_ms"] else None,
           "assembly_gb_per_s": 2 * args.nq * W / med["assembly_ms"] / 1e6 if med["assembly_ms"] else None}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
