#!/usr/bin/env python3
"""Time hmmsearch -A's alignment of the included hits (wh_hits_msa) against the domain stage it follows (wh_domains).

One model of the headline family (bench.py: dna_100k_x200) and headline-shaped queries from witch_amd.synth.  wh_score with
detail records once, then wh_domains and wh_hits_msa on its output, both timed with HIP events through wh_last_kernel_ms:
the domain stage = slot 5 (inside wh_hits_msa it is the same stage), the hit selection = slot 8 (mark, scan, place and slice
kernels with the host's one wait), the alignment assembly = slot 6; and by the wall clock.  Median of the repeats after a
warm-up pass.  --resources: the compiler's -Rpass-analysis=kernel-resource-usage remarks for wh_hits.hip, stored with the
times.  Writes one JSON file (default profiles/hits_msa_mi355x.json).  The numbers are recorded, nothing is asserted.

    python tools/bench_hits_msa.py [--out FILE] [--nq 20000] [--repeats 3] [--resources FILE]
"""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from witch_amd import synth                                    # noqa: E402
from witch_amd.ehmm import EHMM, pack_queries                   # noqa: E402

HEADLINE = ("dna", 20251205, 900, 1024, 0.03, 1e-4, 150)       # bench.py: WORKLOADS["dna_100k_x200"]


def kernel_resources(path):
    """{kernel: {"vgprs", "sgprs", "scratch_bytes_per_lane", "lds_bytes", "occupancy"}} from the compiler's remarks."""
    out, name = {}, None
    keys = {"VGPRs": "vgprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane", "LDS Size [bytes/block]": "lds_bytes",
            "Occupancy [waves/SIMD]": "occupancy"}
    for line in open(path):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            mm = re.search(r"\d+(hits_\w+_kernel)", m.group(1))
            name = mm.group(1) if mm else m.group(1)
            out[name] = {}
            continue
        for k, v in keys.items():
            m = re.search(r"\s" + re.escape(k) + r": (\d+)", line)
            if m and name:
                out[name][v] = int(m.group(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hits_msa_mi355x.json"))
    ap.add_argument("--nq", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--resources", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_hits_msa.py needs a GPU: no figure is taken without one")
    alph, seed, root_len, leaves, sub, indel, qlen = HEADLINE
    fam = synth.make_family(seed, root_len, leaves, alph, sub, indel)
    with tempfile.TemporaryDirectory() as td:
        eh = synth.make_ehmm(fam, 1, td)
        _, seqs = synth.make_queries(fam, seed + 1, args.nq, qlen)
        e = EHMM(eh.paths, hmm_index=eh.index, nseq=eh.nseq)
    res, offs = pack_queries([s.astype(np.uint8) for s in seqs])
    text = "".join(synth.to_text(s.astype(np.int64), alph) for s in seqs)
    e.set_timing(True)
    deci, flags, det = e.score(res, offs, want_detail=True)
    nrep = int((flags & 1).sum())
    runs = []
    for r in range(args.repeats + 1):                            # the first pass loads the code objects: reported apart
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        recs, dom_off = e.domains(res, offs, flags, det)
        t1 = time.perf_counter()
        dom_ms = e.last_kernel_ms(5)[0]
        m = e.hits_msa(res, offs, text, flags, det, Z=args.nq, domZ=max(nrep, 1))
        t2 = time.perf_counter()
        runs.append({"wh_domains_stage_ms": dom_ms, "wh_domains_wall_ms": (t1 - t0) * 1e3,
                     "wh_hits_msa_wall_ms": (t2 - t1) * 1e3, "hits_msa_domain_stage_ms": e.last_kernel_ms(5)[0],
                     "hit_selection_ms": e.last_kernel_ms(8)[0], "hit_selection_launches": e.last_kernel_ms(8)[1],
                     "assembly_ms": e.last_kernel_ms(6)[0]})
        print(json.dumps(runs[-1]), flush=True)
    e.close()
    timed = runs[1:]
    med = {k: statistics.median(r[k] for r in timed) for k in timed[0]}
    out = {"tool": "tools/bench_hits_msa.py", "device": torch.cuda.get_device_name(0), "queries": args.nq, "models": 1,
           "model_nodes": int(e.M[0]), "reported_pairs": nrep, "domains": int(len(recs)), "rows": int(len(m["row_recs"])),
           "alignment_width": int(m["W"]), "first_pass": runs[0], "runs": timed, "median": med,
           "hit_selection_share_of_domain_stage": med["hit_selection_ms"] / med["hits_msa_domain_stage_ms"] if med["hits_msa_domain_stage_ms"] else None,
           "kernel_resources": kernel_resources(args.resources) if args.resources else None}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
