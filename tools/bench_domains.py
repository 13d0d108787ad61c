#!/usr/bin/env python3
"""Time the domain stage (wh_domains) against the scoring stage it follows.

2 000 headline-shaped queries x 200 models from witch_amd.synth, built as bench.py builds its headline workload (the
dna_100k_x200 family and query recipe, fewer queries).  wh_score with detail records, then wh_domains on its output, both
timed with HIP events through wh_last_kernel_ms: scoring = slots 0 + 4 (kernels + resolver), the domain stage = slot 5 (from
the list kernel to the summary kernel, the read-back of the envelope lengths between them included), the alignment launches
inside it = slot 2.  What the stage adds around the alignment it wraps (list, gather and summary kernels, the host's prefix
sum) is the difference.  Writes one JSON file (default profiles/domains_mi355x.json).

    python tools/bench_domains.py [--out FILE] [--nq 2000] [--nh 200] [--repeats 3]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from witch_amd import synth                                    # noqa: E402
from witch_amd.ehmm import EHMM, pack_queries                   # noqa: E402

HEADLINE = ("dna", 20251205, 900, 1024, 0.03, 1e-4, 150)       # bench.py: WORKLOADS["dna_100k_x200"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "domains_mi355x.json"))
    ap.add_argument("--nq", type=int, default=2000)
    ap.add_argument("--nh", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--length-model", default="envelope", choices=("envelope", "sequence"),
                    help="the domain stage's length model (EHMM.set_domain_length_model)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_domains.py needs a GPU: no figure is taken without one")
    alph, seed, root_len, leaves, sub, indel, qlen = HEADLINE
    fam = synth.make_family(seed, root_len, leaves, alph, sub, indel)
    with tempfile.TemporaryDirectory() as td:
        eh = synth.make_ehmm(fam, args.nh, td)
        _, seqs = synth.make_queries(fam, seed + 1, args.nq, qlen)
        e = EHMM(eh.paths, hmm_index=eh.index, nseq=eh.nseq)
    res, offs = pack_queries([s.astype(np.uint8) for s in seqs])
    e.set_domain_length_model(args.length_model)
    e.set_timing(True)
    runs = []
    for r in range(args.repeats + 1):                            # the first pass loads the code objects: reported apart
        deci, flags, det = e.score(res, offs, want_detail=True)
        score_ms = e.last_kernel_ms(0)[0] + e.last_kernel_ms(4)[0]
        recs, dom_off = e.domains(res, offs, flags, det)
        stage_ms, launches = e.last_kernel_ms(5)
        align_ms, align_launches = e.last_kernel_ms(2)
        runs.append({"score_ms": score_ms, "domain_stage_ms": stage_ms, "align_ms": align_ms, "around_align_ms": stage_ms - align_ms,
                     "launches": launches, "align_launches": align_launches})
        print(json.dumps(runs[-1]), flush=True)
    paths = e.last_align_paths()
    e.close()
    timed = runs[1:]
    med = {k: statistics.median(r[k] for r in timed) for k in ("score_ms", "domain_stage_ms", "align_ms", "around_align_ms")}
    Ld = (recs["env_j"] - recs["env_i"] + 1)
    out = {"tool": "tools/bench_domains.py", "device": torch.cuda.get_device_name(0), "queries": args.nq, "models": args.nh,
           "pairs": int(args.nq * args.nh), "reported_pairs": int((flags & 1).sum()), "domains": int(len(recs)),
           "envelope_residues": int(Ld.sum()), "mean_envelope": float(Ld.mean()) if len(recs) else 0.0,
           "domains_with_a_path": int((recs["ali_i"] > 0).sum()), "align_paths": paths,
           "first_pass": runs[0], "runs": timed, "median": med,
           "domain_stage_share_of_scoring": med["domain_stage_ms"] / med["score_ms"] if med["score_ms"] else None,
           "around_align_share_of_stage": med["around_align_ms"] / med["domain_stage_ms"] if med["domain_stage_ms"] else None}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
