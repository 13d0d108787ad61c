#!/usr/bin/env python3
"""Time the alignment display (wh_domain_display_dev) against the domain stage it follows.

2 000 headline-shaped queries x 200 models from witch_amd.synth, the workload of tools/bench_domains.py.  wh_score with detail
records, ONE wh_domain_paths_dev on its output, then wh_domain_display_dev for every model in turn (the stage renders one
model's domains per call, as hmmsearch works one model at a time), all timed with HIP events through wh_last_kernel_ms:
scoring = slots 0 + 4, the domain stage = slot 5, the alignment launches inside it = slot 2, the display = slot 9 summed over
the models (count, scan and render kernels with the host's wait between count and render; the read-back of the lines is not
in it).  Median of the passes after a warm-up.  Writes one JSON file (default profiles/display_mi355x.json).

    python tools/bench_display.py [--out FILE] [--nq 2000] [--nh 200] [--repeats 3]
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

from witch_amd import _lib, synth                              # noqa: E402
from witch_amd.ehmm import EHMM, pack_queries                   # noqa: E402

HEADLINE = ("dna", 20251205, 900, 1024, 0.03, 1e-4, 150)       # bench.py: WORKLOADS["dna_100k_x200"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "display_mi355x.json"))
    ap.add_argument("--nq", type=int, default=2000)
    ap.add_argument("--nh", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--length-model", default="envelope", choices=("envelope", "sequence"),
                    help="the domain stage's length model (EHMM.set_domain_length_model)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_display.py needs a GPU: no figure is taken without one")
    alph, seed, root_len, leaves, sub, indel, qlen = HEADLINE
    fam = synth.make_family(seed, root_len, leaves, alph, sub, indel)
    with tempfile.TemporaryDirectory() as td:
        eh = synth.make_ehmm(fam, args.nh, td)
        _, seqs = synth.make_queries(fam, seed + 1, args.nq, qlen)
        e = EHMM(eh.paths, hmm_index=eh.index, nseq=eh.nseq)
    res, offs = pack_queries([s.astype(np.uint8) for s in seqs])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")      # noqa: E731
    res_t, offs_t = up(res), up(offs)
    max_len = int(np.diff(offs).max())
    e.set_domain_length_model(args.length_model)
    e.set_timing(True)
    runs = []
    for r in range(args.repeats + 1):                            # the first pass loads the code objects: reported apart
        deci, flags, det = e.score(res, offs, want_detail=True)
        score_ms = e.last_kernel_ms(0)[0] + e.last_kernel_ms(4)[0]
        flags_t, det_t = up(flags.reshape(-1)), up(np.frombuffer(bytes(det), dtype=np.uint8).copy())
        dom_t, dom_off_t, env_t, cols_t, pp_t = e.domain_paths_t(res_t, offs_t, max_len, flags_t, det_t)
        stage_ms = e.last_kernel_ms(5)[0]
        align_ms = e.last_kernel_ms(2)[0]
        recs = dom_t.cpu().numpy().reshape(-1).view(np.dtype(_lib.DOMAIN_FIELDS))
        room = (recs["hmm_j"] - recs["hmm_i"] + 1).astype(np.int64) + (recs["env_j"] - recs["env_i"] + 1)
        hh = recs["pair"] % e.H
        display_ms, launches, nsel, chars = 0.0, 0, 0, 0
        for h in range(e.H):
            d = e.domain_display_t(res_t, offs_t, flags_t, dom_off_t, dom_t, env_t, cols_t, pp_t, domE=10.0,
                                   domZ=max(int((flags[:, h] & 1).sum()), 1), h=h, cap=int(room[hh == h].sum()))
            ms, n = e.last_kernel_ms(9)
            display_ms += ms
            launches += n
            nsel += d["nsel"]
            chars += d["total"]
        runs.append({"score_ms": score_ms, "domain_stage_ms": stage_ms, "align_ms": align_ms, "display_ms": display_ms,
                     "display_launches": launches, "displayed_domains": nsel, "columns": chars})
        print(json.dumps(runs[-1]), flush=True)
    e.close()
    timed = runs[1:]
    med = {k: statistics.median(r[k] for r in timed) for k in ("score_ms", "domain_stage_ms", "align_ms", "display_ms")}
    out = {"tool": "tools/bench_display.py", "device": torch.cuda.get_device_name(0), "queries": args.nq, "models": args.nh,
           "pairs": int(args.nq * args.nh), "reported_pairs": int((flags & 1).sum()), "domains": int(len(recs)),
           "domains_with_a_path": int((recs["ali_i"] > 0).sum()), "displayed_domains": timed[-1]["displayed_domains"],
           "columns": timed[-1]["columns"], "display_calls": int(e.H), "first_pass": runs[0], "runs": timed, "median": med,
           "display_share_of_domain_stage": med["display_ms"] / med["domain_stage_ms"] if med["domain_stage_ms"] else None,
           "display_share_of_align_launches": med["display_ms"] / med["align_ms"] if med["align_ms"] else None}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
