#!/usr/bin/env python3
"""Time the counting sweep and the row assembly of hmmsearch --tblout (wh_seq_expect, wh_seq_table) beside the scoring call
of the same inputs.

8 192 headline-shaped queries x 200 models from witch_amd.synth, built as bench.py builds its headline workload (the
dna_100k_x200 family and query recipe, fewer queries).  wh_score with detail records - timed with HIP events through
wh_last_kernel_ms, slots 0 + 4 (kernels + resolver) - then, on tensors resident on the device and between two HIP events on
the stream: wh_seq_expect_dev over the reported pairs (the sweep: P1 and P2 at full width for every reported pair, and the
read-back of the pair list that orders them by model), and wh_seq_table_dev (the compaction, the same sweep, the row
kernel).  Median of three after a first pass that loads the code objects.  The stage is an opt-in and has no gate; the
ratio says what a table costs next to the search it describes.  Writes one JSON file (default profiles/tblout_mi355x.json).

    python tools/bench_tblout.py [--out FILE] [--nq 8192] [--nh 200] [--repeats 3]
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
from witch_amd._lib import SEQ_ROW_FIELDS                       # noqa: E402
from witch_amd.ehmm import EHMM, pack_queries                   # noqa: E402

HEADLINE = ("dna", 20251205, 900, 1024, 0.03, 1e-4, 150)       # bench.py: WORKLOADS["dna_100k_x200"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tblout_mi355x.json"))
    ap.add_argument("--nq", type=int, default=8192)
    ap.add_argument("--nh", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_tblout.py needs a GPU: no figure is taken without one")
    alph, seed, root_len, leaves, sub, indel, qlen = HEADLINE
    fam = synth.make_family(seed, root_len, leaves, alph, sub, indel)
    with tempfile.TemporaryDirectory() as td:
        eh = synth.make_ehmm(fam, args.nh, td)
        _, seqs = synth.make_queries(fam, seed + 1, args.nq, qlen)
        e = EHMM(eh.paths, hmm_index=eh.index, nseq=eh.nseq)
    res, offs = pack_queries([s.astype(np.uint8) for s in seqs])
    max_len = int(np.diff(offs).max())
    dev = torch.device("cuda")
    e.set_timing(True)
    runs, rows = [], None
    for r in range(args.repeats + 1):                            # the first pass loads the code objects: reported apart
        deci, flags, det = e.score(res, offs, want_detail=True)
        score_ms = e.last_kernel_ms(0)[0] + e.last_kernel_ms(4)[0]
        res_t, offs_t, flags_t = torch.from_numpy(res).to(dev), torch.from_numpy(offs).to(dev), torch.from_numpy(flags).to(dev)
        det_t = torch.from_numpy(np.frombuffer(bytes(det), dtype=np.uint8).copy()).to(dev)
        pairs_t = torch.nonzero(flags_t.reshape(-1) & 1).reshape(-1).contiguous()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        torch.cuda.synchronize()
        ev[0].record()
        e.seq_expect_t(res_t, offs_t, max_len, pairs_t)
        ev[1].record()
        torch.cuda.synchronize()
        ev[2].record()
        rows_t = e.seq_table_t(res_t, offs_t, max_len, flags_t, det_t, cap=int(pairs_t.numel()))
        ev[3].record()
        torch.cuda.synchronize()
        sweep_ms, table_ms = ev[0].elapsed_time(ev[1]), ev[2].elapsed_time(ev[3])
        runs.append({"score_ms": score_ms, "sweep_ms": sweep_ms, "table_ms": table_ms, "around_sweep_ms": table_ms - sweep_ms})
        rows = np.frombuffer(rows_t.cpu().numpy().tobytes(), dtype=np.dtype(SEQ_ROW_FIELDS))
        print(json.dumps(runs[-1]), flush=True)
    status = e.last_seq_table_status()
    e.close()
    timed = runs[1:]
    med = {k: statistics.median(r[k] for r in timed) for k in ("score_ms", "sweep_ms", "table_ms", "around_sweep_ms")}
    out = {"tool": "tools/bench_tblout.py", "device": torch.cuda.get_device_name(0), "queries": args.nq, "models": args.nh,
           "pairs": int(args.nq * args.nh), "reported_pairs": int(len(rows)), "status": status,
           "rows_with_a_clustered_region": int((rows["clu"] > 0).sum()), "mean_exp": float(rows["exp"].mean()) if len(rows) else 0.0,
           "first_pass": runs[0], "runs": timed, "median": med,
           "sweep_share_of_scoring": med["sweep_ms"] / med["score_ms"] if med["score_ms"] else None,
           "table_share_of_scoring": med["table_ms"] / med["score_ms"] if med["score_ms"] else None}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
