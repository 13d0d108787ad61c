#!/usr/bin/env python3
"""Time the E-value calibration of a whole eHMM: host (16 threads) against the device batch.

The 15 models of the example backbone (tests/golden/example_e2e/backbone.fasta.gz, 1 278 .. 2 574 nodes), and the
same 15 repeated to 240:
  (a) build_ehmm(stats=False): what the pipeline does today (thread pool, no calibration);
  (b) host calibration: wh_hmmbuild2 with WH_BUILD_STATS from a pool of 16 threads - the yardstick;
  (c) the device batch: ONE wh_hmmbuild_batch call with WH_BUILD_STATS.  The first device call is run and reported
      apart (it loads the code objects); the figure is the median of the following calls.  The call builds its models
      one after the other on the host, so the same batch without WH_BUILD_STATS is timed too: the difference is the
      calibration (conversion, upload, kernel, fits).
The texts of (b) and (c) are compared.  Writes one JSON file (default profiles/calibrate_mi355x.json).

    python tools/bench_calibrate.py [--out FILE] [--repeats 3] [--device 0]
"""
import argparse
import gzip
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from witch_amd import synth                                                                   # noqa: E402
from witch_amd.gcmm.hmmbuild import build_ehmm, hmmbuild_text, hmmbuild_text_batch            # noqa: E402


def backbone():
    names, rows = [], []
    with gzip.open(os.path.join(ROOT, "tests", "golden", "example_e2e", "backbone.fasta.gz"), "rt") as fh:
        for line in fh:
            line = line.strip()
            if line.startswith(">"):
                names.append(line[1:].split()[0])
                rows.append("")
            elif line:
                rows[-1] += line
    return names, [r.upper() for r in rows]


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "calibrate_mi355x.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_calibrate.py needs a GPU: no figure is taken without one")
    names, rows = backbone()
    subs = synth.bfs_subsets(len(rows), 15)
    lists15 = [rows[lo:hi] for lo, hi in subs]
    res = {"tool": "tools/bench_calibrate.py", "device": torch.cuda.get_device_name(args.device), "host_threads": args.threads,
           "repeats": args.repeats, "sizes": {}}
    first = None
    for count in (15, 240):
        lists = lists15 * (count // 15)
        r = {}
        with tempfile.TemporaryDirectory() as td:
            subsets = [("A_0_%d" % i, list(range(*subs[i % 15]))) for i in range(count)]
            r["a_build_ehmm_nostats_s"], _ = timed(lambda: build_ehmm(names, rows, subsets, "dna", td, threads=args.threads))
        with ThreadPoolExecutor(max_workers=args.threads) as ex:
            r["b_host_calibration_s"], host = timed(lambda: list(ex.map(lambda x: hmmbuild_text(x, "dna", "sub", stats=True), lists)))
        r["batch_build_only_s"], _ = timed(lambda: hmmbuild_text_batch(lists, "dna", device=-1))
        if first is None:
            first, _ = timed(lambda: hmmbuild_text_batch(lists, "dna", stats=True, device=args.device))
            res["first_device_call_s"] = first
        runs = []
        for _ in range(args.repeats):
            t, dev = timed(lambda: hmmbuild_text_batch(lists, "dna", stats=True, device=args.device))
            runs.append(t)
        assert [d[0] for d in dev] == [h[0] for h in host], "device and host texts differ"
        r["c_device_batch_runs_s"] = runs
        r["c_device_batch_s"] = statistics.median(runs)
        r["c_minus_build_s"] = r["c_device_batch_s"] - r["batch_build_only_s"]
        r["speedup_b_over_c"] = r["b_host_calibration_s"] / r["c_device_batch_s"]
        r["nodes"] = [d[1] for d in dev[:15]]
        res["sizes"][str(count)] = r
        print(count, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
