#!/usr/bin/env python3
"""hmmsearch's acceleration filters on the headline shape: 150-nt queries x the 200-model eHMM of bench.py's headline
workload (and its first model alone, the level-0 case).  Reported, not a gate:

  * the filter kernels alone (wh_filter_dev): pairs per second;
  * wh_score_filtered_dev against wh_score_dev on the same device-resident inputs;
  * the share of pairs each stage rejects.

The models are built from the family's subset alignments with this library's hmmbuild and CALIBRATED (STATS LOCAL lines
from wh_hmmbuild_batch on the device) - bench.py's own model files carry placeholder statistics, with which a rejection
share would mean nothing.  The filtered runs are those of hmmsearch --nobias; --bias times the filter kernels and the
filtered scoring a second time with HMMER's bias filter switched on (WH_BIAS_FILTER_ON) and reports both.

    python tools/bench_filters.py [--nq 8192] [--nh 200] [--reps 3] [--out profiles/filters_mi355x.json]
    python tools/bench_filters.py --bias --out profiles/filters_bias_mi355x.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def build_models(fam, n_hmms, outdir):
    from witch_amd import synth
    from witch_amd.gcmm.hmmbuild import hmmbuild_text_batch
    sym = np.frombuffer((synth.symbols(fam.alphabet) + "-").encode(), dtype=np.uint8)
    subs = synth.bfs_subsets(fam.n_leaves, n_hmms)
    rows = [[sym[fam.msa[i].astype(np.int64)].tobytes().decode() for i in range(lo, hi)] for lo, hi in subs]
    t0 = time.time()
    built = hmmbuild_text_batch(rows, molecule=fam.alphabet, names=["A_0_%d" % i for i in range(len(subs))], stats=True, device=0)
    paths = []
    for i, b in enumerate(built):
        p = os.path.join(outdir, "A_0_%d.hmm" % i)
        with open(p, "w") as f:
            f.write(b[0])
        paths.append(p)
    return paths, time.time() - t0


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), ms


def run_case(paths, res_t, off_t, maxlen, reps, F, bias=False):
    import torch
    from witch_amd._lib import check, lib
    from witch_amd.ehmm import EHMM
    e = EHMM(paths)
    nq, H = off_t.numel() - 1, len(paths)
    dev = res_t.device
    o = EHMM.filter_opts(F, bias=True) if bias else EHMM.filter_opts(F, nobias=True)
    stage = torch.empty((nq, H), dtype=torch.uint8, device=dev)
    deci = torch.empty((nq, H), dtype=torch.int32, device=dev)
    flags = torch.empty((nq, H), dtype=torch.uint8, device=dev)
    st = e._stream()

    def filt():
        check(lib().wh_filter_dev(e._h, res_t.data_ptr(), off_t.data_ptr(), nq, res_t.numel(), maxlen, C.byref(o), stage.data_ptr(),
                                  None, None, None, st), "wh_filter_dev")

    def plain():
        check(lib().wh_score_dev(e._h, res_t.data_ptr(), off_t.data_ptr(), nq, res_t.numel(), maxlen, deci.data_ptr(), flags.data_ptr(),
                                 None, None, st), "wh_score_dev")

    def filtered():
        check(lib().wh_score_filtered_dev(e._h, res_t.data_ptr(), off_t.data_ptr(), nq, res_t.numel(), maxlen, C.byref(o), deci.data_ptr(),
                                          flags.data_ptr(), None, None, stage.data_ptr(), st), "wh_score_filtered_dev")
    f_ms, f_all = timed(filt, reps)
    p_ms, p_all = timed(plain, reps)
    reported_plain = int((flags & 1).sum().item())
    s_ms, s_all = timed(filtered, reps)
    c = e.last_filter_counts()
    reported = int((flags & 1).sum().item())
    e.close()
    n = float(c["pairs"])
    return {"models": H, "queries": nq, "pairs": c["pairs"], "thresholds": list(F), "bias_filter": bool(bias),
            "filter_kernels_ms": f_ms, "filter_kernels_ms_all": f_all, "filter_pairs_per_s": n / (f_ms * 1e-3),
            "wh_score_ms": p_ms, "wh_score_ms_all": p_all, "wh_score_filtered_ms": s_ms, "wh_score_filtered_ms_all": s_all,
            "filtered_over_plain": s_ms / p_ms,
            "rejected_share": {"msv": 1 - c["msv"] / n, "bias": (c["msv"] - c["bias"]) / n, "viterbi": (c["bias"] - c["vit"]) / n, "forward": (c["vit"] - c["fwd"]) / n},
            "passed": {k: c[k] for k in ("msv", "bias", "vit", "fwd")}, "pairs_scored": c["scored"],
            "reported_plain": reported_plain, "reported_filtered": reported}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=8192)
    ap.add_argument("--nh", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--bias", action="store_true", help="also with the bias filter on (keys H200_bias, H1_bias)")
    ap.add_argument("--note", default="", help="free text stored with the result (e.g. a figure printed by the tests)")
    a = ap.parse_args()
    import torch
    from witch_amd import synth
    alph, seed, root_len, leaves, sub, indel, n_hmms, _, qlen, k = bench.WORKLOADS["dna_100k_x200"]
    fam = synth.make_family(seed, root_len, leaves, alph, sub, indel)
    names, seqs = synth.make_queries(fam, seed + 1, a.nq, qlen)
    with tempfile.TemporaryDirectory() as wd:
        paths, build_s = build_models(fam, a.nh, wd)
        off = np.zeros(len(seqs) + 1, np.int64)
        off[1:] = np.cumsum([len(s) for s in seqs])
        res = np.concatenate(seqs).astype(np.uint8)
        res_t, off_t = torch.from_numpy(res).cuda(), torch.from_numpy(off).cuda()
        F = (0.02, 1e-3, 1e-5)
        out = {"device": torch.cuda.get_device_name(0), "workload": "dna_100k_x200 (queries: the first %d)" % a.nq,
               "query_len": int(qlen), "calibrated_build_s": build_s, "note": a.note,
               "H200": run_case(paths, res_t, off_t, int(qlen), a.reps, F),
               "H1": run_case(paths[:1], res_t, off_t, int(qlen), a.reps, F)}
        if a.bias:
            out["H200_bias"] = run_case(paths, res_t, off_t, int(qlen), a.reps, F, bias=True)
            out["H1_bias"] = run_case(paths[:1], res_t, off_t, int(qlen), a.reps, F, bias=True)
            for k_ in ("H200", "H1"):
                out[k_ + "_bias"]["filter_kernels_on_over_off"] = out[k_ + "_bias"]["filter_kernels_ms"] / out[k_]["filter_kernels_ms"]
    if a.out and os.path.exists(a.out):        # the key tests/test_filters_gpu.py writes into the same file stays
        try:
            old = json.load(open(a.out))
            if "forward_stage_largest_ln_p_difference" in old:
                out["forward_stage_largest_ln_p_difference"] = old["forward_stage_largest_ln_p_difference"]
        except ValueError:
            pass
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
