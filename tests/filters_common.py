"""Shared by tests/test_filters_host.py and tests/test_filters_gpu.py: the fixtures of tests/golden/filters (written by
tests/golden/make_golden_filters.py from the reference's bundled hmmsearch) and the calls into the library."""
import ctypes as C
import gzip
import json
import math
import os

import numpy as np

from tests.conftest import GOLDEN, load_case

FIXTURES = ["amino_hmmbuild", "dna_hmmbuild", "dna_synth", "amino_multidomain", "lowcomplexity"]
MAX_SKIP = 0.01            # pairs of a case whose recorded threshold lies within its own bracket of the F in use
_cache = {}


class Fixture:
    def __init__(self, name):
        with gzip.open(os.path.join(GOLDEN, "filters", name + ".json.gz"), "rt") as f:
            self.g = json.load(f)
        self.name = name
        self.case = load_case(self.g["golden_case"])
        self.alphabet = {"dna": 0, "rna": 1, "amino": 2}.get(self.case.alphabet, self.case.alphabet)
        self.models = self.g["models"]
        self.paths = [self.case.hmm_paths[m["position"]] for m in self.models]
        self.qnames = [q[0] for q in self.g["queries"]]
        self.qtext = [q[1] for q in self.g["queries"]]
        self.seqs = [digitize(self.alphabet, t) for t in self.qtext]
        self.res, self.off = pack(self.seqs)
        self.H, self.nq = len(self.paths), len(self.seqs)

    def F(self, key):
        return tuple(self.g["thresholds"][key])

    def expected(self, key, stage):
        """0 / 1 [nq, H]: the binary's outcome of <stage> (0 MSV, 1 bias, 2 Viterbi, 3 Forward) at thresholds <key>"""
        return np.array([[m["pairs"][q]["out"][key][stage] for m in self.models] for q in range(self.nq)], dtype=np.uint8)

    def near(self, key, stages=(0, 1, 2)):
        """bool [nq, H]: a recorded threshold (T1, T2, T3 by stage 0, 2, 3) lies within its own bisection bracket of the F in use"""
        F = self.F(key)
        out = np.zeros((self.nq, self.H), dtype=bool)
        for h, m in enumerate(self.models):
            for q, p in enumerate(m["pairs"]):
                for t, i, st in (("T1", 0, 0), ("T2", 1, 2), ("T3", 2, 3)):
                    if st in stages and p[t][1] > self.g["ln_lo"] and p[t][0] <= math.log(F[i]) <= p[t][1]:
                        out[q, h] = True
        return out


def fixture(name):
    if name not in _cache:
        _cache[name] = Fixture(name)
    return _cache[name]


def digitize(alphabet, text):
    from witch_amd import _lib
    out = np.zeros(len(text), np.uint8)
    assert _lib.lib().wh_digitize(alphabet, text.encode(), len(text), out.ctypes.data) == 0
    return out


def pack(seqs):
    off = np.zeros(len(seqs) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    res = np.concatenate([np.asarray(s, np.uint8) for s in seqs]) if len(seqs) else np.zeros(0, np.uint8)
    return np.ascontiguousarray(res), off


def filter_host(paths, res, off, F, nobias=1):
    """wh_filter_host -> (rc, stage, bias, msv_raw, vit_raw, counts4)"""
    from witch_amd import _lib
    L = _lib.lib()
    H, nq = len(paths), len(off) - 1
    arr = (C.c_char_p * H)(*[str(p).encode() for p in paths])
    o = _lib.FilterOpts(F[0], F[1], F[2], nobias)
    stage = np.zeros((nq, H), np.uint8)
    bias = np.zeros((nq, H), np.float32)
    msv = np.zeros((nq, H), np.int32)
    vit = np.zeros((nq, H), np.int32)
    cnt = np.zeros(4, np.int64)
    rc = L.wh_filter_host(arr, H, res.ctypes.data, off.ctypes.data, nq, C.byref(o), stage.ctypes.data, bias.ctypes.data,
                          msv.ctypes.data, vit.ctypes.data, cnt.ctypes.data)
    return rc, stage, bias, msv, vit, cnt


def msv_tjb(L):
    """the MSV filter's N/C/J move cost for a query of L residues: -round(scale * logf(3 / (L + 3))), scale = 3 / ln 2"""
    v = np.log(np.float32(3.0) / (np.float32(L) + np.float32(3.0)), dtype=np.float32)
    return int(-np.round(np.float32(3.0 / 0.69314718055994529) * v))
