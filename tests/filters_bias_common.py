"""Shared by tests/test_filters_bias_host.py and tests/test_filters_bias_gpu.py: the fixtures of tests/golden/filters_bias
(written by tests/golden/make_golden_filters_bias.py from the reference's bundled hmmsearch WITHOUT --nobias)."""
import atexit
import gzip
import json
import math
import os
import shutil
import tempfile

import numpy as np

from tests.conftest import GOLDEN, load_case
from tests.filters_common import digitize, pack

BIAS_FIXTURES = ["lowcomplexity", "amino_hmmbuild", "dna_lowcomplexity", "nocompo"]
BIAS_ON = 2                # WH_BIAS_FILTER_ON
_cache = {}
_tmp = []


def _tmpdir():
    if not _tmp:
        _tmp.append(tempfile.mkdtemp(prefix="filters_bias_"))
        atexit.register(shutil.rmtree, _tmp[0], ignore_errors=True)
    return _tmp[0]


class BiasFixture:
    def __init__(self, name):
        with gzip.open(os.path.join(GOLDEN, "filters_bias", name + ".json.gz"), "rt") as f:
            self.g = json.load(f)
        self.name = name
        self.models = self.g["models"]
        self.paths = []
        for m in self.models:
            case = load_case(m["golden_case"])
            p = case.hmm_paths[m["position"]]
            if "hmm_text" in m:               # the file the binary read is not a golden case's: it is in the fixture
                p = os.path.join(_tmpdir(), "%s_%d.hmm" % (name, m["position"]))
                with open(p, "w") as f:
                    f.write(m["hmm_text"])
            self.paths.append(p)
        self.alphabet = {"dna": 0, "rna": 1, "amino": 2}.get(case.alphabet, case.alphabet)
        self.qnames = [q[0] for q in self.g["queries"]]
        self.qtext = [q[1] for q in self.g["queries"]]
        self.seqs = [digitize(self.alphabet, t) for t in self.qtext]
        self.res, self.off = pack(self.seqs)
        self.H, self.nq = len(self.paths), len(self.seqs)
        self.floor = self.g["ln_lo"]

    def F(self, key):
        return tuple(self.g["thresholds"][key])

    def expected(self, key, stage):
        """0 / 1 [nq, H]: the binary's outcome of <stage> (0 MSV, 1 bias, 2 Viterbi, 3 Forward) at thresholds <key>"""
        return np.array([[m["pairs"][q]["out"][key][stage] for m in self.models] for q in range(self.nq)], dtype=np.uint8)

    def near(self, key, brackets=("Tb", "T2b")):
        """bool [nq, H]: a recorded threshold (Tb against F1, T2b against F2, T3b against F3) lies within its own bisection
        bracket of the F in use"""
        F = self.F(key)
        which = {"Tb": 0, "T2b": 1, "T3b": 2}
        out = np.zeros((self.nq, self.H), dtype=bool)
        for h, m in enumerate(self.models):
            for q, p in enumerate(m["pairs"]):
                for t in brackets:
                    if p[t][1] > self.floor and p[t][0] <= math.log(F[which[t]]) <= p[t][1]:
                        out[q, h] = True
        return out

    def viterbi_ran(self, key):
        """(known, ran) bool [nq, H]: whether the Viterbi sweep ran in the binary, where its output decides it.  The sweep
        runs for a pair past the bias stage whose bias-stage P is above F2.  Tb = max(P_MSV, P_bias): below F2 the sweep
        did not run; above F2 it ran if the bias stage's P is the larger one (Tb above T1, the MSV stage's P)."""
        F = self.F(key)
        known = np.zeros((self.nq, self.H), dtype=bool)
        ran = np.zeros((self.nq, self.H), dtype=bool)
        for h, m in enumerate(self.models):
            for q, p in enumerate(m["pairs"]):
                if not p["out"][key][1]:
                    known[q, h] = True
                elif p["Tb"][1] < math.log(F[1]):
                    known[q, h] = True
                elif p["Tb"][0] > math.log(F[1]) and p["Tb"][0] > p["T1"][1]:
                    known[q, h] = ran[q, h] = True
        return known, ran


def bias_fixture(name):
    if name not in _cache:
        _cache[name] = BiasFixture(name)
    return _cache[name]
