"""Shared by tests/test_filters_classes_host.py, tests/test_filters_classes_gpu.py and the two fixture generators: the
fixtures "classes_dna" and "classes_amino" of tests/golden/filters (hmmsearch --nobias) and tests/golden/filters_bias
(hmmsearch with its bias filter) - the reference's bundled hmmsearch on one model per size class of wh_filter.hip.

The models are no files of a golden case: they are made from seeds exactly as _models() of tests/test_filters_gpu.py
makes them, and a fixture holds M, the seed and the sha256 of the model text the binary read (a writer that drifts fails
loudly).  A variant "mu40" is the same text with the mu of its STATS LOCAL MSV line at -40: low MSV scores then have a
P-value below 1, which the writer's own -10 saturates.  A fixture is ragged: every model has its own queries followed by
the shared ones."""
import atexit
import gzip
import hashlib
import json
import math
import os
import shutil
import tempfile

import numpy as np

from tests.conftest import GOLDEN
from tests.filters_common import digitize, pack

CLASSES = {"classes_dna": "dna", "classes_amino": "amino"}
# every class edge of wh_filter.hip (2, 4, 8, 16, 32, 48 cells per lane) and the scalar cores beyond 3 072 nodes
LENGTHS = {"dna": [1, 2, 3, 5, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 3072, 3073],
           "amino": [5, 64, 129, 257, 513, 1025, 2049, 3072, 3073]}
# the models that exist a second time with the MSV mu at -40
MU40 = {"dna": [1, 2, 3, 5, 513], "amino": [5, 513, 3072]}
# the mu40 model whose own queries include the "limit" ones: runs of the 'any' code so long that tjb + tbm + tec + bias
# passes 127, where the binary's MSV stage stops honouring the empty diagonal (wh_calibrate.h, calib_msv_floor).  They are
# tens of thousands of residues long: the full matrix leaves them out, they run on their own model alone (limit_call)
LIMIT_MODEL = {"amino": 3072}
LIMIT_LENGTHS = (30000, 45000)
MSV_LINE = "STATS LOCAL MSV      -10.0000  0.70000\n"
MSV_LINE_MU40 = "STATS LOCAL MSV      -40.0000  0.70000\n"
_cache = {}
_tmp = []


def _tmpdir():
    if not _tmp:
        _tmp.append(tempfile.mkdtemp(prefix="filters_classes_"))
        atexit.register(shutil.rmtree, _tmp[0], ignore_errors=True)
    return _tmp[0]


def model_list(alphabet):
    """[(M, variant)] in the fixture's order: every length as written, then the mu40 variants"""
    return [(M, "plain") for M in LENGTHS[alphabet]] + [(M, "mu40") for M in MU40[alphabet]]


def synth_model(alphabet, M):
    """(SynthHMM, model text) of seed 1000 + M"""
    from witch_amd import synth
    fam = synth.make_family(1000 + M, M, 4, alphabet, indel_rate=0.0)
    h = synth.build_hmm(fam, 0, 4, "syn%d" % M)
    assert h.M == M
    p = os.path.join(_tmpdir(), "w_%s_%d_%d.hmm" % (alphabet, M, os.getpid()))
    synth.write_hmm(h, p)
    with open(p) as f:
        text = f.read()
    os.unlink(p)
    return h, text


def model_text(alphabet, M, variant):
    h, text = synth_model(alphabet, M)
    if variant == "mu40":
        assert text.count(MSV_LINE) == 1
        text = text.replace(MSV_LINE, MSV_LINE_MU40)
    else:
        assert variant == "plain"
    return h, text


def model_file(alphabet, M, variant, text, folder=None):
    p = os.path.join(folder or _tmpdir(), "syn_%s_%d_%s.hmm" % (alphabet, M, variant))
    with open(p, "w") as f:
        f.write(text)
    return p


def sha256(text):
    return hashlib.sha256(text.encode()).hexdigest()


class ClassesFixture:
    """kind: "filters" (brackets T1, T2, T3 of --nobias) or "filters_bias" (T1, Tb, T2b, T3b with the bias filter)"""

    def __init__(self, name, kind):
        with gzip.open(os.path.join(GOLDEN, kind, name + ".json.gz"), "rt") as f:
            self.g = json.load(f)
        self.name, self.kind = name, kind
        self.alph_name = self.g["alphabet"]
        assert self.alph_name == CLASSES[name]
        self.alphabet = {"dna": 0, "amino": 2}[self.alph_name]
        self.models = self.g["models"]
        self.floor = self.g["ln_lo"]
        assert [(m["M"], m["variant"]) for m in self.models] == model_list(self.alph_name)
        self.paths = []
        for m in self.models:
            assert m["seed"] == 1000 + m["M"]
            h, text = model_text(self.alph_name, m["M"], m["variant"])
            assert sha256(text) == m["sha256"], (name, m["M"], m["variant"], "the model writer's text changed")
            self.paths.append(model_file(self.alph_name, m["M"], m["variant"], text))
        self.H = len(self.models)
        # the full matrix: every model's own queries, then the shared ones; listed[q, h]: the pair is in the fixture
        # (pair_q[h][i]: the matrix row of model h's i-th pair, None for a "limit" query, which is in no matrix)
        self.shared = [tuple(q) for q in self.g["shared_queries"]]
        allq, self.pair_q = [], []
        for m in self.models:
            rows = []
            for n, t in m["queries"]:
                rows.append(None if n.startswith("limit") else len(allq))
                if rows[-1] is not None:
                    allq.append((n, t))
            self.pair_q.append(rows)
        for h in range(self.H):
            self.pair_q[h] += list(range(len(allq), len(allq) + len(self.shared)))
            assert len(self.pair_q[h]) == len(self.models[h]["pairs"])
        allq += self.shared
        self.qnames = [q[0] for q in allq]
        self.qtext = [q[1] for q in allq]
        self.seqs = [digitize(self.alphabet, t) for t in self.qtext]
        self.res, self.off = pack(self.seqs)
        self.nq = len(self.seqs)
        self.listed = np.zeros((self.nq, self.H), dtype=bool)
        for q, h, p in self.pairs():
            self.listed[q, h] = True
        self.npairs = int(self.listed.sum())

    def F(self, key):
        return tuple(self.g["thresholds"][key])

    def model_names(self, h):
        return [n for n, _ in self.models[h]["queries"]] + [n for n, _ in self.shared]

    def model_call(self, h, limit=None):
        """(res, off, lengths, records) of model h alone: its listed pairs in the fixture's order.  limit: None - all of
        them; True / False - only the "limit" queries / all but them"""
        texts = [t for _, t in self.models[h]["queries"]] + [t for _, t in self.shared]
        keep = [i for i, r in enumerate(self.pair_q[h]) if limit is None or (r is None) == limit]
        seqs = [digitize(self.alphabet, texts[i]) for i in keep]
        res, off = pack(seqs)
        return res, off, [len(s) for s in seqs], [self.models[h]["pairs"][i] for i in keep]

    def limit_models(self):
        return [h for h in range(self.H) if None in self.pair_q[h]]

    def pairs(self):
        """(q, h, record) of every listed pair of the matrix"""
        for h, m in enumerate(self.models):
            for q, p in zip(self.pair_q[h], m["pairs"]):
                if q is not None:
                    yield q, h, p

    def expected(self, key, stage):
        """0 / 1 [nq, H] of the listed pairs (0 elsewhere): the binary's outcome of <stage> at thresholds <key>"""
        out = np.zeros((self.nq, self.H), dtype=np.uint8)
        for q, h, p in self.pairs():
            out[q, h] = p["out"][key][stage]
        return out

    def near(self, key, brackets):
        """bool [nq, H]: a recorded threshold lies within its own bisection bracket of the F in use.  brackets: names
        among T1, T2, T3 (against F1, F2, F3) or Tb, T2b, T3b"""
        F = self.F(key)
        which = {"T1": 0, "T2": 1, "T3": 2, "Tb": 0, "T2b": 1, "T3b": 2}
        out = np.zeros((self.nq, self.H), dtype=bool)
        for q, h, p in self.pairs():
            for t in brackets:
                if p[t][1] > self.floor and p[t][0] <= math.log(F[which[t]]) <= p[t][1]:
                    out[q, h] = True
        return out

    def field(self, name, dtype=np.float64, missing=np.nan):
        out = np.full((self.nq, self.H), missing, dtype=dtype)
        for q, h, p in self.pairs():
            if p.get(name) is not None:
                out[q, h] = p[name]
        return out

    def bracket(self, name):
        """(lo, hi) [nq, H], nan off the list"""
        lo = np.full((self.nq, self.H), np.nan)
        hi = np.full((self.nq, self.H), np.nan)
        for q, h, p in self.pairs():
            lo[q, h], hi[q, h] = p[name]
        return lo, hi


def classes_fixture(name, kind="filters"):
    if (name, kind) not in _cache:
        _cache[(name, kind)] = ClassesFixture(name, kind)
    return _cache[(name, kind)]
