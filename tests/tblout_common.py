"""Shared by tests/test_tblout_host.py, tests/test_tblout_gpu.py and tests/golden/make_golden_tblout.py: the readers of the
fixture tests/golden/tblout (hmmsearch --tblout of the reference's bundled binary), the rule for its exp column, and the
seeded models and queries at the class edges of the counting sweep (wh_seqtab.hip).

The exp rule.  HMMER prints exp = btot[L] with "%.1f" from a float32 sum; wh_seq_expect_host forms the same sum in float64.
The printed texts are equal unless the float64 value lies within EXP_SLACK = 1e-3 of a print boundary x.x5: the float32 sum
over at most 3 072 rows of an exp of at most 4 is off by at most 3 072 x 2^-24 x 4 = 7.3e-4, rounded up.  On such a row the
two texts may be 0.1 apart; such rows number at most EXEMPT_CAP = 2 % of a fixture file (the generator asserts that
HMMER's own output stays inside this cap)."""
import functools
import gzip
import json
import os

import numpy as np

from tests.conftest import GOLDEN
from tests.filters_classes_common import model_file, model_text, sha256

GOLDEN_TBL = os.path.join(GOLDEN, "tblout")
CASES = ("dna_hmmbuild", "amino_hmmbuild", "amino_multidomain", "example_sub30")
COLUMNS = ["target", "tacc", "query", "qacc", "evalue", "score", "bias", "best_evalue", "best_score", "best_bias", "exp", "reg",
           "clu", "ov", "env", "dom", "rep", "inc"]
INT_COLUMNS = ("reg", "clu", "ov", "env", "dom", "rep", "inc")
EXP_SLACK = 1e-3
EXEMPT_CAP = 0.02

# the node counts at which the sweep takes another instantiation: 1, 2 and the lane edges of the smallest class, the last
# and first node count of every cells-per-lane class (4, 8, ... 48: 64 x Q nodes), and the hand-over to the any-size path
CLASS_NODES = sorted(set([1, 2, 63, 64, 65] + [64 * q for q in range(4, 49, 4)] + [64 * q + 1 for q in range(4, 49, 4)]))
CLASS_ALPHABETS = ("dna", "amino")
SYMS = {"dna": "ACGT", "amino": "ACDEFGHIKLMNPQRSTVWY"}
QUERY_LENGTHS = (1, 3, 63, 64, 65, 128, 129)


@functools.lru_cache(maxsize=None)
def load_fixture(name):
    with gzip.open(os.path.join(GOLDEN_TBL, name + ".json.gz"), "rt") as f:
        return json.load(f)


def exp_ok(value, printed):
    """(accepted, exempt) for the exp column: the text of <value> equals HMMER's, or <value> is within EXP_SLACK of a print
    boundary and the texts are one unit apart."""
    text = "%.1f" % value
    if text == printed:
        return True, False
    near = abs((abs(float(value)) * 10.0) % 1.0 - 0.5) < EXP_SLACK * 10.0
    return bool(near and abs(float(text) - float(printed)) < 0.1001), True


def parse_tblout(text):
    """(header lines, rows, trailer lines) of a --tblout file; a row: its 18 columns as strings, "desc" and "raw"."""
    header, rows, trailer = [], [], []
    for line in text.splitlines():
        if line.startswith("#"):
            (trailer if rows else header).append(line)
            continue
        w = line.split(None, 18)
        rec = dict(zip(COLUMNS, w[:18]))
        rec["desc"] = w[18] if len(w) > 18 else ""
        rec["raw"] = line
        rows.append(rec)
    if not rows:          # (a table without a row: the three header lines, then the trailer)
        header, trailer = header[:3], header[3:]
    return header, rows, trailer


# ------------------------------------------------------------------------------------------------ seeded class models
def _window(rng, cons, n):
    M = len(cons)
    if M >= n:
        a = int(rng.integers(0, M - n + 1))
        return cons[a:a + n].copy()
    return np.tile(cons, -(-n // M))[:n]


def _substitute(rng, s, rate, K):
    s = np.array(s, copy=True)
    mut = rng.random(len(s)) < rate
    s[mut] = rng.integers(0, K, size=int(mut.sum()))
    return s


def class_queries(alphabet, M, h):
    """[(name, residue codes uint8)] of one class model (h: its SynthHMM), seed 8000 + M, in call order: a tiny query first
    and last; windows of the consensus at the lengths around the 64-row batches of the posterior pass and the region
    scan; a tandem (two copies back to back: a multidomain region) and a chimera (two windows around a spacer: two regions)."""
    K = len(SYMS[alphabet])
    rng = np.random.default_rng(8000 + M)
    cons = np.argmax(h.mat[1:], axis=1)
    out = [("none_first", rng.integers(0, K, 3))]
    for n in QUERY_LENGTHS:
        out.append(("len%d" % n, _substitute(rng, _window(rng, cons, n), 0.1, K)))
    frag = _substitute(rng, _window(rng, cons, 40), 0.05, K)
    out.append(("tandem", np.concatenate([frag, frag])))
    out.append(("chimera", np.concatenate([_substitute(rng, _window(rng, cons, 40), 0.05, K), rng.integers(0, K, 25),
                                           _substitute(rng, _window(rng, cons, 40), 0.05, K)])))
    out.append(("none_last", rng.integers(0, K, 2)))
    return [(n, np.asarray(s, dtype=np.uint8)) for n, s in out]


def codes_text(alphabet, codes):
    return "".join(SYMS[alphabet][int(c)] for c in codes)


@functools.lru_cache(maxsize=None)
def class_models(alphabet):
    """[(M, model path, sha256 of its text, [(name, codes)])] for CLASS_NODES, made from seeds as the filter fixtures make them."""
    out = []
    for M in CLASS_NODES:
        h, text = model_text(alphabet, M, "plain")
        out.append((M, model_file(alphabet, M, "tblout", text), sha256(text), class_queries(alphabet, M, h)))
    return out


def class_call(alphabet):
    """One call over every class model of an alphabet: (paths, residues, offsets, pairs, names) - every model's own queries
    in model order; pairs[t] = q * H + h of the t-th listed pair (a model meets its own queries only), names[t] = (M, query
    name)."""
    from witch_amd.ehmm import pack_queries
    models = class_models(alphabet)
    H = len(models)
    seqs, pairs, names = [], [], []
    for h, (M, _, _, queries) in enumerate(models):
        for n, s in queries:
            pairs.append(len(seqs) * H + h)
            names.append((M, n))
            seqs.append(s)
    # the first and the last pair of the call have no domain: ONE residue against the largest register-class model (a few
    # residues already find a region in these models: a query that short leaves the flanking states little to compete with)
    rng = np.random.default_rng(8000)
    K, h_big = len(SYMS[alphabet]), [m[0] for m in models].index(3072)
    for name, front in (("call_first", True), ("call_last", False)):
        pair = len(seqs) * H + h_big
        seqs.append(rng.integers(0, K, 1).astype(np.uint8))
        pairs.insert(0, pair) if front else pairs.append(pair)
        names.insert(0, (3072, name)) if front else names.append((3072, name))
    res, offs = pack_queries(seqs)
    return [m[1] for m in models], res, offs, np.asarray(pairs, dtype=np.int64), names
