"""Reference for the per-residue posterior probabilities of an alignment (hmmalign's PP line) and the readers of the
fixture tests/golden/align_pp (tests/test_align_pp_host.py, tests/test_align_pp.py).

The arithmetic is tests/pp_reference.c, built here on first use the way oracle/ builds its library (cc, into the temp
directory): unihit-local Forward / Backward / posterior decoding with the recurrences, the row rescaling and the float32
pmove / ploop of oracle/p7_oracle.c, on the model parameters the oracle exposes (OracleHMM.pt / odds / entry), evaluated
along a given column path.  Results are float64.
"""
import ctypes as C
import functools
import gzip
import json
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_PP = os.path.join(_HERE, "golden", "align_pp")
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        src = os.path.join(_HERE, "pp_reference.c")
        d = os.path.join(tempfile.gettempdir(), "witch_ppref_%d" % os.getuid())
        os.makedirs(d, exist_ok=True)
        so = os.path.join(d, "libppref.so")
        if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
            tmp = "%s.tmp.%d" % (so, os.getpid())
            subprocess.check_call(["cc", "-O2", "-fPIC", "-shared", "-o", tmp, src, "-lm"])
            os.replace(tmp, so)
        L = C.CDLL(so)
        L.ppref_path.restype = C.c_int
        L.ppref_path.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double,
                                 C.c_void_p, C.c_void_p, C.c_void_p]
        _LIB = L
    return _LIB


def len_config(L):
    """Unihit length model; HMMER forms pmove / ploop in float32."""
    pmove = np.float32(2.0) / (np.float32(L) + np.float32(2.0))
    ploop = np.float32(1.0) - pmove
    return float(ploop), float(pmove)


def path_states(cols):
    """Per residue (state, node): state 0 = M, 1 = I, 2 = N, 3 = C; node k (1-based) for M and I, 0 for a flank.
    None when the path has no match state (a pair returned without a path)."""
    cols = np.asarray(cols, dtype=np.int64)
    hit = np.nonzero(cols >= 0)[0]
    if len(hit) == 0:
        return None
    st = np.empty(len(cols), dtype=np.int64)
    kk = np.zeros(len(cols), dtype=np.int64)
    first, last = hit[0], hit[-1]
    st[:first] = 2
    st[last + 1:] = 3
    k = 0
    for i in range(first, last + 1):
        if cols[i] >= 0:
            k = int(cols[i]) + 1
            st[i] = 0
        else:
            st[i] = 1
        kk[i] = k
    return st, kk


class Model:
    """The oracle's configured profile, as arrays."""

    def __init__(self, ohm):
        self.M = int(ohm.M)
        self.pt = np.ascontiguousarray(ohm.pt, dtype=np.float64)            # [M + 1][7]
        self.odds = np.ascontiguousarray(ohm.odds, dtype=np.float64)        # [Kp][M + 1]
        self.entry = np.ascontiguousarray(ohm.entry, dtype=np.float64)      # [M + 2]
        self.Kp = self.odds.shape[0]


def path_posteriors(model, dsq, cols):
    """float64 posterior of every residue of <dsq> along the path <cols> (0 for a path without a match state)."""
    dsq = np.ascontiguousarray(np.minimum(np.asarray(dsq, dtype=np.int64), model.Kp - 1), dtype=np.uint8)
    L = len(dsq)
    out = np.zeros(L, dtype=np.float64)
    ps = path_states(cols)
    if ps is None or L == 0:
        return out
    st = np.ascontiguousarray(ps[0], dtype=np.int32)
    kk = np.ascontiguousarray(ps[1], dtype=np.int32)
    loop, move = len_config(L)
    lib().ppref_path(model.M, model.pt.ctypes.data, model.odds.ctypes.data, model.entry.ctypes.data, dsq.ctypes.data, L,
                     loop, move, st.ctypes.data, kk.ctypes.data, out.ctypes.data)
    return out


# ------------------------------------------------------------------------------------------------ seeded inputs
def long_model(spec, outdir):
    """The 1 900-node model of the long_model fixture, written into <outdir> from the seeds in <spec>: (family, path)."""
    from witch_amd import synth
    p = spec["family"]
    fam = synth.make_family(p["seed"], p["root_len"], p["n_leaves"], p["alphabet"], p["sub_rate"], p["indel_rate"])
    eh = synth.make_ehmm(fam, spec["n_subsets"], outdir, witch_layout=False)
    return fam, eh.paths[spec["model"]]


def long_queries(spec, fam):
    """(names, residue-code arrays, class per query: "fragment" / "multicopy")."""
    from witch_amd import synth
    f, m = spec["fragments"], spec["multicopy"]
    _, frag = synth.make_queries(fam, f["seed"], f["n"], tuple(f["length"]))
    _, multi = synth.make_queries(fam, m["seed"], m["n"], tuple(m["length"]), flank_frac=m["flank_frac"])
    seqs = list(frag) + [multi[t] for t in m["keep"]]
    kinds = ["fragment"] * len(frag) + ["multicopy"] * len(m["keep"])
    return ["ppq%02d" % t for t in range(len(seqs))], [s.astype(np.uint8) for s in seqs], kinds


def window_case(alphabet, outdir):
    """Two 700-node models (8 or more nodes per lane: the node window's range; the golden models are shorter) and 36
    fragment queries, some in random flanks: (model paths, names, residue-code arrays).  Fixture: window_<alphabet>."""
    from witch_amd import synth
    fam = synth.make_family(4242 + 700, 700, 16, alphabet, 0.04 if alphabet == "dna" else 0.03, 1e-4)
    eh = synth.make_ehmm(fam, 2, outdir, witch_layout=False)
    _, s1 = synth.make_queries(fam, 11, 24, (40, 250), 0.05)
    _, s2 = synth.make_queries(fam, 12, 12, (40, 250), 0.15, flank_frac=0.4)
    seqs = [x.astype(np.uint8) for x in s1 + s2]
    return eh.paths, ["w%03d" % t for t in range(len(seqs))], seqs


def fixture_reference(name, hmm_paths, seqs):
    """Like case_reference for a fixture whose models and queries are regenerated from seeds."""
    from oracle import oracle as orc
    models = [Model(orc.OracleHMM(p)) for p in hmm_paths]
    out = []
    for rec in load_fixture(name)["pairs"]:
        _, row, pp, _, rf = parse_stockholm(rec["sto"])
        cols, digits = row_cols_digits(row, pp, rf)
        out.append((rec["q"], rec["h"], cols, digits, path_posteriors(models[rec["h"]], seqs[rec["q"]], cols)))
    return out


# ------------------------------------------------------------------------------------------------ fixture readers
def parse_stockholm(text):
    """hmmalign's single-sequence Stockholm text -> (name, row, pp line, PP_cons line or None, RF line or None)."""
    name, row, pp, cons, rf = None, "", "", "", ""
    for line in text.splitlines():
        if line.startswith("#=GR"):
            w = line.split()
            if w[2] == "PP":
                pp += w[3]
        elif line.startswith("#=GC PP_cons"):
            cons += line.split()[2]
        elif line.startswith("#=GC RF"):
            rf += line.split()[2]
        elif line.strip() and not line.startswith(("#", "//")):
            n, s = line.split()
            name = n
            row += s
    return name, row, pp, cons or None, rf or None


def row_cols_digits(row, pp, rf):
    """Per residue: the 0-based match column (or -1) by the RF line, and hmmalign's PP character."""
    cols, digits, k = [], [], -1
    for c, p, r in zip(row, pp, rf):
        if r == "x":
            k += 1
        if c not in "-.":
            cols.append(k if r == "x" else -1)
            digits.append(p)
    return np.array(cols, dtype=np.int32), "".join(digits)


@functools.lru_cache(maxsize=None)
def load_fixture(name):
    """tests/golden/align_pp/<name>.json.gz: {"pairs": [{"q", "h", "sto"}], ...}."""
    with gzip.open(os.path.join(GOLDEN_PP, name + ".json.gz"), "rt") as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """For a golden case of tests/conftest.py with a PP fixture: per stored pair (q, h, cols, hmmalign's digits, float64
    reference posteriors).  Computed once per process and shared; callers do not modify it."""
    from oracle import oracle as orc
    from tests.conftest import load_case
    case = load_case(name)
    fx = load_fixture(name)
    ohm = [orc.OracleHMM(p) for p in case.hmm_paths]
    models = [Model(o) for o in ohm]
    seqs = [ohm[0].digitize(s.upper()) for s in case.qseqs]
    out = []
    for rec in fx["pairs"]:
        _, row, pp, _, rf = parse_stockholm(rec["sto"])
        cols, digits = row_cols_digits(row, pp, rf)
        ref = path_posteriors(models[rec["h"]], seqs[rec["q"]], cols)
        out.append((rec["q"], rec["h"], cols, digits, ref))
    return out
