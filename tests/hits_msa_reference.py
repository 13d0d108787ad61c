"""Reference of hmmsearch -A (wh_hits_msa) in plain numpy, and the readers of the fixtures under tests/golden/hits_msa
(tests/golden/make_golden_hits_msa.py).  Pure CPU.

The recipe: the oracle's domain records (tests/domains_reference.case_reference) -> the domains that satisfy the inclusion
thresholds, in HMMER's hit order and domain order -> each sliced to ali_i..ali_j, its posteriors quantised as HMMER keeps
them (the displayed PP character decoded again) -> tests/msa_reference.assemble -> formats.format_hits_msa.

PP_cons: HMMER's p7_tracealign sums the rows' float posteriors in a double, divides by (float) n and hands the quotient to
p7_alidisplay_EncodePostProb(float): the mean is rounded to float32 before it is encoded.  cons_chars() restates that; it
reproduces every PP_cons character of the (b) fixtures, and WH_MSA_CONS_HMMER computes it on the
device."""
import functools
import gzip
import json
import math
import os

import numpy as np

from tests import domains_reference as dr
from tests import msa_reference as mr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hits_msa")
MODELS = {"amino_hmmbuild": [0, 1, 2, 3], "dna_hmmbuild": [0, 1, 2], "amino_multidomain": [0]}


@functools.lru_cache(maxsize=None)
def load_fixture(name):
    with gzip.open(os.path.join(GOLDEN, name + ".json.gz"), "rt") as f:
        return json.load(f)


def encode(p):
    """HMMER's p7_alidisplay_EncodePostProb on a float32 value: the arithmetic in double."""
    p = float(np.float32(p))
    return "*" if p + 0.05 >= 1.0 else mr.CHARS[min(9, max(0, int(p * 10.0 + 0.5)))]


def quantise(pp):
    """float32 posteriors -> what HMMER keeps for a row of -A: '*' -> 1.0, digit d -> (float)d / 10."""
    p = np.asarray(pp, dtype=np.float32).astype(np.float64)
    d = np.clip((p * 10.0 + 0.5).astype(np.int64), 0, 9).astype(np.float32) / np.float32(10.0)
    return np.where(p + 0.05 >= 1.0, np.float32(1.0), d).astype(np.float32)


def cons_chars(M, cols, pps, matmap, W):
    """PP_cons as HMMER computes it: float32 values, double sum in row order, / (float) n in double, rounded to float32."""
    s, n = np.zeros(M, dtype=np.float64), np.zeros(M, dtype=np.int64)
    for c, p in zip(cols, pps):
        c = np.asarray(c)
        m = (c >= 0) & (c < M)
        s[c[m]] += np.asarray(p, dtype=np.float32)[m].astype(np.float64)       # (a row has one residue per node at most)
        n[c[m]] += 1
    out = np.full(W, ord("."), dtype=np.uint8)
    for k in range(M):
        if n[k]:
            out[matmap[k]] = ord(encode(np.float32(s[k] / float(np.float32(n[k])))))
    return out


def tie_columns(M, cols, pps):
    """Nodes whose exact mean of decoded tenths lies on a character boundary ((mean + 0.05) * 10 is an integer)."""
    s, n = np.zeros(M, dtype=np.int64), np.zeros(M, dtype=np.int64)
    for c, p in zip(cols, pps):
        c = np.asarray(c)
        m = (c >= 0) & (c < M)
        s[c[m]] += np.rint(np.asarray(p, dtype=np.float64)[m] * 10.0).astype(np.int64)
        n[c[m]] += 1
    return [k for k in range(M) if n[k] and (2 * s[k] + n[k]) % (2 * n[k]) == 0]


def select(order, seq_lnp, doms, ln_inc_seq, ln_inc_dom):
    """The rows of the alignment: [(query, index within the pair, ali_i, ali_j, record)] over the queries in <order>, a
    query's domains in domain order.  seq_lnp[q]: the sequence's ln P (None: not reported); doms[q]: its records."""
    rows = []
    for q in order:
        if seq_lnp[q] is None or not (seq_lnp[q] != seq_lnp[q] or seq_lnp[q] <= ln_inc_seq):
            continue
        for d in doms[q]:
            lnp = float(d["lnP"])
            if int(d["ali_i"]) != 0 and (lnp != lnp or lnp <= ln_inc_dom):
                rows.append((q, int(d["index"]), int(d["ali_i"]), int(d["ali_j"]), d))
    return rows


def ln_thr(thr, n):
    return math.log(thr / n) if thr > 0 else -math.inf


def assemble_rows(M, rows, texts, hmmer_cons=True):
    """rows of select() whose records carry "cols" / "pp" of the envelope; texts[q]: the query's characters."""
    cols, pps, tx = [], [], []
    for q, _, ai, aj, d in rows:
        i0, i1 = ai - int(d["env_i"]), aj - int(d["env_i"]) + 1
        cols.append(np.asarray(d["cols"][i0:i1], dtype=np.int32))
        pps.append(quantise(np.asarray(d["pp"][i0:i1], dtype=np.float32)))
        tx.append(texts[q][ai - 1:aj])
    m = mr.assemble(M, cols, pps, tx)
    if hmmer_cons:
        m["pp_cons"] = cons_chars(M, cols, pps, m["matmap"], m["W"])
    m["row_recs"] = [r[:4] for r in rows]
    m["cols"], m["pps"] = cols, pps
    return m


@functools.lru_cache(maxsize=None)
def case_scores(name, h):
    """Per query of the domains fixture <name>: the oracle's float32 sequence score on model h, None where not reported."""
    from oracle import oracle as orc
    from tests.conftest import load_case
    case = load_case(name)
    seqs, _ = dr.case_reference(name)
    ohm = orc.OracleHMM(case.hmm_paths[h])
    out = []
    for s in seqs:
        r = ohm.score(s)
        out.append((float(r.seq_score), float(r.pre_score), int(r.decibits), int(r.nenv)) if r.flags & 1 else None)
    return out


def reference(name, h, keep=None, incE=0.01, incdomE=0.01, descriptions=None, notextw=False):
    """The recipe for model h of case <name> on the queries <keep> (indices; None: all of the domains fixture's):
    (file text, assembled dict, names of the kept queries)."""
    from tests.conftest import load_case
    from witch_amd.shim import formats
    case = load_case(name)
    seqs, dom = dr.case_reference(name)
    keep = list(range(len(seqs))) if keep is None else list(keep)
    hdr = formats.hmm_header(case.hmm_paths[h])
    sc = case_scores(name, h)
    names = [case.qnames[q] for q in keep]
    rows = [(case.qnames[q], sc[q][2] / 10.0, 0.0, sc[q][3], sc[q][0]) for q in keep if sc[q] is not None]
    at = {case.qnames[q]: i for i, q in enumerate(keep)}
    order = [at[r[0]] for r in formats.hit_order(rows, hdr)]
    lnp = [None if sc[q] is None else formats.ln_survival(sc[q][0], hdr["ftau"], hdr["flambda"]) for q in keep]
    picked = select(order, lnp, [dom[(q, h)] for q in keep], ln_thr(incE, len(keep)), ln_thr(incdomE, max(len(rows), 1)))
    m = assemble_rows(hdr["M"], picked, [case.qseqs[q] for q in keep])
    text = formats.format_hits_msa(names, m["row_recs"], m["rows"], m["pp_rows"], m["pp_cons"], m["rf"], descriptions=descriptions,
                                   notextw=notextw)
    return text, m, names


def parse_gs(text):
    """The row names of a -A file in order, and {row name: DE text}."""
    names, desc = [], {}
    for line in text.splitlines():
        if line.startswith("#=GS"):
            w = line.split(None, 3)
            names.append(w[1])
            desc[w[1]] = w[3] if len(w) > 3 else ""
    return names, desc


def match_and_inserts(row, rf):
    """A row as (its characters on the match columns, its insert residues in order): what does not depend on the other rows."""
    return "".join(c for c, r in zip(row, rf) if r == "x"), "".join(c for c, r in zip(row, rf) if r != "x" and c != ".")
