"""Reference of hmmsearch's alignment display (wh_domain_display) in plain Python / numpy, and the readers of the fixtures
under tests/golden/display (tests/golden/make_golden_display.py).  Pure CPU.

Per reportable domain the four lines under "== domain N", one character per alignment column from the first match state to
the last (HMMER 3.1b2's p7_alidisplay_Create):
  match state   model: the node's consensus letter as the file prints it; target: the alphabet's symbol of the residue's
                digital code, upper case; match line: the consensus letter where the residue's code is the letter's code,
                else '+' where the float32 match odds of the residue at the node exceed 1.0, else ' '
  insert state  model '.', match line ' ', target: the symbol in lower case
  delete state  model: the consensus letter, match line ' ', target '-', PP '.'
  PP            p7_alidisplay_EncodePostProb of the float32 posterior, in double: '*' where p + 0.05 >= 1.0, else the digit
                (int)((p + 0.05) * 10.0)
render() applies that to ONE domain's arrays, display() to the arrays of a whole call in the layout of
EHMM.domain_display; case_section() composes the oracle's domain records (tests/domains_reference.case_reference) and
formats.format_hmmsearch into the section the binary prints."""
import functools
import gzip
import json
import math
import os

import numpy as np

from tests import domains_reference as dr
from tests import hits_msa_reference as hr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "display")
MODELS = hr.MODELS
SYMBOLS = {2: "ACDEFGHIKLMNPQRSTVWY-BJZOUX*~", 0: "ACGT-RYMKSWHBVDN*~", 1: "ACGU-RYMKSWHBVDN*~"}
EXTRA_RUNS = {"notextw": ["--notextw"], "textw150": ["--textw", "150"], "domE": ["--domE", "1e-10"]}


@functools.lru_cache(maxsize=None)
def load_fixture(name):
    with gzip.open(os.path.join(GOLDEN, name + ".json.gz"), "rt") as f:
        return json.load(f)


def consensus_column(path):
    """(the CONS column of a HMMER3 text model as a str of M letters or None, {"CONS", "RF", "CS": bool}) read from the file."""
    keys, K, cons, body = {"CONS": False, "RF": False, "CS": False}, None, [], False
    with open(path) as f:
        lines = f.read().splitlines()
    for n, line in enumerate(lines):
        w = line.split()
        if not w:
            continue
        if not body:
            if w[0] in keys and len(w) > 1:
                keys[w[0]] = w[1] == "yes"
            elif w[0] == "HMM":
                K, body = len(w) - 1, True
        elif w[0].isdigit() and len(w) >= K + 3 and len(cons) + 1 == int(w[0]):
            cons.append(w[K + 2])
    return ("".join(cons) if keys["CONS"] else None), keys


class DisplayModel:
    """What the display reads of a model: consensus letters and their codes [M + 1], float32 match odds [Kp, M + 1]."""

    def __init__(self, M, alphabet, cons, odds):
        self.M, self.alphabet, self.sym = int(M), int(alphabet), SYMBOLS[int(alphabet)]
        self.Kp = len(self.sym)
        self.cons = " " + cons
        at = {c: i for i, c in enumerate(SYMBOLS[0 if alphabet == 1 else alphabet])}
        self.code = np.array([255] + [at.get(c.upper(), 255) for c in cons], dtype=np.int64)
        self.odds = np.asarray(odds, dtype=np.float64).astype(np.float32)

    @classmethod
    @functools.lru_cache(maxsize=None)
    def from_path(cls, path):
        from oracle import oracle as orc
        ohm = orc.OracleHMM(path)
        cons, _ = consensus_column(path)
        return cls(ohm.M, ohm.alphabet, cons, ohm.odds)


def pp_char(p):
    x = float(np.float32(p)) + 0.05
    return "*" if x >= 1.0 else chr(ord("0") + min(9, max(0, int(x * 10.0))))


def render(model, dsq, rec, cols, pp):
    """The four lines of one domain.  dsq: the query's residue codes; rec: env_i, ali_i, ali_j, hmm_i (1-based); cols / pp:
    the envelope's per-residue 0-based node (-1: none) and posterior."""
    ei, ai, aj = int(rec["env_i"]), int(rec["ali_i"]), int(rec["ali_j"])
    mo, ml, aq, pl = [], [], [], []
    prev = int(rec["hmm_i"]) - 2
    for r in range(ai, aj + 1):
        x, node, p = int(dsq[r - 1]), int(cols[r - ei]), pp[r - ei]
        if node >= 0:
            for k in range(prev + 2, node + 1):                       # delete states, 1-based nodes
                mo.append(model.cons[k]); ml.append(" "); aq.append("-"); pl.append(".")
            k = node + 1
            mo.append(model.cons[k])
            ml.append(model.cons[k] if x == model.code[k] else "+" if model.odds[x, k] > np.float32(1.0) else " ")
            aq.append(model.sym[x])
            prev = node
        else:
            mo.append("."); ml.append(" "); aq.append(model.sym[x].lower())
        pl.append(pp_char(p))
    return "".join(mo), "".join(ml), "".join(aq), "".join(pl)


def envelope_posteriors(pmodel, sub, cols, L):
    """float64 posteriors of an envelope's residues along its path under the unihit length model of the WHOLE sequence's L
    residues.  That is what hmmsearch decodes a domain with: it configures the profile once for the sequence and keeps that
    configuration for every envelope, whereas tests/pp_reference.path_posteriors (hmmalign on the envelope alone, and
    wh_align_pp) uses the envelope's own length.  The two differ where the envelope is much shorter than its sequence (the
    chimeras of the fixtures: up to 0.045 on a weak domain, 0.0125 on one HMMER prints with acc 0.95), always towards a lower
    posterior in hmmsearch."""
    from tests import pp_reference as ppr
    sub = np.ascontiguousarray(np.minimum(np.asarray(sub, dtype=np.int64), pmodel.Kp - 1), dtype=np.uint8)
    out = np.zeros(len(sub), dtype=np.float64)
    ps = ppr.path_states(cols)
    if ps is None or len(sub) == 0:
        return out
    st, kk = np.ascontiguousarray(ps[0], dtype=np.int32), np.ascontiguousarray(ps[1], dtype=np.int32)
    loop, move = ppr.len_config(L)
    ppr.lib().ppref_path(pmodel.M, pmodel.pt.ctypes.data, pmodel.odds.ctypes.data, pmodel.entry.ctypes.data, sub.ctypes.data, len(sub),
                         loop, move, st.ctypes.data, kk.ctypes.data, out.ctypes.data)
    return out


def ln_thr(thr, n):
    return math.log(thr / n) if thr > 0 else -math.inf


def display(model, seqs, flags, dom, dom_off, env_off, cols, pp, H, h, domE, domZ):
    """The arrays of a call -> what EHMM.domain_display returns.  seqs: residue-code arrays per query; flags [nq * H]; dom: the
    wh_domain records (structured array or list of dicts); the envelope CSR with its columns and posteriors."""
    thr = ln_thr(domE, domZ)
    flags = np.asarray(flags).reshape(-1)
    recs, lines, off = [], [[], [], [], []], [0]
    for d in range(len(dom)):
        r = dom[d]
        p = int(r["pair"])
        lnp = float(r["lnP"])
        if p % H != h or not (flags[p] & 1) or int(r["ali_i"]) == 0 or not (lnp != lnp or lnp <= thr):
            continue
        a, b = int(env_off[d]), int(env_off[d + 1])
        four = render(model, seqs[p // H], r, cols[a:b], pp[a:b])
        for t in range(4):
            lines[t].append(four[t])
        recs.append((p // H, int(r["index"])))
        off.append(off[-1] + len(four[0]))
    text = ["".join(x).encode("ascii") for x in lines]
    return {"nsel": len(recs), "disp_off": np.array(off, dtype=np.int64),
            "recs": np.array(recs, dtype=np.dtype([("query", "<i4"), ("index", "<i4")])),
            "model": np.frombuffer(text[0], dtype=np.uint8), "match": np.frombuffer(text[1], dtype=np.uint8),
            "target": np.frombuffer(text[2], dtype=np.uint8), "pp": np.frombuffer(text[3], dtype=np.uint8)}


def same(got, want):
    """None where two display dicts are equal byte for byte, else what differs first."""
    if int(got["nsel"]) != int(want["nsel"]):
        return "nsel %d != %d" % (got["nsel"], want["nsel"])
    if not np.array_equal(got["disp_off"], want["disp_off"]):
        return "disp_off differs"
    if [tuple(int(x) for x in r) for r in got["recs"]] != [tuple(int(x) for x in r) for r in want["recs"]]:
        return "records differ"
    for k in ("model", "match", "target", "pp"):
        if not np.array_equal(got[k], want[k]):
            i = int(np.nonzero(np.asarray(got[k]) != np.asarray(want[k]))[0][0]) if len(got[k]) == len(want[k]) else -1
            return "%s line differs (first at byte %d)" % (k, i)
    return None


# ------------------------------------------------------------------------------------------------ the printed section
def section(text):
    """The "Domain annotation" section of a main output: its lines from the title up to the pipeline summary."""
    lines = text.splitlines()
    a = next(i for i, ln in enumerate(lines) if ln.startswith("Domain annotation for each sequence"))
    b = next(i for i, ln in enumerate(lines) if ln.startswith("Internal pipeline statistics"))
    while b > a and lines[b - 1] == "":
        b -= 1
    return lines[a:b]


def parse_section(lines):
    """(title, {name: {"table": [lines], "acc": {domain number: acc}, "domains": {number: [header + alignment lines]}}}, names
    in order)."""
    out, order, cur, dom = {}, [], None, None
    for ln in lines[1:]:
        if ln.startswith(">> "):
            cur = {"table": [], "acc": {}, "domains": {}}
            out[ln[3:].strip()] = cur
            order.append(ln[3:].strip())
            dom = None
        elif cur is None:
            continue
        elif ln.startswith("  == domain "):
            dom = []
            cur["domains"][int(ln.split()[2])] = dom
            dom.append(ln)
        elif dom is not None:
            dom.append(ln)
        elif ln.startswith("  Alignments for each domain:"):
            dom = []                                                   # (discarded: the next header starts a list)
        else:
            cur["table"].append(ln)
            w = ln.split()
            if len(w) >= 16 and w[0].isdigit() and w[1] in "!?":
                cur["acc"][int(w[0])] = float(w[-1])
    for v in out.values():
        for d in v["domains"].values():
            while d and d[-1] == "":
                d.pop()
    return lines[0], out, order


@functools.lru_cache(maxsize=None)
def case_section(name, h, domE=10.0, textw=120):
    """The section for model h of case <name> over the queries of the domains fixture, from the oracle's records and the
    shim's formatter: its lines.  The PP line is that of hmmsearch's own decoding (envelope_posteriors)."""
    from oracle import oracle as orc
    from tests import pp_reference as ppr
    from tests.conftest import load_case
    from witch_amd.shim import formats
    case = load_case(name)
    seqs, dom = dr.case_reference(name)
    nq = len(seqs)
    hdr = formats.hmm_header(case.hmm_paths[h])
    sc = hr.case_scores(name, h)
    model = DisplayModel.from_path(case.hmm_paths[h])
    pmodel = ppr.Model(orc.OracleHMM(case.hmm_paths[h]))
    rows = [(case.qnames[q], sc[q][2] / 10.0, max(0.0, sc[q][1] - sc[q][0]), sc[q][3], sc[q][0]) for q in range(nq) if sc[q] is not None]
    domains, lines = {}, {}
    thr = ln_thr(domE, max(len(rows), 1))
    for q in range(nq):
        if sc[q] is None or not dom[(q, h)]:
            continue
        domains[case.qnames[q]] = dom[(q, h)]
        for d in dom[(q, h)]:
            lnp = float(d["lnP"])
            if int(d["ali_i"]) != 0 and (lnp != lnp or lnp <= thr):
                pp = envelope_posteriors(pmodel, seqs[q][int(d["env_i"]) - 1:int(d["env_j"])], d["cols"], len(seqs[q]))
                lines.setdefault(case.qnames[q], {})[int(d["index"])] = render(model, seqs[q], d, d["cols"], pp)
    text = formats.format_hmmsearch(case.hmm_paths[h], "queries.fasta", hdr, rows, nq, domains=domains,
                                    lengths={case.qnames[q]: len(seqs[q]) for q in range(nq)}, domE=domE,
                                    display={"lines": lines, "textw": textw})
    return section(text)


def differing_domains(ref_lines, bin_lines):
    """[[name, domain number]] on which two sections differ in a domain's alignment lines (what follows its "== domain"
    header: the four lines of every block with their names and coordinates), or which only one of them has."""
    _, a, _ = parse_section(ref_lines)
    _, b, _ = parse_section(bin_lines)
    out = []
    for name in sorted(set(a) | set(b)):
        da, db = a.get(name, {"domains": {}})["domains"], b.get(name, {"domains": {}})["domains"]
        for n in sorted(set(da) | set(db)):
            if n not in da or n not in db or da[n][1:] != db[n][1:]:
                out.append([name, n])
    return out
