"""Reference for the per-domain records of wh_domains and the readers of the fixture tests/golden/domains
(tests/test_domains_host.py, tests/test_domains.py).  Pure CPU, float64.

A domain is an envelope of the scoring stage.  Its record is composed from pieces the tests already trust:
  envelopes, envsc, domcorr     oracle.OracleHMM.score on the whole query
  alignment                     oracle.OracleHMM.align on the envelope's residues (hmmalign's optimal-accuracy alignment under
                                the unihit length model of Ld = env_j - env_i + 1 residues)
  posteriors along that path    tests/pp_reference.path_posteriors
and HMMER's per-domain score arithmetic (L: query length):
  bits      = (envsc + (L - Ld) ln(L / (L + 3)) - nullsc - dombias) / ln 2,   nullsc = L ln(L / (L + 1)) + ln(1 / (L + 1))
  dombias   = logsum(0, ln(1 / 256) + domcorr)        (printed in bits)
  lnP       = min(0, -lambda (bits - tau))            (STATS LOCAL FORWARD tau lambda of the model file)
  acc       = oasc / Ld,  oasc = the sum of the path's posteriors over the envelope
"""
import functools
import gzip
import json
import math
import os

import numpy as np

from tests import pp_reference as ppr

_HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_DOM = os.path.join(_HERE, "golden", "domains")
CASES = ("dna_hmmbuild", "amino_hmmbuild", "amino_multidomain")
LN2 = math.log(2.0)


def domain_bits(envsc, domcorr, L, Ld):
    """(bits, bias_bits) of a domain, float64."""
    nullsc = L * math.log(L / (L + 1.0)) + math.log(1.0 / (L + 1.0))
    dombias = np.logaddexp(0.0, math.log(1.0 / 256.0) + domcorr)
    bits = (envsc + (L - Ld) * math.log(L / (L + 3.0)) - nullsc - dombias) / LN2
    return float(bits), float(dombias / LN2)


def ln_p(bits, tau, lam):
    return float("nan") if tau is None or lam is None else min(0.0, -lam * (bits - tau))


def pair_domains(ohm, model, dsq, evparams=(None, None), max_list=None):
    """The domain records of one (query, model) pair, in envelope order: dicts with the fields of wh_domain (float64) plus
    "cols" / "pp", the envelope's alignment.  [] for a pair that is not reported.  max_list: list only the first so many."""
    r = ohm.score(dsq)
    if not (r.flags & 1):
        return []
    L, out = len(dsq), []
    for d in range(r.nenv if max_list is None else min(r.nenv, max_list)):
        ei, ej = int(r.env_i[d]), int(r.env_j[d])
        sub = np.ascontiguousarray(dsq[ei - 1:ej])
        Ld = ej - ei + 1
        cols = ohm.align(sub)
        pp = ppr.path_posteriors(model, sub, cols)
        hit = np.nonzero(cols >= 0)[0]
        bits, bias = domain_bits(float(r.envsc[d]), float(r.domcorr[d]), L, Ld)
        rec = {"index": d, "of": int(r.nenv), "env_i": ei, "env_j": ej,
               "ali_i": ei + int(hit[0]) if len(hit) else 0, "ali_j": ei + int(hit[-1]) if len(hit) else 0,
               "hmm_i": int(cols[hit[0]]) + 1 if len(hit) else 0, "hmm_j": int(cols[hit[-1]]) + 1 if len(hit) else 0,
               "bits": bits, "bias_bits": bias, "oasc": float(pp.sum()), "lnP": ln_p(bits, *evparams),
               "envsc": float(r.envsc[d]), "domcorr": float(r.domcorr[d]), "multi": bool(r.env_multi[d]), "cols": cols, "pp": pp}
        out.append(rec)
    return out


@functools.lru_cache(maxsize=None)
def load_fixture(name):
    """tests/golden/domains/<name>.json.gz (tests/golden/make_golden_domains.py)."""
    with gzip.open(os.path.join(GOLDEN_DOM, name + ".json.gz"), "rt") as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """For a fixture case: (queries' residue codes, {(q, h): [domain records]}) over the fixture's models and queries.
    Computed once per process and shared; callers do not modify it."""
    from oracle import oracle as orc
    from tests.conftest import load_case
    from witch_amd.shim.formats import hmm_header
    case = load_case(name)
    fx = load_fixture(name)
    nq = len(fx["queries"])
    assert fx["queries"] == case.qnames[:nq]
    dom = {}
    seqs = None
    for h, m in enumerate(fx["models"]):
        assert m["hmm_file"] == case.hmm_files[h]
        ohm = orc.OracleHMM(case.hmm_paths[h])
        if seqs is None:
            seqs = [ohm.digitize(s.upper()) for s in case.qseqs[:nq]]
        model = ppr.Model(ohm)
        hdr = hmm_header(case.hmm_paths[h])
        for q in range(nq):
            dom[(q, h)] = pair_domains(ohm, model, seqs[q], (hdr["ftau"], hdr["flambda"]))
    return seqs, dom


def fixture_domains(name):
    """{(q, h): [fixture line dicts in domain order]} of the listed (reportable) domains."""
    fx = load_fixture(name)
    qi = {n: i for i, n in enumerate(fx["queries"])}
    out = {}
    for h, m in enumerate(fx["models"]):
        for ln in m["lines"]:
            out.setdefault((qi[ln["target"]], h), []).append(ln)
    for v in out.values():
        v.sort(key=lambda ln: int(ln["num"]))
    return out


def print_boundary_ok(value, printed, slack=0.002):
    """The rule of tests/test_oracle_golden.py for a "%.1f" field: equal as printed, or one unit apart with the value within
    <slack> of a rounding boundary.  Returns (accepted, differs)."""
    want = int(round(float(printed) * 10))
    got = int(np.rint(value * 10.0))
    if got == want:
        return True, False
    return abs(got - want) == 1 and abs((abs(value) * 10.0) % 1.0 - 0.5) < slack * 10.0, True


def compare_with_fixture(name, dom, out=print, multi_from=None):
    """The conditions of the issue for records <dom> ({(q, h): [records]}) against HMMER's printed lines.  Asserted here:
    the envelope lists (equal both ways: HMMER lists the domains with c-Evalue <= --domE = 10), "#" and "of", and on the
    strong stratum (HMMER's acc >= 0.95) identical hmm / ali coordinates and acc within 0.0151.  Counted and returned:
    strong / weak domains, those with acc within 0.00501, weak ones whose coordinates differ, and per stratum the score /
    bias fields that differ as printed ("*_boundary": accepted by the print-boundary rule, "*_rule_misses": not).
    Score and bias: on EVERY strong-stratum domain, and on every weak one of a region HMMER does not flag multidomain, equal
    as printed or one unit apart within 0.002 bit of a print boundary (the single-domain rule of tests/test_oracle_golden.py).
    Only a WEAK-stratum envelope of a MULTIDOMAIN region (the record's "multi"; records without the field - the device's -
    take it from the reference records <multi_from>) follows that file's multidomain class instead: HMMER resolves the
    region by 200 seeded stochastic tracebacks, its null2 correction is the mean over those samples, and one sampled decision
    that flips in float rounding shifts the random stream of every later trace - there a field may differ by up to two
    printed units (more is a miss), on at most max(1, 4 %) of the class's weak domains, by two units on at most 1 %
    ("multi", "multi_differ", "multi_two": multi_class_ok).  Measured: two such fields, both of dna_hmmbuild, one unit each."""
    fxd = fixture_domains(name)
    dom_z = [m["domZ"] for m in load_fixture(name)["models"]]
    st = {"strong": 0, "weak": 0, "strong_acc_5e3": 0, "weak_acc_5e3": 0, "strong_boundary": 0, "weak_boundary": 0,
          "weak_coord_differ": 0, "strong_acc_worst": 0.0, "strong_rule_misses": [], "weak_rule_misses": [],
          "multi": 0, "multi_differ": 0, "multi_two": 0}
    for key in sorted(set(fxd) | set(dom)):
        lines = fxd.get(key, [])
        recs = [r for r in dom.get(key, []) if math.exp(r["lnP"]) * dom_z[key[1]] <= 10.0]
        env = [(int(r["env_i"]), int(r["env_j"])) for r in recs]
        want_env = [(int(ln["env_from"]), int(ln["env_to"])) for ln in lines]
        assert env == want_env, (name, key, env, want_env)
        for r, ln in zip(recs, lines):
            assert (r["index"] + 1, r["of"]) == (int(ln["num"]), int(ln["of"])), (name, key)
            stratum = "strong" if float(ln["acc"]) >= 0.95 else "weak"
            Ld = int(r["env_j"]) - int(r["env_i"]) + 1
            coords = tuple(int(r[k]) for k in ("hmm_i", "hmm_j", "ali_i", "ali_j"))
            want = (int(ln["hmm_from"]), int(ln["hmm_to"]), int(ln["ali_from"]), int(ln["ali_to"]))
            dacc = abs(float(r["oasc"]) / Ld - float(ln["acc"]))
            multi = stratum == "weak" and (r["multi"] if "multi" in r else multi_from[key][int(r["index"])]["multi"])
            units = 0
            for val, field in ((float(r["bits"]), "dom_score"), (float(r["bias_bits"]), "dom_bias")):
                ok, differs = print_boundary_ok(val, ln[field])
                if multi:
                    off = abs(int(np.rint(val * 10.0)) - int(round(float(ln[field]) * 10)))
                    units = max(units, off)
                    ok = off <= 2
                else:
                    st[stratum + "_boundary"] += differs and ok
                if not ok:
                    st[stratum + "_rule_misses"].append((name, key, int(r["index"]), field, val, ln[field]))
            st["multi"] += bool(multi)
            st["multi_differ"] += units >= 1
            st["multi_two"] += units >= 2
            st[stratum] += 1
            st[stratum + "_acc_5e3"] += dacc <= 0.00501
            if stratum == "strong":
                assert coords == want, (name, key, coords, want)
                assert dacc <= 0.0151, (name, key, float(r["oasc"]) / Ld, ln["acc"])
                st["strong_acc_worst"] = max(st["strong_acc_worst"], dacc)
            else:
                st["weak_coord_differ"] += coords != want
    out("[%s] strong stratum (HMMER acc >= 0.95): %d domains, hmm / ali coordinates identical, acc within 0.00501 on %d (worst "
        "%.4f), %d score / bias fields one unit off at a print boundary, %d beyond the rule; weak stratum: %d domains, coordinates "
        "differ on %d, acc within 0.00501 on %d, %d fields at a print boundary, %d beyond the rule; weak envelopes of multidomain "
        "regions: %d, score or bias differs as printed on %d, by two units on %d" %
        (name, st["strong"], st["strong_acc_5e3"], st["strong_acc_worst"], st["strong_boundary"], len(st["strong_rule_misses"]),
         st["weak"], st["weak_coord_differ"], st["weak_acc_5e3"], st["weak_boundary"], len(st["weak_rule_misses"]),
         st["multi"], st["multi_differ"], st["multi_two"]))
    return st


def multi_class_ok(st):
    """The caps of tests/test_oracle_golden.py on the multidomain class of one case (weak stratum only)."""
    return st["multi_differ"] <= max(1, st["multi"] // 25) and st["multi_two"] <= st["multi"] // 100


def check_strong_lines(body, fixture_lines, out=print):
    """--domtblout lines <body> against HMMER's: the same targets and envelopes in the same order, and every line of the
    strong stratum (HMMER's acc >= 0.95) byte-identical to HMMER's raw line - but for lines whose only difference is a print
    boundary (a score or bias one printed unit apart, an E-value that differs in its last printed digit), which are counted.
    Returns (strong lines, identical ones, print-boundary ones, weak lines, identical weak ones)."""
    assert [b.split()[0] for b in body] == [ln["target"] for ln in fixture_lines], "targets or their order differ"
    assert [b.split()[19:21] for b in body] == [[ln["env_from"], ln["env_to"]] for ln in fixture_lines]
    printed = {6: 2, 7: 1, 8: 1, 11: 2, 12: 2, 13: 1, 14: 1}          # column -> 1: "%.1f", 2: "%9.2g"
    n = same = boundary = weak = weak_same = 0
    for b, ln in zip(body, fixture_lines):
        r = ln["raw"]
        if float(ln["acc"]) < 0.95:
            weak += 1
            weak_same += b == r
            continue
        n += 1
        if b == r:
            same += 1
            continue
        bw, rw = b.split(), r.split()
        diff = [c for c in range(len(rw)) if bw[c] != rw[c]]
        assert len(bw) == len(rw) and all(c in printed for c in diff), (b, r)
        for c in diff:
            got, want = float(bw[c]), float(rw[c])
            if printed[c] == 1:
                assert abs(got - want) < 0.1001, (b, r)
            else:
                assert abs(got - want) <= 0.11 * 10 ** (math.floor(math.log10(abs(want))) - 1) * 10, (b, r)
        boundary += 1
    out("strong stratum: %d lines, %d byte-identical to HMMER's, %d differ at a print boundary only; weak stratum: %d lines, %d "
        "byte-identical" % (n, same, boundary, weak, weak_same))
    return n, same, boundary, weak, weak_same


# ------------------------------------------------------------------------------------------------ seeded synthetic cases
def shapes_case(outdir):
    """Two DNA models of about 120 nodes (witch_amd.synth; the second with its STATS lines taken out: lnP is NaN) and queries whose pairs meet the edges
    of the domain kernels, in this order: (model paths, names, residue-code arrays)
      none0      a 3-residue query: no pair of it has a domain (first pairs of the call)
      whole      a whole leaf: the envelope starts at residue 1 and ends at L, more than 64 residues
      none1      no domain, between domain-bearing pairs
      short      a 40-residue fragment: fewer than 64 residues (a partial lane trip)
      chimera    two windows from different places joined by a spacer: two envelopes
      tandem     two copies of a fragment back to back: a multidomain region, finished by the resolver
      none2      no domain (last pairs of the call)."""
    from witch_amd import synth
    fam = synth.make_family(9100, 120, 16, "dna", 0.04, 1e-3)
    eh = synth.make_ehmm(fam, 2, outdir, witch_layout=False)
    with open(eh.paths[1]) as f:
        kept = [ln for ln in f if not ln.startswith("STATS")]
    with open(eh.paths[1], "w") as f:
        f.writelines(kept)
    rng = np.random.default_rng(9101)
    leaf = fam.leaf_seq(3).astype(np.uint8)
    _, frags = synth.make_queries(fam, 9102, 4, 40)
    other = fam.leaf_seq(9).astype(np.uint8)
    spacer = rng.integers(0, 4, size=25).astype(np.uint8)
    chim = np.concatenate([other[70:110], spacer, other[5:45]])
    tandem = np.concatenate([frags[1].astype(np.uint8), frags[1].astype(np.uint8)])
    tiny = [np.array(t, dtype=np.uint8) for t in ([0, 1, 2], [3, 3, 0], [2, 0, 1])]
    names = ["none0", "whole", "none1", "short", "chimera", "tandem", "none2"]
    seqs = [tiny[0], leaf, tiny[1], frags[0].astype(np.uint8), chim, tandem, tiny[2]]
    return eh.paths, names, seqs


def long_list_case(outdir):
    """A variant of the generator of tests/tools/fuzz_long_list.py at its smallest size (18 fragments of 40 residues, one
    150-node DNA family, two models).  It DEVIATES from that generator: there a spacer of 15 to 60 residues follows a fragment
    with probability 0.85, which at this size merges fragments into 13 regions of 16 envelopes - no long-list pair; here a
    spacer of 40 to 60 random residues follows EVERY fragment, so that each is a region of its own with one envelope: 18
    regions and 18 envelopes on both models (oracle), more than a detail record lists, and a full count the device exports."""
    from witch_amd import synth
    rng = np.random.default_rng(70001)
    fam = synth.make_family(71001, 150, 16, "dna", 0.04, 1e-3)
    eh = synth.make_ehmm(fam, 2, outdir, witch_layout=False)
    _, frags = synth.make_queries(fam, 72001, 12, 40)
    parts = []
    for _ in range(18):
        parts.append(frags[int(rng.integers(0, len(frags)))].astype(np.uint8))
        parts.append(rng.integers(0, 4, size=int(rng.integers(40, 60))).astype(np.uint8))
    return eh.paths, ["long18", "frag"], [np.concatenate(parts), frags[0].astype(np.uint8)]


def reference_for(paths, seqs, max_list=None):
    """{(q, h): [records]} for seeded models and queries, and the oracle's (flags, nregions, nenv) per pair."""
    from oracle import oracle as orc
    from witch_amd.shim.formats import hmm_header
    dom, info = {}, {}
    for h, p in enumerate(paths):
        ohm = orc.OracleHMM(p)
        model = ppr.Model(ohm)
        hdr = hmm_header(p)
        for q, s in enumerate(seqs):
            r = ohm.score(s)
            info[(q, h)] = (int(r.flags), int(r.nregions), int(r.nenv))
            dom[(q, h)] = pair_domains(ohm, model, s, (hdr["ftau"], hdr["flambda"]), max_list)
    return dom, info
