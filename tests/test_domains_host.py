"""Per-domain results, host side (no GPU): the float64 reference of tests/domains_reference.py against hmmsearch's own
--domtblout lines (tests/golden/domains), the text formats of the shim, and the parts of the C ABI that need no device.

A domain's alignment is DEFINED as wh_align's (hmmalign's) alignment of the envelope.  On the domains HMMER prints with an
accuracy of 0.95 or more that is hmmsearch's printed alignment, coordinate for coordinate, and the conditions are asserted;
on weaker ones hmmsearch usually prints it with columns trimmed at an end (its rule is not in the reference), so the
agreement there is counted and printed, not asserted - only the score and bias columns are.

Measured here (reference against fixture):
  case               strong  coords differ  acc within 0.00501  |  weak  coords differ  acc within 0.00501
  dna_hmmbuild          178        0              178            |   238       29              201
  amino_hmmbuild        100        0               99            |    90       13               74
  amino_multidomain      60        0               60            |     3        1                3
Score and bias (domains_reference.compare_with_fixture): every strong-stratum domain, multidomain region or not, and every
weak one of a region HMMER does not flag multidomain, under the print-boundary rule - equal as printed or one unit apart within
0.002 bit of a "%.1f" boundary; one field differs, inside it (67.65013 vs 67.6, strong).  Weak envelopes of multidomain regions
alone (dna_hmmbuild 57, amino_hmmbuild 14, amino_multidomain 3), whose null2 correction HMMER averages over 200 sampled traces,
follow the multidomain class of tests/test_oracle_golden.py (up to two printed units, on at most max(1, 4 %) of the class, two
units on at most 1 %): two of dna_hmmbuild differ, one unit each - rnd01 x A_0_4, 0.55173 against HMMER's 0.5, and rnd03 x A_0_5,
envelope 5-60 of 90 residues, -1.35211 against HMMER's -1.3 (0.00211 bit from the boundary: sampling noise of the class).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import domains_reference as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def strata():
    """compare_with_fixture of every case, once per module."""
    out = {}
    for name in dr.CASES:
        _, dom = dr.case_reference(name)
        out[name] = dr.compare_with_fixture(name, dom)
    return out


def test_reference_strong_stratum(strata):
    """Envelope lists equal both ways on every pair, "#" / "of", identical coordinates and acc within 0.0151 on every strong
    domain (asserted inside compare_with_fixture); score and bias of EVERY strong domain under the print-boundary rule; acc within 0.00501 on at
    least 99 % of the strong domains."""
    n = sum(st["strong"] for st in strata.values())
    close = sum(st["strong_acc_5e3"] for st in strata.values())
    misses = [m for st in strata.values() for m in st["strong_rule_misses"]]
    print("strong stratum: %d domains, acc within 0.00501 on %d" % (n, close))
    assert n >= 300
    assert not misses, misses
    assert close >= 0.99 * n, (close, n)


@pytest.mark.parametrize("name", dr.CASES)
def test_weak_stratum_scores(strata, name):
    """HMMER acc < 0.95: score and bias under the same print-boundary rule, except envelopes of multidomain regions, which follow
    the multidomain class of tests/test_oracle_golden.py with its caps; the coordinate and acc agreement is printed by
    compare_with_fixture and not asserted."""
    st = strata[name]
    assert st["weak"] > 0
    assert not st["weak_rule_misses"], st["weak_rule_misses"]
    assert dr.multi_class_ok(st), (st["multi"], st["multi_differ"], st["multi_two"])


# ------------------------------------------------------------------------------------------------ formats
def _numbers(ln):
    from witch_amd.shim.formats import DOMTBL_COLUMNS
    text = {"target", "tacc", "query", "qacc"}
    ints = {"tlen", "qlen", "num", "of", "hmm_from", "hmm_to", "ali_from", "ali_to", "env_from", "env_to"}
    return {k: ln[k] if k in text else int(ln[k]) if k in ints else float(ln[k]) for k in DOMTBL_COLUMNS}


@pytest.mark.parametrize("name", dr.CASES)
def test_domtblout_lines_reproduce_hmmer(name):
    """format_domtblout_lines on the fixture's own numbers gives HMMER's raw lines byte for byte, and the header lines."""
    from witch_amd.shim import formats
    n = 0
    for m in dr.load_fixture(name)["models"]:
        entries = [_numbers(ln) for ln in m["lines"]]
        widths = formats._domtbl_widths(entries)
        assert formats.format_domtblout_header(widths) == m["header"]
        assert formats.format_domtblout_lines(entries) == [ln["raw"] for ln in m["lines"]]
        n += len(entries)
    assert n > 0


def _reference_rows(name, h):
    """(hdr, rows, lengths, domains) of model h of a case as the GPU backend would return them, from the oracle."""
    from oracle import oracle as orc
    from tests.conftest import load_case
    from witch_amd.shim import formats
    case = load_case(name)
    fx = dr.load_fixture(name)
    seqs, dom = dr.case_reference(name)
    ohm = orc.OracleHMM(case.hmm_paths[h])
    hdr = formats.hmm_header(case.hmm_paths[h])
    rows, lengths, domains = [], {}, {}
    for q, qn in enumerate(fx["queries"]):
        lengths[qn] = len(seqs[q])
        r = ohm.score(seqs[q])
        if r.flags & 1:
            rows.append((qn, r.decibits / 10.0, max(0.0, float(r.pre_score) - float(r.seq_score)), int(r.nenv), float(r.seq_score)))
            domains[qn] = dom[(q, h)]
    return hdr, rows, lengths, domains


def test_evalues_domE_Z_and_domZ_against_the_fixture(tmp_path):
    """The whole file from reference records: Z and domZ default to the fixture's (targets, reported sequences), the lines
    HMMER lists are the reportable ones, and every line whose fields all agree with HMMER's is byte-identical to HMMER's
    (most are; the others differ in a printed digit of an E-value, a score at a print boundary or a weak domain's
    alignment).  --domE, -Z and --domZ filter and scale as HMMER's do."""
    from witch_amd.shim import formats
    name, h = "dna_hmmbuild", 0
    m = dr.load_fixture(name)["models"][h]
    hdr, rows, lengths, domains = _reference_rows(name, h)
    assert (len(lengths), len(rows)) == (m["Z"], m["domZ"])
    text = formats.format_domtblout("m.hmm", "q.fa", hdr, rows, lengths, domains, len(lengths))
    lines = text.splitlines()
    assert lines[:3] == m["header"]
    body = [ln for ln in lines if not ln.startswith("#")]
    raw = [ln["raw"] for ln in m["lines"]]
    n, same, boundary, weak, weak_same = dr.check_strong_lines(body, m["lines"])
    assert n > 0 and same + boundary == n and boundary <= max(1, n // 20)
    for b, r in zip(body, raw):          # E-values of every line, weak ones included: HMMER's printed digits
        for col in (6, 11, 12):
            got, want = float(b.split()[col]), float(r.split()[col])
            assert want == 0 or 0.9 < got / want < 1.1, (b, r)
    tail = [ln for ln in lines[3 + len(body):]]
    assert [t for t in tail if not t.startswith(("# Query file", "# Target file"))] == m["trailer"]
    # --domE keeps c-Evalue <= domE; "#" and "of" still count all domains
    strict = formats.format_domtblout("m.hmm", "q.fa", hdr, rows, lengths, domains, len(lengths), domE=1e-5)
    kept = [ln for ln in strict.splitlines() if not ln.startswith("#")]
    assert 0 < len(kept) < len(body) and all(float(k.split()[11]) <= 1e-5 for k in kept)
    assert set(kept) <= set(body)
    # -Z scales the full-sequence and independent E-values, --domZ the conditional one
    z2 = formats.format_domtblout("m.hmm", "q.fa", hdr, rows, lengths, domains, len(lengths), Z=2 * m["Z"], domZ=m["domZ"])
    e1 = formats.domain_entries(hdr, rows, lengths, domains, len(lengths))
    e2 = formats.domain_entries(hdr, rows, lengths, domains, len(lengths), Z=2 * m["Z"], domZ=3 * m["domZ"])
    for a, b in zip(e1, e2):
        assert b["i_evalue"] == pytest.approx(2 * a["i_evalue"]) and b["evalue"] == pytest.approx(2 * a["evalue"])
        assert b["c_evalue"] == pytest.approx(3 * a["c_evalue"])
    assert z2 != text


def test_domain_tables_of_the_main_output():
    """format_hmmsearch(domains=...) appends HMMER's ">> name" tables: on the fixture's own numbers they are HMMER's lines."""
    from witch_amd.shim import formats
    name, h = "dna_hmmbuild", 0
    m = dr.load_fixture(name)["models"][h]
    hdr, rows, lengths, domains = _reference_rows(name, h)
    by = {}
    for ln in m["lines"]:
        e = _numbers(ln)
        e["reportable"] = True
        e["included"] = None
        by.setdefault(ln["target"], []).append(e)
    n = 0
    for qn, want in m["tables"].items():
        entries = by.get(qn, [])
        for t, e in enumerate(entries):
            e["included"] = want[3 + t][5] == "!"
        got = formats.format_domain_table(qn, entries, hdr["M"], lengths[qn])
        assert got[:-1] == want and got[-1] == "", (qn, got, want)
        n += 1
    assert n == len(rows)
    text = formats.format_hmmsearch("m.hmm", "q.fa", hdr, rows, len(lengths), domains=domains, lengths=lengths)
    assert "Domain annotation for each sequence:" in text and text.count("\n>> ") == len(rows)
    # the '!' / '?' marks and the reportable count N follow the E-values
    for qn, want in m["tables"].items():
        sect = text.split(">> %s  \n" % qn)[1].split("\n\n")[0].splitlines()
        assert len(sect) == len(want) - 1, (qn, sect, want)
        assert [ln[5] for ln in sect[2:]] == [ln[5] for ln in want[3:]], qn


def test_format_hmmsearch_without_domains_is_unchanged(tmp_path):
    """Without domains= the output is byte for byte what it was (the inputs of tests/test_shim_host.py)."""
    import hashlib
    from witch_amd.shim import formats
    p = tmp_path / "m.hmm"
    p.write_text("HMMER3/f [3.1b2 | February 2015]\nNAME  A_0_7\nLENG  12\nALPH  DNA\n"
                 "STATS LOCAL MSV      -9.0 0.71\nSTATS LOCAL VITERBI -9.5 0.71\nSTATS LOCAL FORWARD  -4.2 0.71\nHMM  A C G T\n")
    hdr = formats.hmm_header(str(p))
    rows = [("q1", 123.4, 0.3, 1), ("a_long_query_name_with_many_chars", -5.2, 0.0, 2), ("q3", 7.0, 11.1, 1)]
    text = formats.format_hmmsearch("m.hmm", "q.fa", hdr, rows, 3)
    assert hashlib.sha256(text.encode()).hexdigest() == "3530249d5bd61a8ee952d18223af96f6bf79322b892e7c73bd0dcbb9af9d32a9"
    assert hashlib.sha256(formats.format_hmmsearch("m.hmm", "q.fa", hdr, [], 3).encode()).hexdigest() == "7f18adfd3a4e9dc508bb63f649dcb41b97f76a2a5b376c9334215fef6787dcb1"
    assert "Domain annotation" not in text and ">>" not in text


def test_server_writes_domtblout_only_when_asked(tmp_path):
    """run_hmmsearch with --domtblout asks the backend for domains and writes the file; without it the backend is called as
    before (two arguments: a backend that knows nothing of domains still serves) and the output is today's."""
    from witch_amd.shim import formats
    from witch_amd.shim.server import Server, check_hmmsearch_options, parse_hmmsearch_argv, ArgError
    calls = []

    class Backend:
        def search(self, hmm_path, records, **kw):
            calls.append(kw)
            hdr = formats.hmm_header(hmm_path)
            rows = [(n, 20.5, 0.1, 1) for n, _ in records]
            doms = {n: [{"index": 0, "of": 1, "env_i": 1, "env_j": len(t), "ali_i": 2, "ali_j": len(t), "hmm_i": 1, "hmm_j": 12,
                         "bits": 20.25, "bias_bits": 0.1, "oasc": 0.9 * len(t), "lnP": -17.0}] for n, t in records}
            return (hdr, rows, doms) if kw.get("want_domains") else (hdr, rows)

    (tmp_path / "m.hmm").write_text("HMMER3/f [3.1b2 | February 2015]\nNAME  A_0_7\nLENG  12\nALPH  DNA\n"
                                    "STATS LOCAL FORWARD  -4.2 0.71\nHMM  A C G T\n")
    (tmp_path / "q.fa").write_text(">q1\nACGTACGTAC\n>q2\nACGTTT\n")
    srv = Server.__new__(Server)
    srv.backend = Backend()
    plain = srv.run_hmmsearch("--max -E 99999999 m.hmm q.fa".split(), str(tmp_path))
    assert calls == [{}] and ">>" not in plain
    out = srv.run_hmmsearch("--max -E 99999999 --domtblout d.tbl m.hmm q.fa".split(), str(tmp_path))
    assert calls[1] == {"want_domains": True}
    body = [ln for ln in open(tmp_path / "d.tbl") if not ln.startswith("#")]
    assert len(body) == 2 and body[0].split()[0] == "q1" and body[0].split()[13] == "20.2" and body[0].split()[21] == "0.90"
    assert out.count("\n>> ") == 2 and plain.split("Domain annotation")[0].splitlines()[:12] == out.splitlines()[:12]
    srv.run_hmmsearch("--max -E 99999999 --domE 1e-30 --domtblout d.tbl m.hmm q.fa".split(), str(tmp_path))
    assert not [ln for ln in open(tmp_path / "d.tbl") if not ln.startswith("#")]
    for bad in ("--max --domE x m q", "--max --domtblout d -Z 0 m q", "--max --domtblout d --domZ -3 m q"):
        with pytest.raises(ArgError):
            check_hmmsearch_options(parse_hmmsearch_argv(bad.split())[0])
    for unread in ("--max -Z 0 m q", "--max --domZ x m q"):          # without --domtblout they are not read, as before
        check_hmmsearch_options(parse_hmmsearch_argv(unread.split())[0])
    # --incE / --incdomE decide the '!' / '?' marks of the domain tables
    marks = lambda text: [ln[5] for ln in text.splitlines() if ln[:5].strip().isdigit() and ln[4:7] in (" ! ", " ? ")]
    assert marks(out) == ["!", "!"]
    strict = srv.run_hmmsearch("--max -E 99999999 --incdomE 1e-30 --domtblout d.tbl m.hmm q.fa".split(), str(tmp_path))
    assert marks(strict) == ["?", "?"]


# ------------------------------------------------------------------------------------------------ ABI without a device
def test_evparams_parser_with_and_without_the_stats_line(tmp_path):
    from tests.conftest import load_case
    from witch_amd import _lib
    from witch_amd.shim import formats
    L = _lib.lib()
    tau, lam, present = C.c_float(0), C.c_float(0), C.c_int32(-1)
    path = load_case("dna_hmmbuild").hmm_paths[0]
    assert L.wh_hmm_evparams(path.encode(), C.byref(tau), C.byref(lam), C.byref(present)) == 0
    hdr = formats.hmm_header(path)
    assert present.value == 1 and tau.value == np.float32(hdr["ftau"]) and lam.value == np.float32(hdr["flambda"])
    bare = tmp_path / "bare.hmm"
    bare.write_text("".join(ln for ln in open(path) if not ln.startswith("STATS")))
    assert L.wh_hmm_evparams(str(bare).encode(), C.byref(tau), C.byref(lam), C.byref(present)) == 0
    assert present.value == 0 and np.isnan(tau.value) and np.isnan(lam.value)
    assert L.wh_hmm_evparams(str(tmp_path / "missing.hmm").encode(), None, None, None) == _lib.WH_EIO
    assert L.wh_ehmm_evparams(None, None, None, None) == _lib.WH_EINVAL
    assert L.wh_domains(None, None, None, 0, None, None, None, None) == _lib.WH_EINVAL and b"wh_domains" in L.wh_last_error()
    assert L.wh_domain_counts(None, None, None, 0, None, None) == _lib.WH_EINVAL


def test_wh_domain_layout_matches_the_ctypes_and_numpy_mirrors(tmp_path):
    from witch_amd import _lib
    names = [f[0] for f in _lib.Domain._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "witch_hip.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(wh_domain));\n' +
                   "".join('  printf("%%zu\\n", offsetof(wh_domain, %s));\n' % n for n in names) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(_lib.Domain) == np.dtype(_lib.DOMAIN_FIELDS).itemsize == 56
    assert got[1:] == [getattr(_lib.Domain, n).offset for n in names]
    dt = np.dtype(_lib.DOMAIN_FIELDS)
    assert got[1:] == [dt.fields[n][1] for n in names] and list(dt.names) == names
