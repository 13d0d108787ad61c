"""hmmsearch --tblout, host side (no GPU): the float64 replica of the counting sweep (wh_seq_expect_host), the text of the
table (witch_amd.shim.formats), the host half of the row assembly (wh_seq_table_host) and the shim's options, against the
per-sequence tables of the reference's bundled hmmsearch 3.1b2 (tests/golden/tblout, made by make_golden_tblout.py)."""
import math

import numpy as np
import pytest

from tests import tblout_common as tc


def _digitized(case):
    from tests.filters_common import digitize, pack
    alph = {"dna": 0, "rna": 1, "amino": 2}.get(case.alphabet, case.alphabet)
    seqs = [digitize(alph, s.upper()) for s in case.qseqs]
    return seqs, pack(seqs)


def _check_expect(name, got, rows):
    exempt = 0
    for g, r in zip(got, rows):
        assert (int(g["reg"]), int(g["clu"])) == (int(r["reg"]), int(r["clu"])), (name, r["raw"], g)
        ok, ex = tc.exp_ok(float(g["exp"]), r["exp"])
        assert ok, (name, r["raw"], g)
        exempt += ex
    assert exempt <= tc.EXEMPT_CAP * len(rows), (name, exempt, len(rows))
    print("[%s] %d rows: reg and clu equal, exp equal as printed but for %d rows at a print boundary" % (name, len(rows), exempt))


# ------------------------------------------------------------------------------------------------ 1. the host replica
@pytest.mark.parametrize("name", tc.CASES)
def test_host_replica_against_hmmsearch_on_the_golden_cases(name):
    """reg and clu equal on every fixture row; "%.1f" % exp equals the printed text unless the float64 value lies within
    1e-3 of a print boundary (tests/tblout_common.py: the bound), on at most 2 % of a file's rows."""
    from tests.conftest import load_case
    from witch_amd.ehmm import seq_expect_host
    case, fx = load_case(name), tc.load_fixture(name)
    assert fx["queries"] == case.qnames and [m["hmm_file"] for m in fx["models"]] == case.hmm_files
    _, (res, off) = _digitized(case)
    H = len(case.hmm_paths)
    qi = {n: i for i, n in enumerate(case.qnames)}
    pairs, rows = [], []
    for h, m in enumerate(fx["models"]):
        for r in m["rows"]:
            pairs.append(qi[r["target"]] * H + h)
            rows.append(r)
    assert rows
    _check_expect(name, seq_expect_host(case.hmm_paths, res, off, pairs), rows)


@pytest.mark.parametrize("alphabet", tc.CLASS_ALPHABETS)
def test_host_replica_against_hmmsearch_on_the_class_models(alphabet):
    """The same on the seeded models at the class edges of the counting sweep (1 to 3 073 nodes), each on its own queries."""
    from witch_amd.ehmm import seq_expect_host
    fx = tc.load_fixture("classes")
    assert fx["nodes"] == tc.CLASS_NODES
    models = tc.class_models(alphabet)
    paths, res, off, pairs, names = tc.class_call(alphabet)
    at = {nm: t for t, nm in enumerate(names)}
    sel, rows = [], []
    for (M, _, digest, queries), rec in zip(models, fx["alphabets"][alphabet]):
        assert (rec["M"], rec["seed"], rec["sha256"]) == (M, 1000 + M, digest), (alphabet, M, "the model writer's text changed")
        assert rec["queries"] == [n for n, _ in queries]
        for r in rec["rows"]:
            sel.append(pairs[at[(M, r["target"])]])
            rows.append(r)
    assert len(rows) >= 100
    _check_expect("classes " + alphabet, seq_expect_host(paths, res, off, sel), rows)


def test_host_replica_refuses_a_pair_outside_the_call():
    from tests.conftest import load_case
    from witch_amd._lib import WitchHipError
    from witch_amd.ehmm import seq_expect_host
    case = load_case("dna_hmmbuild")
    _, (res, off) = _digitized(case)
    with pytest.raises(WitchHipError):
        seq_expect_host(case.hmm_paths, res, off, [len(case.qnames) * len(case.hmm_paths)])
    assert len(seq_expect_host(case.hmm_paths, res, off, [])) == 0


# ------------------------------------------------------------------------------------------------ 2. the text
def _entry(r):
    e = {k: r[k] for k in ("target", "tacc", "query", "qacc")}
    for k in ("evalue", "score", "bias", "best_evalue", "best_score", "best_bias", "exp"):
        e[k] = float(r[k])
    for k in tc.INT_COLUMNS:
        e[k] = int(r[k])
    e["desc"] = r["desc"]
    return e


@pytest.mark.parametrize("name", tc.CASES + ("classes",))
def test_format_tblout_lines_byte_for_byte(name):
    """From the fixture's own numbers the formatter gives HMMER's raw lines, its three header lines and its trailer."""
    from witch_amd.shim import formats
    fx = tc.load_fixture(name)
    models = fx["models"] if "models" in fx else [m for a in tc.CLASS_ALPHABETS for m in fx["alphabets"][a]]
    n = 0
    for m in models:
        entries = [_entry(r) for r in m["rows"]]
        widths = formats._tbl_widths(entries)
        assert formats.format_tblout_lines(entries) == [r["raw"] for r in m["rows"]]
        assert formats.format_tblout_header(widths) == m["header"]
        text = formats.format_tblout("m.hmm", "q.fa", {"name": "x"}, entries, option_settings="hmmsearch m.hmm q.fa", cwd="/d",
                                     date="Wed Oct 21 05:57:13 2026").splitlines()
        body = len(m["header"]) + len(entries)
        assert text[:body] == m["header"] + [r["raw"] for r in m["rows"]]
        assert [t for t in text[body:] if not t.startswith(("# Query file", "# Target file", "# Option settings", "# Current dir", "# Date"))] == m["trailer"]
        assert text[body + 4:body + 9] == ["# Query file:      m.hmm", "# Target file:     q.fa", "# Option settings: hmmsearch m.hmm q.fa",
                                           "# Current dir:     /d", "# Date:            Wed Oct 21 05:57:13 2026"]
        n += len(entries)
    assert n > 0


def test_format_tblout_widths_descriptions_and_capped_rows():
    from witch_amd.shim import formats
    e = _entry(tc.load_fixture("dna_hmmbuild")["models"][0]["rows"][0])
    long = dict(e, target="a_target_name_of_more_than_twenty_characters", desc="16S ribosomal RNA", capped=True)
    lines = formats.format_tblout_lines([e, long])
    assert lines[0].startswith(e["target"].ljust(44) + " -") and lines[1].endswith(" 16S ribosomal RNA")
    hdr = formats.format_tblout_header(formats._tbl_widths([e, long]))
    assert hdr[1].startswith("# target name".ljust(44) + " accession") and hdr[2].startswith("#" + "-" * 43 + " ")
    text = formats.format_tblout("m.hmm", "q.fa", {"name": "sub"}, [e, long]).splitlines()
    assert text[5].startswith("# witch-hip:") and text[5].endswith(": " + long["target"]) and text[6] == "#" and text[-1] == "# [ok]"
    assert not [t for t in formats.format_tblout("m.hmm", "q.fa", {"name": "sub"}, [e]).splitlines() if "witch-hip" in t]


# ------------------------------------------------------------------------------------------------ 3. the assembly
def _invert_domain(score, bias, L, Ld):
    """(envsc, domcorr) in nats that give HMMER's printed per-domain score and bias (include/witch_hip.h: the formula)."""
    ln2 = math.log(2.0)
    dombias = float(bias) * ln2
    domcorr = (math.log(math.expm1(dombias)) if dombias > 1e-9 else -40.0) + math.log(256.0)
    nullsc = L * math.log(L / (L + 1.0)) + math.log(1.0 / (L + 1.0))
    envsc = float(score) * ln2 + nullsc + dombias - (L - Ld) * math.log(L / (L + 3.0))
    return envsc, domcorr


@pytest.mark.parametrize("name", ("dna_hmmbuild", "amino_hmmbuild", "amino_multidomain"))
def test_assembly_host_half_against_hmmsearch_columns(name):
    """wh_seq_table_host fed with HMMER's own domain lists (tests/golden/domains): ov, env, dom, rep, inc and the best
    domain's score and bias equal HMMER's --tblout columns on every row that both fixtures cover - a pair of a model and a
    query that the domain fixture ran, ALL of whose domains it lists (it holds the reportable ones: "of" says how many
    there are).  The domain records hold HMMER's printed numbers: envsc and domcorr are inverted from the printed score and
    bias, so a domain's E-value is known to the 0.05 bit of the print; a row one of whose E-values lies within that of a
    threshold it is compared with could not be decided and is counted (none does)."""
    from tests import domains_reference as dr
    from tests.conftest import load_case
    from witch_amd import _lib
    from witch_amd.ehmm import seq_table_host
    from witch_amd.shim.formats import hmm_header
    case, fx, dfx = load_case(name), tc.load_fixture(name), dr.load_fixture(name)
    fxd = dr.fixture_domains(name)
    nq, H = len(dfx["queries"]), len(dfx["models"])
    assert dfx["queries"] == case.qnames[:nq]
    lengths = np.array([len(s) for s in case.qseqs[:nq]], dtype=np.int64)
    checked = uncovered = undecided = 0
    for h in range(H):
        m = fx["models"][h]
        hdr = hmm_header(case.hmm_paths[h])
        lam, tau = hdr["flambda"], hdr["ftau"]
        Z, domZ = float(m["Z"]), float(m["domZ"])
        flags = np.zeros((nq, 1), dtype=np.uint8)
        det = (_lib.PairDetail * nq)()
        want, expect = [], []
        rows = {r["target"]: r for r in m["rows"]}
        for q in range(nq):
            r = rows.get(case.qnames[q])
            lines = fxd.get((q, h), [])
            if r is None:
                continue
            if not lines or len(lines) != int(lines[0]["of"]) or int(lines[0]["of"]) > _lib.WH_MAX_ENVELOPES:
                uncovered += 1
                continue
            L = int(lengths[q])
            d = det[q]
            d.seq_score, d.pre_score = float(r["score"]), float(r["score"]) + float(r["bias"])
            d.nregions, d.nenv = int(r["reg"]), len(lines)
            near = False
            for t, ln in enumerate(lines):
                d.env_i[t], d.env_j[t] = int(ln["env_from"]), int(ln["env_to"])
                d.envsc[t], d.domcorr[t] = _invert_domain(ln["dom_score"], ln["dom_bias"], L, d.env_j[t] - d.env_i[t] + 1)
                bits = float(ln["dom_score"])
                for thr in (10.0, 0.01):
                    edge = tau - math.log(thr / domZ) / lam          # the score at which exp(lnP) domZ == thr
                    near |= abs(bits - edge) <= 0.0501
            edge = tau - math.log(0.01 / Z) / lam
            if near or abs(float(r["score"]) - edge) <= 0.0501:
                undecided += 1
                continue
            flags[q, 0] = 1
            want.append(r)
            expect.append((float(r["exp"]), int(r["reg"]), int(r["clu"])))
        got = seq_table_host([tau], [lam], lengths, flags, det, np.array(expect, dtype=np.dtype(_lib.SEQ_EXPECT_FIELDS)),
                             Z=Z, domZ=domZ, E=99999999.0)
        assert len(got) == len(want)
        for g, r in zip(got, want):
            assert [int(g[k]) for k in ("reg", "clu", "ov", "env", "dom", "rep", "inc")] == [int(r[k]) for k in ("reg", "clu", "ov", "env", "dom", "rep", "inc")], (name, h, r["raw"], g)
            assert ("%.1f" % g["best_bits"], "%.1f" % g["best_bias_bits"]) == (r["best_score"], r["best_bias"]), (name, h, r["raw"], g)
            assert int(g["capped"]) == (1 if int(r["env"]) == _lib.WH_MAX_ENVELOPES else 0)
            checked += 1
    print("[%s] %d rows checked, %d rows whose domain list the fixture holds in part, %d at a threshold" % (name, checked, uncovered, undecided))
    assert checked >= 20 and undecided == 0


def test_assembly_host_half_capacity_and_options():
    from witch_amd import _lib
    from witch_amd.ehmm import seq_table_host
    det = (_lib.PairDetail * 2)()
    for d in det:
        d.nenv, d.nregions, d.env_i[0], d.env_j[0], d.envsc[0], d.seq_score, d.pre_score = 1, 1, 1, 10, 5.0, 3.0, 3.5
    flags = np.array([[1], [1]], dtype=np.uint8)
    exp = np.array([(1.0, 1, 0)] * 2, dtype=np.dtype(_lib.SEQ_EXPECT_FIELDS))
    rows = seq_table_host([np.nan], [np.nan], [10, 10], flags, det, exp)
    assert len(rows) == 2 and list(rows["pair"]) == [0, 1] and list(rows["rep"]) == [1, 1] and np.isnan(rows["seq_lnP"]).all()
    assert np.allclose(rows["seq_bias_bits"], 0.5)
    import ctypes as C
    out = np.zeros(1, dtype=np.dtype(_lib.SEQ_ROW_FIELDS))
    lens = np.array([10, 10], dtype=np.int64)
    tau = np.array([np.nan], dtype=np.float32)
    rc = _lib.lib().wh_seq_table_host(1, tau.ctypes.data, tau.ctypes.data, lens.ctypes.data, 2, flags.ctypes.data, C.addressof(det),
                                      exp.ctypes.data, None, out.ctypes.data, 1)
    assert rc == _lib.WH_ERANGE
    with pytest.raises(_lib.WitchHipError):
        seq_table_host([np.nan], [np.nan], [10, 10], flags, det, exp, domE=-1.0)


# ------------------------------------------------------------------------------------------------ 4. the server
class _Backend:
    def __init__(self):
        self.calls = []

    def _rows(self, records):
        return [(n, 10.0 * len(t), 0.5, 1, 10.0 * len(t) + 0.04) for n, t in records]

    def search(self, hmm_path, records, **kw):
        from witch_amd.shim import formats
        self.calls.append(("search", kw))
        rows = self._rows(records)
        if kw.get("want_domains"):
            return formats.hmm_header(hmm_path), rows, {}
        return formats.hmm_header(hmm_path), [r[:4] for r in rows]

    def search_table(self, hmm_path, records, table, **kw):
        from witch_amd import _lib
        from witch_amd.shim import formats
        self.calls.append(("search_table", dict(kw, table=table)))
        tbl = np.zeros(len(records), dtype=np.dtype(_lib.SEQ_ROW_FIELDS))
        for i, (n, t) in enumerate(records):
            tbl[i] = (i, -3.0 * len(t), 10.0 * len(t) + 0.04, 0.5, 1.2, 1, 0, 0, 1, 1, 1, 1, 0, 9.0 * len(t), 0.25, -2.5 * len(t), 0, 0)
        return formats.hmm_header(hmm_path), self._rows(records), ({} if kw.get("want_domains") else None), None, tbl


class _OldBackend:
    def search(self, hmm_path, records, **kw):
        from witch_amd.shim import formats
        return formats.hmm_header(hmm_path), [(n, 10.0 * len(t), 0.5, 1) for n, t in records]


def test_server_writes_tblout_only_when_asked(tmp_path):
    from witch_amd.shim.server import ArgError, Server, check_hmmsearch_options, parse_hmmsearch_argv
    (tmp_path / "m.hmm").write_text("HMMER3/f [3.1b2 | February 2015]\nNAME  A_0_7\nLENG  12\nALPH  DNA\n"
                                    "STATS LOCAL FORWARD  -4.2 0.71\nHMM  A C G T\n")
    (tmp_path / "q.fa").write_text(">q1 first record\nACGTACGTAC\n>q2\nACGTTT\n")
    srv = Server.__new__(Server)
    srv.backend = _Backend()
    plain = srv.run_hmmsearch("--max -E 99999999 m.hmm q.fa".split(), str(tmp_path))
    assert srv.backend.calls == [("search", {})] and not (tmp_path / "t.tbl").exists()      # (the backend is reached as before)
    out = srv.run_hmmsearch("--max -E 99999999 --tblout t.tbl m.hmm q.fa".split(), str(tmp_path))
    assert out == plain
    kind, kw = srv.backend.calls[1]
    assert kind == "search_table" and kw["want_domains"] is False and kw["inc"] is None
    assert kw["table"] == {"Z": None, "domZ": None, "E": 99999999.0, "domE": 10.0, "incE": 0.01, "incdomE": 0.01}
    text = (tmp_path / "t.tbl").read_text().splitlines()
    body = [ln for ln in text if not ln.startswith("#")]
    assert [ln.split()[0] for ln in body] == ["q1", "q2"] and body[0].endswith(" first record") and body[1].endswith(" -")
    assert body[0].split()[2:13] == ["A_0_7", "-", "1.9e-13", "100.0", "0.5", "2.8e-11", "90.0", "0.2", "1.2", "1", "0"]
    assert text[0].startswith("#") and text[-1] == "# [ok]" and any(t.startswith("# Date:") for t in text)
    assert any(t == "# Option settings: hmmsearch --max -E 99999999 --tblout t.tbl m.hmm q.fa" for t in text)
    # together with --domtblout: both files, the main output that of the call without --tblout
    both = srv.run_hmmsearch("--max -E 99999999 -Z 50 --domZ 7 --tblout t2.tbl --domtblout d.tbl m.hmm q.fa".split(), str(tmp_path))
    alone = srv.run_hmmsearch("--max -E 99999999 -Z 50 --domZ 7 --domtblout d2.tbl m.hmm q.fa".split(), str(tmp_path))
    assert both == alone and (tmp_path / "d.tbl").read_text() == (tmp_path / "d2.tbl").read_text() and (tmp_path / "t2.tbl").exists()
    assert srv.backend.calls[2][1]["table"]["Z"] == 50.0 and srv.backend.calls[2][1]["table"]["domZ"] == 7.0 and srv.backend.calls[2][1]["want_domains"] is True
    for bad in ("--max --tblout t -Z 0 m q", "--max --tblout t --domZ -3 m q", "--max --tblout t --domZ x m q", "--max --tblout t --incE -1 m q"):
        with pytest.raises(ArgError):
            check_hmmsearch_options(parse_hmmsearch_argv(bad.split())[0])
    srv.backend = _OldBackend()
    with pytest.raises(ArgError, match="--tblout"):
        srv.run_hmmsearch("--max -E 99999999 --tblout t3.tbl m.hmm q.fa".split(), str(tmp_path))
    assert not (tmp_path / "t3.tbl").exists()
    assert srv.run_hmmsearch("--max -E 99999999 m.hmm q.fa".split(), str(tmp_path)) == plain


# ------------------------------------------------------------------------------------------------ resources
def test_counting_sweep_kernels_use_no_scratch():
    """The compiler's own report for wh_seqtab.hip (no GPU): the twelve register-class instantiations of the counting sweep,
    the any-size kernel and the two assembly kernels keep their state in registers - no scratch frame, hence none in a row
    loop."""
    import os
    import re
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "witch_amd", "csrc", "wh_seqtab.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-c", src, "-o", os.devnull], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == 15 and sum("seq_expect_kernelILi" in n for n in names) == 12, names
    assert not any(scratch), list(zip(names, scratch))
