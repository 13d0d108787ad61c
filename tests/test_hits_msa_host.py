"""hmmsearch -A without a GPU: the CPU recipe (tests/hits_msa_reference.py: oracle records -> slice -> quantise ->
msa_reference.assemble -> formats.format_hits_msa) against the bundled binary's files (tests/golden/hits_msa), the formats, the
server with a stub backend, and the C ABI's argument checks.

What the recipe reproduces: on the queries without the chim* records, (b), the WHOLE file - names, order, "#=GS DE" lines, rows,
every PP character, PP_cons in HMMER's own arithmetic (found: hr.cons_chars), RF - wherever the fixture lists no row in
ref_mismatch_b (amino_hmmbuild 0, dna_hmmbuild 0 and 1).  The listed rows are WEAK domains, the known difference of DESIGN.md
section 4.10, and this file checks that they are: HMMER prints an accuracy below 0.95 for the domain, or the row differs in
PP characters alone, each one step apart where the float64 posterior is within 0.0151 of a character boundary - the bound
tests/domains_reference.py puts on HMMER's own float32 accuracy of a strong domain against the float64 reference."""
import numpy as np
import pytest

from tests import domains_reference as dr
from tests import hits_msa_reference as hr
from tests import msa_reference as mr
from tests.conftest import load_case

HMMER_PP = 0.0151      # (tests/domains_reference.py: how far HMMER's own accuracy of a strong domain lies from the float64 one)
BOUNDS = 0.05 + np.arange(10) / 10.0


def _keep(fx, run):
    return [fx["queries"].index(n) for n in run["queries"]]


def _weak_or_band(case_name, h, name, ours, theirs):
    """A row of ref_mismatch is what DESIGN.md section 4.10 describes (see the module's docstring)."""
    seqs, dom = dr.case_reference(case_name)
    qname, rng_ = name.rsplit("/", 1)
    ai, aj = (int(x) for x in rng_.split("-"))
    q = dr.load_fixture(case_name)["queries"].index(qname)
    best = max(dom[(q, h)], key=lambda d: min(aj, d["ali_j"]) - max(ai, d["ali_i"]))
    Ld = best["env_j"] - best["env_i"] + 1
    # the strata are HMMER's: the accuracy it prints for the domain (tests/golden/domains), as in tests/domains_reference.py
    lines = dr.fixture_domains(case_name).get((q, h), [])
    line = max(lines, key=lambda ln: min(aj, int(ln["ali_to"])) - max(ai, int(ln["ali_from"])))
    if float(line["acc"]) < 0.95:
        return "weak"
    assert name in ours[0] and name in theirs[0], (name, "a strong domain whose coordinates differ")
    assert hr.match_and_inserts(ours[0][name], ours[3]) == hr.match_and_inserts(theirs[0][name], theirs[3]), name
    ref = np.asarray(best["pp"][ai - best["env_i"]:aj - best["env_i"] + 1])
    _, a = mr.decode_row(ours[0][name], ours[1][name], ours[3])
    _, b = mr.decode_row(theirs[0][name], theirs[1][name], theirs[3])
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            assert abs(mr.CHARS.index(x) - mr.CHARS.index(y)) == 1 and np.min(np.abs(ref[i] - BOUNDS)) <= HMMER_PP, (name, i, x, y, ref[i])
    return "band"


@pytest.mark.parametrize("case_name", list(hr.MODELS))
def test_recipe_against_the_binary(case_name):
    fx = hr.load_fixture(case_name)
    assert [m["h"] for m in fx["models"]] == hr.MODELS[case_name]
    whole = 0
    for model in fx["models"]:
        h = model["h"]
        for key, run in sorted(model["runs"].items()):
            inc = dict(zip([o[2:] for o in run["args"][::2]], [float(v) for v in run["args"][1::2]])) if "--notextw" not in run["args"] else {}
            text, m, names = hr.reference(case_name, h, keep=_keep(fx, run), descriptions=run["desc"], notextw="--notextw" in run["args"], **inc)
            from witch_amd.shim import formats
            assert formats.hits_msa_trailer(len(m["row_recs"]), "ALI") == run["trailer"], (case_name, h, key)
            listed = set(model["ref_mismatch"] if key == "a" else model["ref_mismatch_b"])
            if key != "a" and not listed:
                assert text == run["sto"], (case_name, h, key, "whole file")
                whole += 1
                continue
            ours, theirs = mr.parse_msa(text), mr.parse_msa(run["sto"])
            (on, od), (tn, td) = hr.parse_gs(text), hr.parse_gs(run["sto"])
            assert [n for n in on if n not in listed] == [n for n in tn if n not in listed], (case_name, h, key)
            assert [n.split("/")[0] for n in on] == [n.split("/")[0] for n in tn]
            for n in on:
                if n not in listed:
                    assert od[n] == td[n]
                    for part in (0, 1):           # the row and its PP row: on the match columns and in the insert residues
                        assert hr.match_and_inserts(ours[part][n], ours[3]) == hr.match_and_inserts(theirs[part][n], theirs[3]), (case_name, h, key, n)
            kinds = [_weak_or_band(case_name, h, n, ours, theirs) for n in sorted(listed) if n in on or n in tn]
            assert len(listed) <= 0.3 * len(tn) or key in ("inc", "none"), (case_name, h, key, "most rows must be compared")
            print("%s model %d %s: %d rows, %d listed in ref_mismatch (%d weak, %d guard band)" %
                  (case_name, h, key, len(tn), len(kinds), kinds.count("weak"), kinds.count("band")))
    assert whole >= {"amino_hmmbuild": 4, "dna_hmmbuild": 5, "amino_multidomain": 0}[case_name], (case_name, whole)


def test_pp_cons_arithmetic_and_tie_columns():
    """HMMER's arithmetic differs from wh_msa's float32 sum exactly where it matters: the (b) files have tie columns (the exact
    mean of the decoded tenths on a character boundary), and hr.cons_chars gives the binary's character on every one."""
    ties = 0
    for case_name, h in (("amino_hmmbuild", 0), ("dna_hmmbuild", 0), ("dna_hmmbuild", 1)):
        fx = hr.load_fixture(case_name)
        model = [m for m in fx["models"] if m["h"] == h][0]
        run = model["runs"]["b"]
        _, m, _ = hr.reference(case_name, h, keep=_keep(fx, run))
        cons = mr.parse_msa(run["sto"])[2]
        assert m["pp_cons"].tobytes().decode() == cons
        t = hr.tie_columns(len(m["matmap"]), m["cols"], m["pps"])
        ties += len(t)
        for k in t:
            assert cons[m["matmap"][k]] in "123456789*"
    assert ties >= 3
    assert [hr.encode(p) for p in (0.0499, 0.05, 0.9499, 0.95, np.float32(0.95000005), 1.0)] == list("0199**")
    assert hr.quantise([0.0499, 0.05, 0.9499, 0.95, 1.0, 0.25]).tolist() == [np.float32(x) for x in (0.0, 0.1, 0.9, 0.9, 1.0, 0.3)]


def test_formats(tmp_path):
    from witch_amd.shim import formats
    fa = tmp_path / "q.fa"
    fa.write_text(">s1 a protein  of interest\nACGT\nAC\n>s2\nGG\n>s3   \nTT\n")
    desc = {}
    assert formats.read_fasta(str(fa), descriptions=desc) == formats.read_fasta(str(fa)) == [("s1", "ACGTAC"), ("s2", "GG"), ("s3", "TT")]
    assert desc == {"s1": "a protein  of interest"}
    recs = np.array([(1, 0, 1, 2), (0, 1, 3, 6)], dtype=np.int32)
    rows, pps = [b"GG--", b"ACgt"], [b"98..", b"**55"]
    text = formats.format_hits_msa(["s1", "s2", "s3"], recs, rows, pps, b"9*..", b"xx..", descriptions=desc)
    assert text.splitlines()[:4] == ["# STOCKHOLM 1.0", "", "#=GS s2/1-2 DE [subseq from] s2", "#=GS s1/3-6 DE [subseq from] a protein  of interest"]
    assert "s2/1-2         GG--" in text and "#=GR s1/3-6 PP **55" in text and text.endswith("#=GC RF        xx..\n//\n")
    assert formats.format_hits_msa(["s1"], [], [], [], b"", b"") == ""
    assert formats.hits_msa_trailer(0, "f.sto") == "# No hits satisfy inclusion thresholds; no alignment saved"
    assert formats.hits_msa_trailer(3, "f.sto") == "# Alignment of 3 hits satisfying inclusion thresholds saved to: f.sto"
    wide = formats.format_hits_msa(["s"], [(0, 0, 1, 300)], [b"A" * 300], [b"9" * 300], b"9" * 300, b"x" * 300)
    one = formats.format_hits_msa(["s"], [(0, 0, 1, 300)], [b"A" * 300], [b"9" * 300], b"9" * 300, b"x" * 300, notextw=True)
    assert wide.count("s/1-300 ") == 1 + 2 * 2 and one.count("s/1-300 ") == 1 + 2


# ------------------------------------------------------------------------------------------------ the server, stub backend
class StubBackend:
    """Records how it is called; a canned two-row alignment."""

    def __init__(self):
        self.calls = []

    def search(self, hmm_path, records, **kw):
        from witch_amd.shim import formats
        self.calls.append(("search", [n for n, _ in records], kw))
        hdr = formats.hmm_header(hmm_path)
        rows = [(n, 10.0 * len(t) + 0.5, 1.25, 1) for n, t in records]
        if kw.get("want_domains"):
            return hdr, [r + (r[1],) for r in rows], {}
        return hdr, rows

    def search_hits(self, hmm_path, records, inc, want_domains=False, **kw):
        hdr, rows = self.search(hmm_path, records)[:2]
        self.calls[-1] = ("search_hits", [n for n, _ in records], dict(kw, inc=inc, want_domains=want_domains))
        n = 0 if inc["incE"] < 1e-100 else 2
        hits = {"row_recs": np.array([(1, 0, 2, 5), (0, 0, 1, 4)][:n], dtype=np.int32).reshape(n, 4), "rows": [b"CGTA", b"ACGT"][:n],
                "pp_rows": [b"9999", b"****"][:n], "pp_cons": b"****", "rf": b"xxxx", "W": 4}
        return hdr, [r + (r[1],) for r in rows], ({} if want_domains else None), hits


class OldBackend:
    def search(self, hmm_path, records, **kw):
        return StubBackend().search(hmm_path, records, **kw)


def test_server_with_a_stub_backend(tmp_path):
    from witch_amd.shim.server import ArgError, Server
    case = load_case("dna_hmmbuild")
    hmm = case.hmm_paths[0]
    (tmp_path / "q.fa").write_text(">one first record\nACGTA\n>two\nACGTAC\n")
    be = StubBackend()
    srv = Server(be, str(tmp_path / "unused.sock"))
    base = ["--noali", "-E", "99999999", "--max"]
    plain = srv.run_hmmsearch(base + [hmm, "q.fa"], str(tmp_path))
    assert be.calls == [("search", ["one", "two"], {})]
    # -Z 0 without --domtblout / -A is still not read
    assert srv.run_hmmsearch(base + ["-Z", "0", hmm, "q.fa"], str(tmp_path)) == plain and be.calls[-1] == ("search", ["one", "two"], {})
    text = srv.run_hmmsearch(base + ["-A", "hits.sto", "--incE", "1e-5", "-Z", "1000", hmm, "q.fa"], str(tmp_path))
    assert be.calls[-1] == ("search_hits", ["one", "two"], {"inc": {"incE": 1e-5, "incdomE": 0.01, "Z": 1000.0, "domZ": None}, "want_domains": False})
    lines = text.splitlines()
    at = lines.index("//")
    assert lines[at + 1] == "# Alignment of 2 hits satisfying inclusion thresholds saved to: hits.sto" and lines[at + 2:] == ["[ok]"]
    assert lines[:at + 1] + lines[at + 2:] == plain.splitlines(), "without the trailer the text is today's"
    sto = (tmp_path / "hits.sto").read_text()
    assert sto.splitlines()[2:4] == ["#=GS two/2-5 DE [subseq from] two", "#=GS one/1-4 DE [subseq from] first record"]
    assert "two/2-5         CGTA" in sto and sto.endswith("//\n")
    # with --domtblout in the same call: one backend call serves both files
    n = len(be.calls)
    srv.run_hmmsearch(base + ["-A", "hits2.sto", "--domtblout", "d.tbl", "-o", "o.txt", hmm, "q.fa"], str(tmp_path))
    assert len(be.calls) == n + 1 and be.calls[-1][0] == "search_hits" and be.calls[-1][2]["want_domains"] is True
    assert (tmp_path / "hits2.sto").read_text() == sto and (tmp_path / "d.tbl").exists() and "saved to: hits2.sto" in (tmp_path / "o.txt").read_text()
    # nothing included: the file is created empty
    text = srv.run_hmmsearch(base + ["-A", "none.sto", "--incE", "1e-200", hmm, "q.fa"], str(tmp_path))
    assert (tmp_path / "none.sto").read_text() == "" and "# No hits satisfy inclusion thresholds; no alignment saved\n[ok]\n" in text
    for bad in (["-Z", "0"], ["--domZ", "x"], ["--incE", "-1"], ["--incdomE", "nan"], ["--incT", "3"]):
        with pytest.raises(ArgError):
            srv.run_hmmsearch(base + ["-A", "x.sto"] + bad + [hmm, "q.fa"], str(tmp_path))
    assert not (tmp_path / "x.sto").exists()
    with pytest.raises(ArgError, match="-A needs a backend"):
        Server(OldBackend(), str(tmp_path / "unused2.sock")).run_hmmsearch(base + ["-A", "y.sto", hmm, "q.fa"], str(tmp_path))
    assert not (tmp_path / "y.sto").exists()


def test_abi_refuses_without_a_device():
    import ctypes as C
    from witch_amd import _lib
    L = _lib.lib()
    ok, bad = _lib.HitsOpts(10.0, 5.0, 0.01, 0.01), _lib.HitsOpts(0.0, 5.0, 0.01, 0.01)
    n, W = C.c_int64(0), C.c_int64(0)
    p = [C.c_void_p(None) for _ in range(6)]
    outs = [C.byref(n), C.byref(p[0]), C.byref(W)] + [C.byref(x) for x in p[1:]]

    def host(handle, h, o):
        return L.wh_hits_msa(handle, None, None, None, 0, None, None, None, h, None, C.byref(o) if o else None, 0, None, *outs)

    def dev(handle, h, o):
        return L.wh_hits_msa_dev(handle, None, None, 0, None, None, None, None, None, None, None, h, None, C.byref(o) if o else None, 0, *outs, None)
    for f, who in ((host, b"wh_hits_msa:"), (dev, b"wh_hits_msa_dev:")):
        assert f(None, 0, ok) == _lib.WH_EINVAL and who in L.wh_last_error() and b"null handle" in L.wh_last_error()
        assert f(None, -1, ok) == _lib.WH_EINVAL and who in L.wh_last_error() and b"model position" in L.wh_last_error()
        assert f(None, 0, bad) == _lib.WH_EINVAL and who in L.wh_last_error() and b"Z = 0" in L.wh_last_error()
        assert f(None, 0, _lib.HitsOpts(10.0, -1.0, 0.01, 0.01)) == _lib.WH_EINVAL and b"domZ" in L.wh_last_error()
        assert f(None, 0, None) == _lib.WH_EINVAL and who in L.wh_last_error()
    e_off, pc, pp = (C.c_int64 * 1)(), C.c_void_p(None), C.c_void_p(None)
    assert L.wh_domain_paths(None, None, None, 0, None, None, None, None, e_off, C.byref(pc), C.byref(pp)) == _lib.WH_EINVAL
    assert b"wh_domain_paths" in L.wh_last_error()
    assert L.wh_domain_paths_dev(None, None, None, 0, 0, 0, None, None, None, None, C.byref(pc), C.byref(pc), C.byref(pp), C.byref(n), None) == _lib.WH_EINVAL
    assert b"wh_domain_paths_dev" in L.wh_last_error()
    assert L.wh_last_kernel_ms(None, 8, None, None) == _lib.WH_EINVAL


def test_hand_made_shapes_build_without_a_device():
    """The hand-made arrays of tests/test_hits_msa_gpu.py and their numpy restatement, checked here for what they promise."""
    from tests.test_hits_msa_gpu import Shapes
    s = Shapes(device="cpu")
    want = s.want(list(range(s.nq)), 8, 6, 0.01, 0.01)
    assert sorted(r[3] - r[2] + 1 for r in want["row_recs"]) == [1, 48, 63, 64, 65, 65, 129]
    assert [r[:2] for r in want["row_recs"]] == [(0, 0), (0, 1), (1, 0), (2, 0), (3, 0), (5, 1), (7, 1)]
    assert want["W"] > s.M and len(s.want(list(range(s.nq)), 8, 6, 1e9, 1e9)["row_recs"]) == 9
    assert len(s.want(list(range(s.nq)), 8, 6, 0.0, 0.0)["row_recs"]) == 0
