"""hmmalign --mapali, the parts that need no GPU: the numpy restatement (tests/mapali_reference.py) against the bundled
binary's outputs, the alignment checksum against hmmbuild's CKSUM lines, the alignment readers, format_msa with rows that
have no PP line and with the "#=GS DE" block, run_hmmalign --mapali over a stub backend, the checksum-mismatch message, and the
error paths of wh_msa_mapali / wh_msa_mapali_dev.  Fixtures: tests/golden/mapali (tests/golden/make_golden_mapali.py)."""
import glob
import os

import numpy as np
import pytest

from tests import mapali_reference as mp
from tests import msa_reference as mr
from witch_amd.shim import formats

FORMATS = [("sto", "Stockholm", False), ("trim", "Stockholm", True), ("pfam", "Pfam", False), ("afa", "afa", False)]


def _restated(name, i, trim):
    """The restatement on the alignment's rows and on the new sequences' columns and PP characters as decoded from the binary's
    default output."""
    p, d = mp.load_fixture(name)[i], mp.part_inputs(name, i)
    n_map = len(d["names"])
    return mp.assemble(d["M"], d["map_cols"] + d["cols"], [None] * n_map + [mr.midpoints(x) for x in d["digits"]],
                       d["map_texts"] + p["seqs"], n_nopp=n_map, trim=trim)


@pytest.mark.parametrize("name,i", mp.all_parts())
def test_restatement_reproduces_the_four_outputs(name, i):
    """Rows (the alignment's and the new sequences'), PP rows and RF byte for byte, with and without --trim; PP_cons between the
    characters the new sequences' PP characters allow (tests/test_msa_host.py); and format_msa on the restatement's matrices
    (with the binary's PP_cons line) is the binary's text in all four forms."""
    p, d = mp.load_fixture(name)[i], mp.part_inputs(name, i)
    names = d["names"] + p["names"]
    for key, fmt, trim in FORMATS:
        rows, pps, cons, rf = mr.parse_msa(p["out"]["trim" if trim else "sto"])
        got = _restated(name, i, trim)
        assert got["W"] == len(rf) and got["rf"].tobytes().decode() == rf
        assert np.array_equal(got["rows"], mr.matrix(rows, names)), (name, i, key)
        assert np.array_equal(got["pp_rows"], mr.matrix(pps, p["names"])), (name, i, key)
        assert not set(pps) & set(d["names"]) and got["pathless"] == 0
        lo, hi = mr.cons_interval(d["M"], d["cols"], d["digits"])
        ours = got["pp_cons"].tobytes().decode()
        for k, at in enumerate(got["matmap"]):
            assert (cons[at] == ".") == (lo[k] == ".") == (ours[at] == "."), (name, i, key, k)
            if cons[at] != ".":
                assert mr.CHARS.index(lo[k]) <= mr.CHARS.index(cons[at]) <= mr.CHARS.index(hi[k]), (name, i, key, k)
                assert mr.CHARS.index(lo[k]) <= mr.CHARS.index(ours[at]) <= mr.CHARS.index(hi[k]), (name, i, key, k)
        text = formats.format_msa(names, got["rows"], [None] * len(d["names"]) + list(got["pp_rows"]), cons, got["rf"], fmt, desc=d["desc"])
        assert text == p["out"][key], (name, i, key)


def test_fixtures_show_the_rules():
    """The probe's output holds what it was planted for: an insert behind a deleted node and before a row's first match
    residue (r3), two rows' single residues in the last cell of block 0, a run of two split left / right (r6), blocks 0 and M
    emptied by --trim, a "#=GS" line carried over, and no PP line for a row of the alignment."""
    p = mp.load_fixture("one_new")[0]
    rows, pps, cons, rf = mr.parse_msa(p["out"]["sto"])
    assert rf == "..xxxxxxx.xxxxxx...xxxxxxxxxxxx.."
    assert rows["r3"] == "..-------gGTTGC-tct-CGTGCATG---.." and rows["r6"] == "..ACGTACAg------t.c------------.."
    assert rows["r5"][:2] == ".a" and rows["r2"][:2] == ".c" and rows["r0"][:2] == "gt" and rows["r1"][8] == "A"
    assert list(pps) == ["n1"] and cons == pps["n1"]
    assert mr.parse_msa(p["out"]["trim"])[3] == rf[2:-2]
    sto = mp.load_fixture("planted_sto")[0]
    assert sto["out"]["sto"].startswith("# STOCKHOLM 1.0\n\n#=GS r0 DE the first row of the probe\n\nr0 ")
    assert sto["out"]["afa"].startswith(">r0 the first row of the probe\n")
    assert len(mp.part_inputs("rows65", 0)["names"]) == 65 and len(mp.part_inputs("rows65", 0)["rows"][0]) > 128
    bad = mp.load_fixture("mismatch")[0]
    assert bad["status"] == 1 and bad["stderr"] == "--mapali MSA ALN isn't same as the one HMM came from (checksum mismatch)\n"


def test_checksum_is_hmmbuilds_cksum_line():
    """wh_alignment_checksum (wh_build.cpp's own code) and the restatement on all the .afa / .hmm pairs of hmmbuild_cases, and on
    the Stockholm copy of the probe ('.' gaps, upper case: neither enters the checksum)."""
    from witch_amd.ehmm import alignment_checksum
    pairs = sorted(glob.glob(os.path.join(mr.GOLDEN, "hmmbuild_cases", "*.afa")))
    assert len(pairs) == 20
    for afa in pairs:
        with open(afa[:-4] + ".hmm") as f:
            M, alph, cksum, mapc = mp.model_header(f.read())
        rows = formats.read_msa(afa)["rows"]
        assert cksum is not None and alignment_checksum(alph, rows) == cksum == mp.checksum(rows, alph), afa
    d, s = mp.part_inputs("planted", 0), mp.part_inputs("planted_sto", 0)
    assert d["rows"] != s["rows"] and alignment_checksum("dna", s["rows"]) == d["cksum"] == alignment_checksum("dna", d["rows"])
    assert alignment_checksum("dna", mp.part_inputs("mismatch", 0)["rows"]) != d["cksum"]
    with pytest.raises(RuntimeError) as ei:
        alignment_checksum("dna", ["AC!T"])
    assert "wh_alignment_checksum" in str(ei.value)


def test_alignment_readers(tmp_path):
    p = mp.load_fixture("planted")[0]
    names, rows, _ = mp.parse_alignment(p["aln"])
    afa = tmp_path / "a.afa"
    afa.write_text("".join(">%s some words\n%s\n%s\n" % (n, r[:10], r[10:]) for n, r in zip(names, rows)))      # wrapped lines
    got = formats.read_msa(str(afa))
    assert got["names"] == names and got["rows"] == rows and got["desc"] == {}
    sto = tmp_path / "a.sto"
    sto.write_text(mp.load_fixture("planted_sto")[0]["aln"])                                  # interleaved blocks of 20 columns
    got = formats.read_msa(str(sto))
    assert got["names"] == names and got["rows"] == [r.upper().replace("-", ".") for r in rows]
    assert got["desc"] == {"r0": "the first row of the probe"}
    one = tmp_path / "a.pfam"
    one.write_text("# STOCKHOLM 1.0\n#=GF ID x\n#=GS r1 DE  two  words \n" + "".join("%s  %s\n" % z for z in zip(names, rows)) +
                   "#=GC RF " + "x" * len(rows[0]) + "\n//\n")                                 # one line per row
    got = formats.read_msa(str(one))
    assert got["names"] == names and got["rows"] == rows and got["desc"] == {"r1": "two  words"}
    ragged = tmp_path / "r.afa"
    ragged.write_text(">a\nAC-T\n>b\nACT\n")
    with pytest.raises(ValueError):
        formats.read_msa(str(ragged))
    empty = tmp_path / "e.afa"
    empty.write_text("")
    with pytest.raises(ValueError):
        formats.read_msa(str(empty))


def test_format_msa_rows_without_pp_and_gs_lines():
    text = formats.format_msa(["bb1", "n1"], ["AC-g", "A-Tg"], [None, "9.88"], "9.8.", "xxx.", desc={"bb1": "a backbone row"})
    assert text == ("# STOCKHOLM 1.0\n\n#=GS bb1 DE a backbone row\n\n"
                    "bb1          AC-g\nn1           A-Tg\n#=GR n1  PP  9.88\n#=GC PP_cons 9.8.\n#=GC RF      xxx.\n//\n")
    assert formats.format_msa(["bb1", "n1"], ["AC-g", "A-Tg"], [None, "9.88"], "9.8.", "xxx.", "afa", desc={"bb1": "a backbone row"}) == \
        ">bb1 a backbone row\nAC-g\n>n1\nA-Tg\n"
    # without either the text is what it was
    assert formats.format_msa(["seq1"], ["AC-g"], ["99.*"], "99..", "xxx.") == formats.format_stockholm("seq1", "AC-g", pp="99*")


class StubMapaliBackend:
    """A backend whose align_msa hands back a fixture part's matrices, and refuses an alignment with another checksum."""

    def __init__(self, name, i=0):
        self.part, self.d, self.calls = mp.load_fixture(name)[i], mp.part_inputs(name, i), []

    def align(self, jobs):
        raise AssertionError("the single-sequence path was taken")

    def align_msa(self, hmm_path, records, trim=False, mapali=None):
        from witch_amd.ehmm import alignment_checksum
        from witch_amd.shim.server import MapaliMismatch
        self.calls.append((hmm_path, [n for n, _ in records], trim, mapali))
        assert mapali is not None and [n for n, _ in records] == self.part["names"] and [t for _, t in records] == self.part["seqs"]
        if alignment_checksum(self.d["alph"], mapali[1]) != self.d["cksum"]:
            raise MapaliMismatch()
        assert list(mapali[0]) == self.d["names"] and list(mapali[1]) == self.d["rows"]
        rows, pps, cons, rf = mr.parse_msa(self.part["out"]["trim" if trim else "sto"])
        b = lambda t: np.frombuffer(t.encode(), dtype=np.uint8)      # noqa: E731
        return {"W": len(cons), "rows": mr.matrix(rows, self.d["names"] + self.part["names"]), "pp_rows": mr.matrix(pps, self.part["names"]),
                "pp_cons": b(cons), "rf": b(rf), "matmap": None, "pathless": 0}


def _files(part, tmp_path):
    aln = tmp_path / ("aln.sto" if part["aln_format"] == "stockholm" else "aln.afa")
    aln.write_text(part["aln"])
    fa = tmp_path / "new.fa"
    fa.write_text("".join(">%s\n%s\n" % z for z in zip(part["names"], part["seqs"])))
    return mp.hmm_file(part, tmp_path), aln.name, str(fa)


@pytest.mark.parametrize("name", ["planted", "planted_sto", "one_new"])
def test_run_hmmalign_mapali_writes_the_binary_text(name, tmp_path):
    """All four forms, to stdout and with -o; one_new: a sequence file with ONE record takes this path under --mapali."""
    from witch_amd.shim.server import Server
    backend = StubMapaliBackend(name)
    part = backend.part
    hmm, aln, fa = _files(part, tmp_path)
    srv = Server(backend, str(tmp_path / "s.sock"))
    assert srv.run_hmmalign(["--mapali", aln, hmm, fa], str(tmp_path)) == part["out"]["sto"]
    assert srv.run_hmmalign(["--mapali", aln, "-o", "out.sto", hmm, fa], str(tmp_path)) == ""
    assert (tmp_path / "out.sto").read_text() == part["out"]["sto"]
    assert srv.run_hmmalign(["--trim", "--mapali", aln, hmm, fa], str(tmp_path)) == part["out"]["trim"] and backend.calls[-1][2] is True
    assert srv.run_hmmalign(["--mapali", aln, "--outformat", "Pfam", hmm, fa], str(tmp_path)) == part["out"]["pfam"]
    assert srv.run_hmmalign(["--outformat", "afa", "--mapali", aln, hmm, fa], str(tmp_path)) == part["out"]["afa"]


def test_checksum_mismatch_is_hmmers_message(tmp_path):
    from witch_amd.shim.server import ArgError, Server
    backend = StubMapaliBackend("one_new")
    bad = mp.load_fixture("mismatch")[0]
    hmm, aln, fa = _files(bad, tmp_path)
    with pytest.raises(ArgError) as ei:                      # (the server answers an ArgError with exit status 1 and its text)
        Server(backend, str(tmp_path / "s.sock")).run_hmmalign(["--mapali", aln, hmm, fa], str(tmp_path))
    assert str(ei.value) + "\n" == bad["stderr"].replace("ALN", aln) and bad["status"] == 1
    with pytest.raises(ArgError) as ei:
        Server(backend, str(tmp_path / "s.sock")).run_hmmalign(["--mapali", "nowhere.afa", hmm, fa], str(tmp_path))
    assert "--mapali" in str(ei.value) and "nowhere.afa" in str(ei.value)


def test_without_mapali_the_backend_is_called_as_before(tmp_path):
    """The stub of tests/test_msa_host.py accepts (hmm_path, records, trim) and nothing else; a file with one record and no
    --mapali keeps the batched single-sequence path."""
    from tests.test_msa_host import _server
    srv, backend, fx, fa = _server("dna_planted", tmp_path)
    assert srv.run_hmmalign([fx["hmm_path"], fa], str(tmp_path)) == fx["out"]["sto"]
    assert srv.run_hmmalign(["--trim", fx["hmm_path"], fa], str(tmp_path)) == fx["out"]["trim"]

    class Single:
        def __init__(self):
            self.jobs = []

        def align(self, jobs):
            self.jobs += jobs
            return [(3, np.array([0, 1, 2], dtype=np.int32), np.array([0.9, 0.9, 0.9], dtype=np.float32)) for _ in jobs]

        def align_msa(self, *a, **k):
            raise AssertionError("a single record without --mapali took the alignment path")
    from witch_amd.shim.server import Server
    one = tmp_path / "one.fa"
    one.write_text(">q\nACG\n")
    b = Single()
    out = Server(b, str(tmp_path / "t.sock")).run_hmmalign([mp.hmm_file(mp.load_fixture("one_new")[0], tmp_path), str(one)], str(tmp_path))
    assert len(b.jobs) == 1 and out == formats.format_stockholm("q", "ACG", pp=[0.9, 0.9, 0.9])


def test_a_backend_without_align_msa_refuses_mapali(tmp_path):
    from witch_amd.shim.server import ArgError, Server

    class Old:
        def align(self, jobs):
            raise AssertionError("--mapali was ignored")
    part = mp.load_fixture("one_new")[0]
    hmm, aln, fa = _files(part, tmp_path)
    with pytest.raises(ArgError) as ei:
        Server(Old(), str(tmp_path / "s.sock")).run_hmmalign(["--mapali", aln, hmm, fa], str(tmp_path))
    assert "--mapali" in str(ei.value)


def test_abi_error_paths_without_a_device():
    import ctypes as C
    from witch_amd import _lib
    L = _lib.lib()
    W, npl = C.c_int64(0), C.c_int64(0)
    ptrs = [C.c_void_p(None) for _ in range(5)]
    out = [C.byref(W)] + [C.byref(p) for p in ptrs] + [C.byref(npl)]
    assert L.wh_msa_mapali(None, None, None, None, 0, 0, 0, None, 0, 0, *out) == _lib.WH_EINVAL
    assert L.wh_last_error().startswith(b"wh_msa_mapali:")
    assert L.wh_msa_mapali_dev(None, None, None, None, None, 0, 0, 0, 0, None, 0, 0, *out, None) == _lib.WH_EINVAL
    assert L.wh_last_error().startswith(b"wh_msa_mapali_dev:")
    assert all(p.value is None for p in ptrs)
    ck, present = C.c_uint32(0), C.c_int32(0)
    assert L.wh_ehmm_cksum(None, 0, C.byref(ck), C.byref(present)) == _lib.WH_EINVAL and L.wh_last_error().startswith(b"wh_ehmm_cksum:")
    assert L.wh_alignment_checksum(b"dna", None, 1, 4, C.byref(ck)) == _lib.WH_EINVAL
    assert L.wh_alignment_checksum(b"xna", b"ACGT", 1, 4, C.byref(ck)) == _lib.WH_EINVAL and b"xna" in L.wh_last_error()
    assert L.wh_alignment_checksum(b"dna", b"ACGT", 1, 4, C.byref(ck)) == 0 and ck.value == mp.checksum(["ACGT"], "dna")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "witch_hip.h")).read()
    for sym in ("wh_msa_mapali(", "wh_msa_mapali_dev(", "wh_alignment_checksum(", "wh_ehmm_cksum("):
        assert sym in header, sym
