"""hmmalign for a file of several sequences, the parts that need no GPU: the numpy assembly (tests/msa_reference.py) against
the bundled binary's own matrices, format_msa against its text, run_hmmalign's multi-sequence path over a stub backend, and
the error paths of wh_msa / wh_msa_dev.  Fixtures: tests/golden/msa (tests/golden/make_golden_msa.py)."""
import os

import numpy as np
import pytest

from tests import msa_reference as mr
from witch_amd.shim import formats

OPTIONS = [("sto", "Stockholm", False), ("trim", "Stockholm", True), ("pfam", "Pfam", False), ("afa", "afa", False)]


def _assembled(name, trim):
    """The reference assembly from the columns and PP characters decoded from the binary's default output."""
    M, names, texts, cols, digits, _ = mr.fixture_inputs(name)
    return mr.assemble(M, cols, [mr.midpoints(d) for d in digits], texts, trim=trim)


@pytest.mark.parametrize("name", mr.CASES)
@pytest.mark.parametrize("key,fmt,trim", OPTIONS[:3])
def test_reference_assembly_reproduces_the_binary(name, key, fmt, trim):
    """Rows, PP rows and RF byte for byte.  PP_cons: '.' exactly where the binary has it; elsewhere the binary's character lies
    between the characters of the smallest and the largest mean the sequences' PP characters allow (a character tells its
    posterior to within its interval only, so the mean is known to within the mean of the intervals)."""
    fx = mr.load_fixture(name)
    M, names, texts, cols, digits, _ = mr.fixture_inputs(name)
    rows, pps, cons, rf = mr.parse_msa(fx["out"][key])
    got = _assembled(name, trim)
    assert got["W"] == len(rf) and got["rf"].tobytes().decode() == rf
    assert np.array_equal(got["rows"], mr.matrix(rows, names))
    assert np.array_equal(got["pp_rows"], mr.matrix(pps, names))
    assert got["pathless"] == 0
    assert np.array_equal(got["matmap"], np.array([i for i, c in enumerate(rf) if c == "x"]))
    lo, hi = mr.cons_interval(M, cols, digits)
    ours = got["pp_cons"].tobytes().decode()
    for k, at in enumerate(got["matmap"]):
        want = cons[at]
        assert (want == ".") == (lo[k] == ".") == (ours[at] == "."), (name, key, k)
        if want != ".":
            assert mr.CHARS.index(lo[k]) <= mr.CHARS.index(want) <= mr.CHARS.index(hi[k]), (name, key, k, lo[k], want, hi[k])
            assert mr.CHARS.index(lo[k]) <= mr.CHARS.index(ours[at]) <= mr.CHARS.index(hi[k])
    ins = np.frombuffer(rf.encode(), dtype=np.uint8) != ord("x")
    assert np.all(got["pp_cons"][ins] == ord(".")) and all(cons[i] == "." for i in np.nonzero(ins)[0])


def test_fixtures_show_the_layout_rules():
    """What the planted case was built for is in the binary's output: a one-residue run in a wider block sits flush right, a
    two-residue run is split left / right, an N flank is right-justified beside an empty one, a C flank left-justified."""
    M, names, texts, cols, digits, (rows, pps, cons, rf) = mr.fixture_inputs("dna_planted")
    blocks = rf.split("x")
    widths = [len(b) for b in blocks]
    assert len(blocks) == M + 1 and widths[0] >= 5 and widths[M] >= 5 and max(widths[1:M]) >= 7
    k = int(np.argmax(widths[1:M])) + 1
    at = sum(widths[:k]) + k
    cells = {n: rows[n][at:at + widths[k]] for n in names}
    assert any(c.strip(".") and c[0] != "." and c[-1] != "." and "." in c for c in cells.values()), cells      # split run
    assert any(set(c) == {"."} for c in cells.values())
    n_cells = {n: rows[n][:widths[0]] for n in names}
    assert any(c.startswith(".") and not c.endswith(".") for c in n_cells.values()) and any(set(c) == {"."} for c in n_cells.values())
    c_cells = {n: rows[n][len(rf) - widths[M]:] for n in names}
    assert any(c.endswith(".") and not c.startswith(".") for c in c_cells.values())
    assert len(mr.load_fixture("dna_65")["names"]) == 65
    assert len(mr.fixture_inputs("sub30_two")[5][3]) > 1400 and mr.load_fixture("sub30_two")["out"]["sto"].count("#=GC RF") == 8


@pytest.mark.parametrize("name", mr.CASES)
@pytest.mark.parametrize("key,fmt,trim", OPTIONS)
def test_format_msa_is_the_binary_text(name, key, fmt, trim):
    fx = mr.load_fixture(name)
    names = fx["names"]
    rows, pps, cons, rf = mr.parse_msa(fx["out"]["trim" if trim else "sto"])
    text = formats.format_msa(names, mr.matrix(rows, names), mr.matrix(pps, names), np.frombuffer(cons.encode(), dtype=np.uint8), rf, fmt)
    assert text == fx["out"][key]
    assert formats.format_msa(names, [rows[n] for n in names], [pps[n] for n in names], cons, rf, fmt.upper()) == fx["out"][key]


def test_format_msa_refuses_other_formats_and_leaves_the_single_sequence_writer_alone():
    with pytest.raises(formats.FormatError):
        formats.format_msa(["a"], ["AC"], ["99"], "99", "xx", "a2m")
    with pytest.raises(formats.FormatError):
        formats.format_msa(["a"], ["AC"], ["99"], "99", "xx", "foo")
    # no RF line for a model that brings its own
    assert "#=GC RF" not in formats.format_msa(["a"], ["AC"], ["99"], "99", None)
    # one sequence through both writers: the same lines where the tags are as wide (names of four characters or more)
    one = formats.format_stockholm("seq1", "AC-g", pp="99*")
    assert one == formats.format_msa(["seq1"], ["AC-g"], ["99.*"], "99..", "xxx.")


class StubMsaBackend:
    """A backend with align_msa that hands back a fixture's matrices."""

    def __init__(self, name):
        self.name, self.calls = name, []

    def align(self, jobs):
        raise AssertionError("the single-sequence path was taken")

    def align_msa(self, hmm_path, records, trim=False):
        self.calls.append((hmm_path, [n for n, _ in records], trim))
        fx = mr.load_fixture(self.name)
        assert [n for n, _ in records] == fx["names"] and [t for _, t in records] == fx["seqs"]
        rows, pps, cons, rf = mr.parse_msa(fx["out"]["trim" if trim else "sto"])
        b = lambda t: np.frombuffer(t.encode(), dtype=np.uint8)      # noqa: E731
        return {"W": len(cons), "rows": mr.matrix(rows, fx["names"]), "pp_rows": mr.matrix(pps, fx["names"]), "pp_cons": b(cons),
                "rf": b(rf), "matmap": None, "pathless": 0}


def _server(name, tmp_path):
    from witch_amd.shim.server import Server
    fx = mr.load_fixture(name)
    fa = tmp_path / "in.fa"
    fa.write_text("".join(">%s\n%s\n" % (n, s) for n, s in zip(fx["names"], fx["seqs"])))
    backend = StubMsaBackend(name)
    return Server(backend, str(tmp_path / "s.sock")), backend, fx, str(fa)


def test_run_hmmalign_writes_the_binary_text(tmp_path):
    from witch_amd.shim.server import ArgError
    srv, backend, fx, fa = _server("dna_planted", tmp_path)
    hmm = fx["hmm_path"]
    assert srv.run_hmmalign([hmm, fa], str(tmp_path)) == fx["out"]["sto"]                    # stdout without -o
    assert srv.run_hmmalign(["-o", "out.sto", hmm, fa], str(tmp_path)) == ""
    assert (tmp_path / "out.sto").read_text() == fx["out"]["sto"]
    assert srv.run_hmmalign(["--trim", "-o", "trim.sto", hmm, fa], str(tmp_path)) == ""
    assert (tmp_path / "trim.sto").read_text() == fx["out"]["trim"] and backend.calls[-1][2] is True
    assert srv.run_hmmalign(["--outformat", "Pfam", hmm, fa], str(tmp_path)) == fx["out"]["pfam"]
    assert srv.run_hmmalign(["--outformat", "afa", hmm, fa], str(tmp_path)) == fx["out"]["afa"]
    n = len(backend.calls)
    with pytest.raises(ArgError) as ei:
        srv.run_hmmalign(["--outformat", "foo", hmm, fa], str(tmp_path))
    assert "foo is not a recognized output MSA file format" in str(ei.value) and len(backend.calls) == n
    empty = tmp_path / "empty.fa"
    empty.write_text("")
    with pytest.raises(ArgError) as ei:
        srv.run_hmmalign([hmm, str(empty)], str(tmp_path))
    assert "is empty or misformatted" in str(ei.value)


def test_a_backend_without_align_msa_keeps_the_refusal(tmp_path):
    from witch_amd.shim.server import ArgError, Server

    class Old:
        def align(self, jobs):
            raise AssertionError("not reached")
    fx = mr.load_fixture("dna_planted")
    fa = tmp_path / "in.fa"
    fa.write_text(">a\nACGT\n>b\nACGT\n")
    with pytest.raises(ArgError) as ei:
        Server(Old(), str(tmp_path / "s.sock")).run_hmmalign([fx["hmm_path"], str(fa)], str(tmp_path))
    assert str(ei.value) == "witch-hip hmmalign shim: exactly one sequence per call (got 2)"


def test_abi_error_paths_without_a_device():
    import ctypes as C
    from witch_amd import _lib
    L = _lib.lib()
    W, npl = C.c_int64(0), C.c_int64(0)
    ptrs = [C.c_void_p(None) for _ in range(5)]
    out = [C.byref(W)] + [C.byref(p) for p in ptrs] + [C.byref(npl)]
    assert L.wh_msa(None, None, None, None, 0, 0, 0, *out) == _lib.WH_EINVAL
    assert L.wh_last_error().startswith(b"wh_msa:")
    assert L.wh_msa_dev(None, None, None, None, None, 0, 0, 0, 0, *out, None) == _lib.WH_EINVAL
    assert L.wh_last_error().startswith(b"wh_msa_dev:")
    assert all(p.value is None for p in ptrs)
    assert (_lib.WH_MSA_TRIM, _lib.WH_MSA_NO_LDS) == (1, 2)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "witch_hip.h")).read()
    assert "#define WH_MSA_TRIM   1" in header and "#define WH_MSA_NO_LDS 2" in header
