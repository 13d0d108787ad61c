"""hmmsearch's alignment display without a GPU: the CPU restatement (tests/display_reference.py) with formats.format_alidisplay
against the bundled binary's section (tests/golden/display), the opt-in of the level-0 server (WITCH_HIP_ALIDISPLAY=1 and no
--noali) with fake backends, its refusals, and the consensus getter.

Against the binary: the section's title, the sequences and their order, and - on every domain outside the fixture's
ref_mismatch list - every line under the "== domain" header byte for byte: wrapped blocks with their coordinates, --notextw,
--textw 150, --domE 1e-10.  The listed domains are weak ones (HMMER acc < 0.95; DESIGN.md section 4.10: hmmsearch trims
columns at an end of such alignments).  The header line itself carries two numbers of the domain TABLE, its score and its
conditional E-value; it is compared byte for byte too, except where it differs by the table's own print-boundary rule
(tests/domains_reference.check_strong_lines: a score one printed unit apart, an E-value that differs in its last printed
digit) - counted and printed: 2 of 664 headers (dna_hmmbuild model 2 q000000, 67.650 bits printed 67.6 / 67.7;
amino_hmmbuild model 1 q000008, 2.2e-23 / 2.1e-23)."""
import numpy as np
import pytest

from tests import display_reference as ref
from tests.conftest import load_case

RUN_KW = {"default": {}, "notextw": {"textw": None}, "textw150": {"textw": 150}, "domE": {"domE": 1e-10}}


# ------------------------------------------------------------------------------------------------ 1. against the binary
def _header_boundary(mine, theirs):
    """Two "== domain" headers that differ only by a print boundary of the score ("%.1f": one unit) or of the E-value
    ("%.2g": one unit of its last printed digit)."""
    a, b = mine.split(), theirs.split()
    if len(a) != len(b) or a[:4] != b[:4] or a[5:8] != b[5:8] or len(a) != 9:
        return False
    sa, sb, ea, eb = float(a[4]), float(b[4]), float(a[8]), float(b[8])
    if abs(sa - sb) > 0.1001:
        return False
    if ea == eb:
        return True
    lo = min(abs(ea), abs(eb))
    return lo > 0 and abs(ea - eb) <= 1.1 * 10 ** (np.floor(np.log10(lo)) - 1)


@pytest.mark.parametrize("case_name", list(ref.MODELS))
def test_reference_reproduces_the_binary(case_name):
    fx = ref.load_fixture(case_name)
    n_dom = n_same = n_head = n_wrapped = 0
    for model in fx["models"]:
        for run, r in model["runs"].items():
            mine = ref.case_section(case_name, model["h"], **RUN_KW[run])
            title, theirs, order = ref.parse_section(r["section"])
            title_m, ours, order_m = ref.parse_section(mine)
            assert title_m == title == "Domain annotation for each sequence (and alignments):"
            assert order_m == order, (case_name, model["h"], run)
            listed = model["ref_mismatch"][run]
            # the recorded list is what differs, and all of it is weak
            assert ref.differing_domains(mine, r["section"]) == listed, (case_name, model["h"], run)
            for name, d in listed:
                acc = theirs[name]["acc"].get(d)
                assert acc is not None and acc < 0.95, (case_name, model["h"], run, name, d, acc)
            for name in order:
                t, o = theirs[name], ours[name]
                assert sorted(t["domains"]) == sorted(o["domains"]) or any(n == name for n, _ in listed), (case_name, run, name)
                if not t["domains"]:                  # "No individual domains ...": the table says so, and nothing follows it
                    assert not o["domains"] and o["table"] == t["table"], (case_name, run, name)
                for d, lines in t["domains"].items():
                    if [name, d] in listed:
                        continue
                    n_dom += 1
                    assert o["domains"][d][1:] == lines[1:], (case_name, model["h"], run, name, d)
                    if o["domains"][d][0] == lines[0]:
                        n_same += 1
                    else:
                        assert _header_boundary(o["domains"][d][0], lines[0]), (o["domains"][d][0], lines[0])
                        n_head += 1
                    blocks = 1 + sum(1 for ln in lines[1:] if ln == "")
                    n_wrapped += blocks > 1
                    assert run != "notextw" or blocks == 1
    print("[%s] %d domains outside the recorded lists: alignment lines byte-identical on all, header identical on %d, at a print "
          "boundary on %d; %d of them wrapped into more than one block" % (case_name, n_dom, n_same, n_head, n_wrapped))
    assert n_dom > 0 and n_head <= 2 * len(fx["models"][0]["runs"])
    if case_name != "amino_hmmbuild":                  # (models of 99 nodes and less: one block at 120 columns)
        assert n_wrapped > 0


def test_layout_rules():
    """format_alidisplay by hand: names right-aligned to the longer, coordinates to the widest of the four, blocks of
    textw - name - 2 x coordinate - 5 columns but at least 40, per-block coordinates, a block without residues."""
    from witch_amd.shim import formats
    model, aseq = "a" * 130, "C" * 30 + "-" * 100
    out = formats.format_alidisplay("m", "query01", 7, 95, model, " " * 130, aseq, "9" * 30 + "." * 100, textw=120)
    # name width 7, coordinate width 3 (136, 124): 120 - 7 - 6 - 5 = 102 columns
    assert out[0] == "  %7s %3d %s %-3d" % ("m", 7, "a" * 102, 108)
    assert out[2] == "  query01  95 %s 124" % (aseq[:102])
    assert out[4] == "" and out[5] == "  %7s 109 %s 136" % ("m", "a" * 28)
    assert out[7] == "  query01   - %s   -" % ("-" * 28)
    assert out[8] == "  %7s %3s %s PP" % ("", "", "." * 28)
    one = formats.format_alidisplay("m", "query01", 7, 95, model, " " * 130, aseq, "9" * 30 + "." * 100, textw=None)
    assert len(one) == 4 and one[0].endswith(" 136")
    narrow = formats.format_alidisplay("m" * 90, "q", 1, 1, "a" * 50, " " * 50, "C" * 50, "9" * 50, textw=120)
    assert len(narrow) == 9 and narrow[0].split()[2] == "a" * 40          # (120 - 90 - 4 - 5 = 21: the floor of 40 holds)


# ------------------------------------------------------------------------------------------------ 2. the opt-in
HMM_HEAD = ("HMMER3/f [3.1b2 | February 2015]\nNAME  A_0_7\nLENG  12\nALPH  DNA\nRF    no\nMM    no\nCONS  yes\nCS    no\n"
            "STATS LOCAL FORWARD  -4.2 0.71\nHMM  A C G T\n")
LINES = ("acgtacgtacgt"[:9], "acgtacgta", "ACGTACGTA", "9********")


class Backend:
    """The fake backend of tests/test_domains_host.py, with the calls recorded and (subclass) the display method."""

    def __init__(self):
        self.calls = []

    def _doms(self, records):
        return {n: [{"index": 0, "of": 1, "env_i": 1, "env_j": len(t), "ali_i": 2, "ali_j": len(t), "hmm_i": 1, "hmm_j": 12,
                     "bits": 20.25, "bias_bits": 0.1, "oasc": 0.9 * len(t), "lnP": -17.0}] for n, t in records}

    def search(self, hmm_path, records, **kw):
        from witch_amd.shim import formats
        self.calls.append(("search", kw))
        rows = [(n, 20.5, 0.1, 1) for n, _ in records]
        return (formats.hmm_header(hmm_path), rows, self._doms(records)) if kw.get("want_domains") else (formats.hmm_header(hmm_path), rows)


class DisplayBackend(Backend):
    def search_display(self, hmm_path, records, display, inc=None, table=None, **kw):
        from witch_amd.shim import formats
        self.calls.append(("search_display", display, inc, table, kw))
        rows = [(n, 20.5, 0.1, 1, 20.5) for n, _ in records]
        return formats.hmm_header(hmm_path), rows, self._doms(records), None, None, {n: {0: LINES} for n, _ in records}


def _server(tmp_path, backend, head=HMM_HEAD):
    from witch_amd.shim.server import Server
    (tmp_path / "m.hmm").write_text(head)
    (tmp_path / "q.fa").write_text(">q1\nACGTACGTAC\n>q2\nACGTTT\n")
    srv = Server.__new__(Server)
    srv.backend = backend
    return srv


def test_opt_in_off_is_todays_output_and_calls(tmp_path, monkeypatch):
    monkeypatch.delenv("WITCH_HIP_ALIDISPLAY", raising=False)
    be = DisplayBackend()
    srv = _server(tmp_path, be)
    plain = srv.run_hmmsearch("--max -E 99999999 m.hmm q.fa".split(), str(tmp_path))
    noali = srv.run_hmmsearch("--max -E 99999999 --noali m.hmm q.fa".split(), str(tmp_path))
    # (what tests/test_domains_host.py pins for this backend and these files)
    assert plain == noali and be.calls == [("search", {}), ("search", {})] and ">>" not in plain
    dom = srv.run_hmmsearch("--max -E 99999999 --domtblout d.tbl m.hmm q.fa".split(), str(tmp_path))
    dom_noali = srv.run_hmmsearch("--max -E 99999999 --noali --domtblout d.tbl m.hmm q.fa".split(), str(tmp_path))
    assert dom == dom_noali and be.calls[2:] == [("search", {"want_domains": True})] * 2
    assert "Domain annotation for each sequence:\n" in dom and "== domain" not in dom and dom.count("\n>> ") == 2
    # --textw below 120 is not even read without the opt-in, as before
    assert srv.run_hmmsearch("--max -E 99999999 --textw 100 m.hmm q.fa".split(), str(tmp_path)) == plain
    # the variable with --noali: the same again, and any other value of the variable is "off"
    monkeypatch.setenv("WITCH_HIP_ALIDISPLAY", "1")
    assert srv.run_hmmsearch("--max -E 99999999 --noali m.hmm q.fa".split(), str(tmp_path)) == plain
    assert srv.run_hmmsearch("--max -E 99999999 --noali --domtblout d.tbl m.hmm q.fa".split(), str(tmp_path)) == dom
    monkeypatch.setenv("WITCH_HIP_ALIDISPLAY", "yes")
    assert srv.run_hmmsearch("--max -E 99999999 m.hmm q.fa".split(), str(tmp_path)) == plain
    assert all(c[0] == "search" for c in be.calls)


def test_opt_in_on_carries_the_section(tmp_path, monkeypatch):
    """Fails on the parent commit: there the variable changes nothing."""
    monkeypatch.setenv("WITCH_HIP_ALIDISPLAY", "1")
    be = DisplayBackend()
    srv = _server(tmp_path, be)
    out = srv.run_hmmsearch("--max -E 99999999 m.hmm q.fa".split(), str(tmp_path))
    assert be.calls == [("search_display", {"domE": 10.0, "domZ": None}, None, None, {})]
    assert "Domain annotation for each sequence (and alignments):\n>> q1  \n" in out
    want = ["  Alignments for each domain:", "  == domain 1  score: 20.2 bits;  conditional E-value: 8.3e-08",
            "  A_0_7  1 acgtacgta 9 ", "           acgtacgta", "     q1  2 ACGTACGTA 10", "           9******** PP", ""]
    lines = out.splitlines()
    at = lines.index("  Alignments for each domain:")
    assert lines[at:at + len(want)] == want
    assert out.count("  == domain 1") == 2 and out.rstrip().endswith("[ok]")
    # the tables around the alignments are those of the line with --noali --domtblout
    monkeypatch.delenv("WITCH_HIP_ALIDISPLAY")
    base = srv.run_hmmsearch("--max -E 99999999 --domtblout d.tbl m.hmm q.fa".split(), str(tmp_path)).splitlines()
    kept = [ln for ln in lines if not ln.startswith(("  Alignments for", "  == domain", "  A_0_7 ", "     q1 ", "     q2 ", " " * 11))]
    strip = lambda ls: [ln for ln in ls if ln != ""]      # noqa: E731
    assert strip(kept) == strip([ln.replace("each sequence:", "each sequence (and alignments):") for ln in base])
    # --domtblout on the same line: one backend call, the file as ever
    monkeypatch.setenv("WITCH_HIP_ALIDISPLAY", "1")
    both = srv.run_hmmsearch("--max -E 99999999 --domZ 7 --notextw --domtblout e.tbl m.hmm q.fa".split(), str(tmp_path))
    assert be.calls[-1][:2] == ("search_display", {"domE": 10.0, "domZ": 7.0}) and "== domain 1" in both
    assert [ln for ln in open(tmp_path / "e.tbl") if not ln.startswith("#")][0].split()[0] == "q1"


def test_refusals(tmp_path, monkeypatch):
    from witch_amd.shim.server import ArgError
    monkeypatch.setenv("WITCH_HIP_ALIDISPLAY", "1")
    srv = _server(tmp_path, DisplayBackend())
    with pytest.raises(ArgError, match="--textw takes integer arg in range n>=120; got 100"):
        srv.run_hmmsearch("--max -E 99999999 --textw 100 m.hmm q.fa".split(), str(tmp_path))
    assert "== domain" in srv.run_hmmsearch("--max -E 99999999 --textw 120 m.hmm q.fa".split(), str(tmp_path))
    with pytest.raises(ArgError, match="bad value for --domZ"):
        srv.run_hmmsearch("--max -E 99999999 --domZ 0 m.hmm q.fa".split(), str(tmp_path))
    with pytest.raises(ArgError, match="search_display"):
        _server(tmp_path, Backend()).run_hmmsearch("--max -E 99999999 m.hmm q.fa".split(), str(tmp_path))
    with pytest.raises(ArgError, match="RF yes"):
        _server(tmp_path, DisplayBackend(), HMM_HEAD.replace("RF    no", "RF    yes")).run_hmmsearch("--max -E 99999999 m.hmm q.fa".split(), str(tmp_path))
    with pytest.raises(ArgError, match="CS yes"):
        _server(tmp_path, DisplayBackend(), HMM_HEAD.replace("CS    no", "CS    yes")).run_hmmsearch("--max -E 99999999 m.hmm q.fa".split(), str(tmp_path))
    for head in (HMM_HEAD.replace("CONS  yes", "CONS  no"), HMM_HEAD.replace("CONS  yes\n", "")):
        with pytest.raises(ArgError, match="CONS no"):
            _server(tmp_path, DisplayBackend(), head).run_hmmsearch("--max -E 99999999 m.hmm q.fa".split(), str(tmp_path))
    # with --noali the same models are served as ever
    out = _server(tmp_path, DisplayBackend(), HMM_HEAD.replace("RF    no", "RF    yes")).run_hmmsearch(
        "--max -E 99999999 --noali m.hmm q.fa".split(), str(tmp_path))
    assert "[ok]" in out


# ------------------------------------------------------------------------------------------------ 3. the library's parser
@pytest.mark.parametrize("case_name,h", [("amino_hmmbuild", 0), ("dna_hmmbuild", 1)])
def test_consensus_getter_is_the_files_column(case_name, h):
    """The library's parser keeps the CONS column (wh_hmm_consensus: the handle-less twin of wh_ehmm_consensus, through the
    same parse_hmm_file - a handle needs a device; tests/test_display_gpu.py asks the handle).  Fails on the parent commit:
    the symbol does not exist."""
    from witch_amd.ehmm import hmm_consensus
    path = load_case(case_name).hmm_paths[h]
    want, keys = ref.consensus_column(path)
    got, got_keys = hmm_consensus(path)
    assert got == want and len(got) > 0 and got_keys == keys == {"CONS": True, "RF": False, "CS": False}
    assert any(c.islower() for c in got) and (case_name != "amino_hmmbuild" or any(c.isupper() for c in got))      # (the file's own case)


def test_consensus_getter_header_keys(tmp_path):
    """An edited copy of a fixture model: "RF yes" is reported, and a header without CONS has no consensus."""
    from witch_amd.ehmm import hmm_consensus
    text = open(load_case("dna_hmmbuild").hmm_paths[0]).read()
    p = tmp_path / "rf.hmm"
    p.write_text(text.replace("RF    no", "RF    yes"))
    assert hmm_consensus(p)[1] == {"CONS": True, "RF": True, "CS": False}
    p.write_text(text.replace("CONS  yes", "CONS  no"))
    assert hmm_consensus(p) == (None, {"CONS": False, "RF": False, "CS": False})
