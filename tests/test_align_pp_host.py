"""Per-residue posterior probabilities, the parts that need no GPU: the reference of tests/pp_reference.py is pinned to
hmmalign's own PP characters (fixture: tests/golden/align_pp, written by tests/golden/make_golden_pp.py from the
reference's bundled hmmalign), formats.pp_char at its boundaries, and formats.format_stockholm(..., pp=...) against
hmmalign's stored files byte for byte."""
import numpy as np
import pytest

from tests import pp_reference as ppr
from tests.conftest import load_case
from witch_amd.shim import formats

FULL_CASES = ["dna_hmmbuild", "amino_hmmbuild"]


@pytest.mark.parametrize("name", FULL_CASES)
def test_reference_digits_equal_hmmalign_on_every_residue(name):
    """The float64 reference reproduces hmmalign's PP character on every residue of the two full cases - match, insert,
    N and C residues alike.  This pins the reference (and the encoding rule) like test_oracle_golden.py pins the oracle."""
    pairs = ppr.case_reference(name)
    case = load_case(name)
    assert len(pairs) == len(case.qseqs) * len(case.hmm_paths)
    n = 0
    kinds = set()
    for q, h, cols, digits, ref in pairs:
        assert len(digits) == len(case.qseqs[q]) == len(ref)
        mine = "".join(formats.pp_char(p) for p in ref)
        assert mine == digits, (name, q, h)
        assert np.all(ref >= 0.0) and np.all(ref <= 1.0 + 1e-12)
        st, _ = ppr.path_states(cols)
        kinds.update(int(s) for s in st)
        n += len(digits)
    assert kinds == {0, 1, 2, 3}, "the case must hold match, insert, N and C residues"
    assert n > 10000


def test_stored_columns_are_the_golden_columns():
    """The columns read from the stored Stockholm files (RF line) are the case's recorded hmmalign columns."""
    for name in FULL_CASES:
        case = load_case(name)
        if "align" not in case.g:
            continue
        for q, h, cols, _, _ in ppr.case_reference(name):
            row = ppr.parse_stockholm(ppr.load_fixture(name)["pairs"][q * len(case.hmm_paths) + h]["sto"])[1]
            assert np.array_equal(cols, np.array(formats.decode_stockholm_row(row), dtype=np.int32))


def test_pp_char_boundaries():
    """HMMER's rule: '*' when p + 0.05 >= 1, else the digit floor((p + 0.05) * 10)."""
    assert formats.pp_char(0.0) == "0" and formats.pp_char(1.0) == "*" and formats.pp_char(1.0 + 1e-6) == "*"
    chars = "0123456789*"
    for d in range(10):                    # the boundary between chars[d] and chars[d + 1] lies at 0.05 + d / 10
        b = 0.05 + d / 10.0
        assert formats.pp_char(b - 1e-9) == chars[d], (d, b)
        assert formats.pp_char(b + 1e-9) == chars[d + 1], (d, b)
        assert formats.pp_char(np.float32(b - 1e-4)) == chars[d] and formats.pp_char(np.float32(b + 1e-4)) == chars[d + 1]
    for p, c in ((0.04, "0"), (0.06, "1"), (0.5, "5"), (0.849, "8"), (0.851, "9"), (0.949, "9"), (0.951, "*")):
        assert formats.pp_char(p) == c


@pytest.mark.parametrize("name", FULL_CASES)
def test_format_stockholm_reproduces_hmmalign_files(name):
    """From the stored columns and characters, format_stockholm writes hmmalign's file byte for byte at hmmalign's width
    of 200; at a short width the same lines come out in several blocks."""
    case = load_case(name)
    fx = ppr.load_fixture(name)
    M = [formats.hmm_header(p)["M"] for p in case.hmm_paths]
    multi_block = 0
    for rec, (q, h, cols, digits, _) in zip(fx["pairs"], ppr.case_reference(name)):
        assert not formats.hmm_has_rf(case.hmm_paths[h])
        row = formats.stockholm_row(case.qseqs[q], cols, M[h], flank_at_end=True)
        text = formats.format_stockholm(case.qnames[q], row, 200, pp=digits)
        assert text == rec["sto"], (name, q, h)
        multi_block += len(row) > 200
        # short width: every block carries the four lines, the blocks concatenate to the one-block lines
        short = formats.format_stockholm(case.qnames[q], row, 37, pp=digits)
        assert ppr.parse_stockholm(short) == ppr.parse_stockholm(rec["sto"])
        assert short.count("#=GC RF") == -(-len(row) // 37) == short.count("#=GR") == short.count("#=GC PP_cons")
        assert short.count("\n\n") == -(-len(row) // 37)           # one blank line in front of every block, none before "//"
    if name == "amino_hmmbuild":
        assert multi_block > 0, "no stored file with a second block at width 200"


def test_format_stockholm_from_probabilities_and_without_pp():
    """Probabilities are encoded by pp_char; pp=None is the sequence-only output the shim wrote before."""
    case = load_case("dna_hmmbuild")
    rec = ppr.load_fixture("dna_hmmbuild")["pairs"][0]
    q, h, cols, digits, ref = ppr.case_reference("dna_hmmbuild")[0]
    M = formats.hmm_header(case.hmm_paths[h])["M"]
    row = formats.stockholm_row(case.qseqs[q], cols, M, flank_at_end=True)
    assert formats.format_stockholm(case.qnames[q], row, 200, pp=ref) == rec["sto"]
    assert formats.format_stockholm(case.qnames[q], row, 200, pp=ref.astype(np.float32), rf=False) == \
        "".join(l + "\n" for l in rec["sto"].splitlines() if not l.startswith("#=GC RF"))
    plain = formats.format_stockholm(case.qnames[q], row)
    assert plain == "# STOCKHOLM 1.0\n\n%s %s\n\n//\n" % (case.qnames[q], row)
    assert plain == formats.format_stockholm(case.qnames[q], row, 200, pp=None)


def test_long_model_fixture_matches_its_recipe(tmp_path):
    """The 1 900-node model and its four queries are regenerated from the seeds in the fixture: the stored hmmalign rows
    spell the regenerated queries, and the share of residues on which hmmalign's character differs from the reference's -
    from which the log-space pairs' cap derives - is the one the generator recorded."""
    from oracle import oracle as orc
    from witch_amd import synth
    fx = ppr.load_fixture("long_model")
    fam, hp = ppr.long_model(fx["spec"], str(tmp_path))
    names, seqs, kinds = ppr.long_queries(fx["spec"], fam)
    assert kinds == ["fragment", "fragment", "multicopy", "multicopy"] == [p["kind"] for p in fx["pairs"]]
    assert all(150 <= p["L"] <= 400 for p in fx["pairs"][:2])
    model = ppr.Model(orc.OracleHMM(hp))
    differ, total = {}, {}
    for s, kind, name, rec in zip(seqs, kinds, names, fx["pairs"]):
        n, row, pp, _, rf = ppr.parse_stockholm(rec["sto"])
        assert n == name and row.replace("-", "").replace(".", "").upper() == synth.to_text(s.astype(np.int64), "dna").upper()
        cols, digits = ppr.row_cols_digits(row, pp, rf)
        ref = ppr.path_posteriors(model, s, cols)
        differ[kind] = differ.get(kind, 0) + sum(1 for a, b in zip(digits, ref) if a != formats.pp_char(b))
        total[kind] = total.get(kind, 0) + len(s)
    assert {k: differ[k] / total[k] for k in total} == fx["hmmalign_vs_reference_share"]
    assert all(v <= 0.005 for v in fx["hmmalign_vs_reference_share"].values())


@pytest.mark.parametrize("alphabet", ["dna", "amino"])
def test_window_fixture_reference_digits_equal_hmmalign(alphabet, tmp_path):
    """The node-window inputs (700-node models, regenerated from their seeds): the reference's characters are hmmalign's."""
    paths, names, seqs = ppr.window_case(alphabet, str(tmp_path))
    for q, h, cols, digits, ref in ppr.fixture_reference("window_" + alphabet, paths, seqs):
        assert len(digits) == len(seqs[q]) and "".join(formats.pp_char(p) for p in ref) == digits, (alphabet, q, h)
