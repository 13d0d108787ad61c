"""The domain records under the sequence's length model, host side (no GPU): the float64 reference of
tests/domains_seqlen_reference.py against hmmsearch's own --domtblout lines (tests/golden/domains), and the refusals of the
C ABI that need no device.

hmmsearch aligns an envelope under the length model of its whole sequence.  With that model the reference gives HMMER's
printed alignment on EVERY reportable domain of the three cases, the weak stratum (HMMER's acc < 0.95) included, where the
envelope's own length model (tests/test_domains_host.py) leaves columns at an end:

  case               strong / weak   coords differ, envelope model   sequence model   acc beyond 0.00501, envelope   sequence
  dna_hmmbuild         178 / 238              0 / 29                      0 / 0                  0 / 37                0 / 0
  amino_hmmbuild       100 /  90              0 / 13                      0 / 0                  1 / 16                0 / 0
  amino_multidomain     60 /   3              0 /  1                      0 / 0                  0 /  0                0 / 0

Both conditions are asserted on every domain of both strata, with no share left out.  0.00501: HMMER prints acc with two
decimals (half a unit, 0.005) and the reference is float64 where HMMER's posteriors are float32 (1e-5 covers their sum / Ld).
"""
import numpy as np
import pytest

from tests import domains_reference as dr
from tests import domains_seqlen_reference as sr

ACC_TOL = 0.00501
EXPECT = {"dna_hmmbuild": (178, 238), "amino_hmmbuild": (100, 90), "amino_multidomain": (60, 3)}


@pytest.mark.parametrize("name", dr.CASES)
def test_sequence_model_reference_is_hmmsearchs_alignment_on_every_domain(name):
    _, dom = sr.reference_seqlen(name)
    fxd = dr.fixture_domains(name)
    dom_z = [m["domZ"] for m in dr.load_fixture(name)["models"]]
    n = {"strong": 0, "weak": 0}
    worst = 0.0
    for key in sorted(set(fxd) | set(dom)):
        recs = [r for r in dom.get(key, []) if np.exp(r["lnP"]) * dom_z[key[1]] <= 10.0]
        lines = fxd.get(key, [])
        assert [(r["env_i"], r["env_j"]) for r in recs] == [(int(ln["env_from"]), int(ln["env_to"])) for ln in lines], (name, key)
        for r, ln in zip(recs, lines):
            stratum = "strong" if float(ln["acc"]) >= 0.95 else "weak"
            n[stratum] += 1
            got = (r["hmm_i"], r["hmm_j"], r["ali_i"], r["ali_j"])
            want = (int(ln["hmm_from"]), int(ln["hmm_to"]), int(ln["ali_from"]), int(ln["ali_to"]))
            assert got == want, (name, key, r["index"], stratum, got, want)
            dacc = abs(r["oasc"] / (r["env_j"] - r["env_i"] + 1) - float(ln["acc"]))
            worst = max(worst, dacc)
            assert dacc <= ACC_TOL, (name, key, r["index"], stratum, r["oasc"] / (r["env_j"] - r["env_i"] + 1), ln["acc"])
    print("[%s] sequence model: %d strong + %d weak domains, coordinates HMMER's on all, largest |acc - printed| %.5f" % (name, n["strong"], n["weak"], worst))
    assert (n["strong"], n["weak"]) == EXPECT[name]


@pytest.mark.parametrize("name", dr.CASES)
def test_compare_with_fixture_counts_no_weak_difference(name):
    """The project's own comparison (domains_reference.compare_with_fixture) on the new records: no weak-stratum coordinate
    differs, every acc is within 0.00501, and the score columns are what they were (they do not depend on the alignment)."""
    _, dom = sr.reference_seqlen(name)
    _, env = dr.case_reference(name)
    st = dr.compare_with_fixture(name, dom)
    st0 = dr.compare_with_fixture(name, env, out=lambda s: None)
    assert st["weak_coord_differ"] == 0
    assert st["strong_acc_5e3"] == st["strong"] and st["weak_acc_5e3"] == st["weak"]
    for k in ("strong", "weak", "strong_boundary", "weak_boundary", "strong_rule_misses", "weak_rule_misses", "multi", "multi_differ", "multi_two"):
        assert st[k] == st0[k], k


def test_the_paths_that_change_are_weak_domains_and_include_the_named_one():
    """Every case has domains whose path changes under the sequence's model (the GPU tests take their envelopes from these
    lists); rnd01 x dna_hmmbuild/A_0_0 is one.  (Over the reportable domains 43 coordinate tuples change: the weak-stratum
    differences of tests/test_domains_host.py's table, all of them; the lists here hold unreportable domains too.)"""
    from tests.conftest import load_case
    case = load_case("dna_hmmbuild")
    ch = sr.changed_domains("dna_hmmbuild")
    assert any(case.qnames[q] == "rnd01" and h == 0 for q, h, _ in ch), ch[:5]
    for name in dr.CASES:
        assert len(sr.changed_domains(name)) > 0, name


# ------------------------------------------------------------------------------------------------ C ABI, no device
def test_abi_refusals_without_a_device():
    from witch_amd import _lib
    L = _lib.lib()
    assert (_lib.WH_LENMODEL_ENVELOPE, _lib.WH_LENMODEL_SEQUENCE) == (0, 1)
    # an unknown model constant is refused before the handle is looked at, and a null handle after it
    assert L.wh_set_domain_length_model(None, 7) == _lib.WH_EINVAL
    assert b"unknown length model 7" in L.wh_last_error()
    assert L.wh_set_domain_length_model(None, _lib.WH_LENMODEL_SEQUENCE) == _lib.WH_EINVAL
    assert b"null handle" in L.wh_last_error()
    assert L.wh_get_domain_length_model(None) == _lib.WH_EINVAL
    # a cfg_len entry below 1: refused by the host-pointer entry point, naming the query
    res = np.zeros(12, dtype=np.uint8)
    offs = np.array([0, 5, 12], dtype=np.int64)
    pq, ph = np.array([0, 1], dtype=np.int64), np.zeros(2, dtype=np.int32)
    cols = np.full(12, -9, dtype=np.int32)
    for bad in (0, -3):
        cfg = np.array([40, bad], dtype=np.int32)
        rc = L.wh_align_pp_len(None, res.ctypes.data, offs.ctypes.data, 2, pq.ctypes.data, ph.ctypes.data, 2, offs.ctypes.data,
                               cols.ctypes.data, None, cfg.ctypes.data)
        assert rc == _lib.WH_EINVAL
        msg = L.wh_last_error().decode()
        assert "cfg_len[1] = %d" % bad in msg and "query 1" in msg, msg
    assert np.all(cols == -9)
    # valid lengths pass that check (the null handle is what is refused next)
    cfg = np.array([40, 1], dtype=np.int32)
    assert L.wh_align_pp_len(None, res.ctypes.data, offs.ctypes.data, 2, pq.ctypes.data, ph.ctypes.data, 2, offs.ctypes.data,
                             cols.ctypes.data, None, cfg.ctypes.data) == _lib.WH_EINVAL
    assert "cfg_len" not in L.wh_last_error().decode()


def test_python_setter_refuses_an_unknown_name():
    from witch_amd.ehmm import EHMM
    e = EHMM.__new__(EHMM)          # no handle: the name is checked before the library is called
    e._h = None
    with pytest.raises(ValueError):
        e.set_domain_length_model("hmmalign")
    assert EHMM._LENGTH_MODELS == ("envelope", "sequence")
