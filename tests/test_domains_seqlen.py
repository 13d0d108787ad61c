"""The domain stage under the sequence's length model on the GPU (EHMM.set_domain_length_model("sequence")) and the level-0
server with WITCH_HIP_DOMAIN_SEQLEN=1, against the float64 reference of tests/domains_seqlen_reference.py and HMMER's own
lines (tests/golden/domains, tests/golden/display).

What does not depend on the alignment (env_*, bits, bias_bits, lnP, index, of, pair) is the default setting's, bit for bit;
the coordinates are the reference's - HMMER's - on every domain, acc within wh_align_pp's bound of the reference."""
import os

import numpy as np
import pytest

from tests import display_reference as ref
from tests import domains_reference as dr
from tests import domains_seqlen_reference as sr
from tests import test_display_gpu as tdg
from tests.conftest import load_case
from tests.test_align_pp import _need_gpu
from tests.test_domains import _by_pair, _check_against_reference

pytestmark = pytest.mark.gpu

ALIGNED = ("ali_i", "ali_j", "hmm_i", "hmm_j", "oasc")


@pytest.mark.parametrize("name", dr.CASES)
def test_domain_stage_under_the_sequence_model(name):
    _need_gpu()
    from witch_amd.ehmm import EHMM, pack_queries
    case = load_case(name)
    fx = dr.load_fixture(name)
    seqs, want = sr.reference_seqlen(name)
    paths = case.hmm_paths[:len(fx["models"])]
    e = EHMM(paths)
    res, offs = pack_queries(seqs)
    deci, flags, det = e.score(res, offs, want_detail=True)
    assert e.domain_length_model == "envelope"
    a, off_a = e.domains(res, offs, flags, det)
    e.set_domain_length_model("sequence")
    assert e.domain_length_model == "sequence"
    b, off_b = e.domains(res, offs, flags, det)
    recs, _, env_off, cols, pp = e.domain_paths(res, offs, flags, det)
    e.set_domain_length_model("envelope")
    c, off_c = e.domains(res, offs, flags, det)
    e.close()
    assert np.array_equal(off_a, off_b) and np.array_equal(off_a, off_c) and len(a) == len(b) > 0
    assert a.tobytes() == c.tobytes(), "switching the setting back does not restore the default records"
    assert recs.tobytes() == b.tobytes()
    for k in a.dtype.names:
        if k not in ALIGNED:
            assert a[k].tobytes() == b[k].tobytes(), k
    assert any(a[k].tobytes() != b[k].tobytes() for k in ALIGNED[:4]), "no coordinate changed"
    got = _by_pair(b, off_b, len(seqs), len(paths))
    # coordinates identical to the reference on every domain, acc within 2e-4 + 3e-6 Ld (tests/test_domains.py's check)
    assert _check_against_reference(name + " sequence model", got, want, paths) > 0
    st = dr.compare_with_fixture(name, got, multi_from=want)
    assert st["weak_coord_differ"] == 0 and st["weak"] > 0
    assert st["strong"] > 0 and not st["strong_rule_misses"] and dr.multi_class_ok(st)
    # the stage's columns are the reference's, residue for residue
    d = 0
    for key in sorted(want):
        for w in want[key]:
            assert np.array_equal(cols[env_off[d]:env_off[d + 1]], w["cols"]), (name, key, w["index"])
            d += 1
    assert d == len(b)


# ------------------------------------------------------------------------------------------------ level 0
def _backend(monkeypatch, seqlen):
    from witch_amd.shim.server import GpuBackend, Server
    monkeypatch.setenv("WITCH_HIP_ALIDISPLAY", "1")
    if seqlen:
        monkeypatch.setenv("WITCH_HIP_DOMAIN_SEQLEN", "1")
    else:
        monkeypatch.delenv("WITCH_HIP_DOMAIN_SEQLEN", raising=False)
    srv = Server.__new__(Server)
    srv.backend = GpuBackend(0)
    return srv


def _close(srv):
    for _, e, _ in srv.backend.cache.values():
        e.close()
    srv.backend.cache.clear()


def test_display_against_the_binary_with_one_alignment_launch(tmp_path, monkeypatch):
    """tests/test_display_gpu.py's comparison against the binary's display section (its default run), the server started with
    WITCH_HIP_DOMAIN_SEQLEN=1 and WITCH_HIP_ALIDISPLAY=1: the three lines HMMER's bytes, no PP character beyond the bound
    outside the recorded lists - from one alignment launch per search, where the default setting needs two."""
    _need_gpu()
    from witch_amd.ehmm import pack_queries
    srv = _backend(monkeypatch, True)
    assert srv.backend.seqlen
    runs = []
    for case_name in ref.MODELS:
        fx, case = ref.load_fixture(case_name), load_case(case_name)
        names = fx["queries"]
        fa = tmp_path / (case_name + ".fa")
        fa.write_text("".join(">%s\n%s\n" % (n, s) for n, s in zip(names, case.qseqs[:len(names)])))
        for model in fx["models"]:
            hp = case.hmm_paths[model["h"]]
            e, _ = srv.backend.model(hp)
            assert e.domain_length_model == "sequence"
            seqs = [e.digitize(s.upper()) for s in case.qseqs[:len(names)]]
            res, offs = pack_queries(seqs)
            deci, flags, det = e.score(res, offs, want_detail=True)
            dom, dom_off, env_off, cols, pp = e.domain_paths(res, offs, flags, det)
            r = model["runs"]["default"]
            e.set_timing(True)
            text = srv.run_hmmsearch(["--max", "-E", "99999999"] + r["args"] + [hp, str(fa)], str(tmp_path))
            launches = e.last_kernel_ms(2)[1]
            e.set_timing(False)
            assert srv.backend.calls == ["domain_paths"], srv.backend.calls
            assert 1 <= launches == e.last_kernel_ms(5)[1] - 3, "the last alignment launches are not the domain stage's"
            _, ours, order = ref.parse_section(ref.section(text))
            _, theirs, order_t = ref.parse_section(r["section"])
            assert order == order_t
            post = {}
            for q, name in enumerate(names):
                nd = 0
                for d in range(int(dom_off[q]), int(dom_off[q + 1])):
                    if int(dom[d]["ali_i"]) and float(dom[d]["lnP"]) <= ref.ln_thr(10.0, max(int((flags[:, 0] & 1).sum()), 1)):
                        nd += 1
                        a = int(env_off[d]) + int(dom[d]["ali_i"] - dom[d]["env_i"])
                        post[(name, nd)] = (pp[a:a + int(dom[d]["ali_j"] - dom[d]["ali_i"]) + 1], int(dom[d]["env_j"] - dom[d]["env_i"]) + 1)
            runs.append((case_name, model["h"], "default", theirs, ours, model["ref_mismatch"]["default"], post))
    _close(srv)
    n = sum(1 for _ in tdg._compared(runs))
    n_all = sum(len(t["domains"]) for _, _, _, theirs, _, _, _ in runs for t in theirs.values())
    print("sequence model: %d of HMMER's %d displayed domains compared (the coordinates are HMMER's, outside the recorded lists)" % (n, n_all))
    assert n > 0
    tdg.test_pp_line_against_the_binary(runs)
    for case_name, h, run, name, d, his, mine, _ in tdg._compared(runs):
        for x, y in zip(his[1:], mine[1:]):
            if not x.endswith(" PP"):
                assert x == y, (case_name, h, name, d, x, y)


def _domtbl(srv, hp, fa, cwd, tag):
    srv.run_hmmsearch(["--noali", "-E", "99999999", "--max", "-o", tag + ".out", "--domtblout", tag + ".dom", hp, fa], cwd)
    return [ln for ln in open(os.path.join(cwd, tag + ".dom")).read().splitlines() if not ln.startswith("#")]


def test_domtblout_weak_lines_become_hmmers(tmp_path, monkeypatch):
    """hmmsearch --domtblout on dna_hmmbuild/A_0_0: with WITCH_HIP_DOMAIN_SEQLEN=1 a weak-stratum line whose score, bias and
    E-value fields agree with HMMER's as printed is HMMER's line byte for byte; their number is not below the default's.  The
    default's display search makes the padded-envelope pass, this one does not."""
    _need_gpu()
    case = load_case("dna_hmmbuild")
    m = dr.load_fixture("dna_hmmbuild")["models"][0]
    hp, fa = case.hmm_paths[0], os.path.join(case.dir, "queries.fasta")
    printed = (6, 7, 8, 11, 12, 13, 14)
    count = {}
    for seqlen in (False, True):
        srv = _backend(monkeypatch, seqlen)
        body = _domtbl(srv, hp, fa, str(tmp_path), "s%d" % seqlen)
        srv.run_hmmsearch(["-E", "99999999", "--max", "-o", "ali%d.out" % seqlen, hp, fa], str(tmp_path))
        assert srv.backend.calls == ["domain_paths"] + ([] if seqlen else ["sequence_model_posteriors"])
        _close(srv)
        n, same, boundary, weak, weak_same = dr.check_strong_lines(body, m["lines"])
        assert n > 0 and same + boundary == n
        agree = 0
        for b, ln in zip(body, m["lines"]):
            if float(ln["acc"]) < 0.95 and all(b.split()[c] == ln["raw"].split()[c] for c in printed):
                agree += 1
                if seqlen:
                    assert b == ln["raw"], (b, ln["raw"])
        count[seqlen] = (weak, weak_same, agree)
    print("weak lines %d: byte-identical to HMMER's %d by default, %d under the sequence model (%d agree in the printed score fields)" %
          (count[True][0], count[False][1], count[True][1], count[True][2]))
    assert count[True][1] >= count[False][1] and count[True][1] == count[True][2] > 0
