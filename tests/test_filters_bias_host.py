"""hmmsearch's bias filter, host side (no GPU): the logarithm that host and device share, wh_filter_host with
WH_BIAS_FILTER_ON against the stage outcomes of the reference's bundled hmmsearch run WITHOUT --nobias
(tests/golden/filters_bias, written by tests/golden/make_golden_filters_bias.py), the opt-in's error paths, and the Python
and level-0 switches."""
import math
import os

import numpy as np
import pytest

from tests.filters_bias_common import BIAS_FIXTURES, BIAS_ON, bias_fixture
from tests.filters_common import MAX_SKIP, filter_host, fixture

LOG2 = 0.69314718055994529


def test_filter_log_equals_the_float64_logarithm_rounded_once():
    """filter_log (float64 + - x / alone) against (float) log((double) x) of the host's libm on every float32 in
    [2^-2, 2^2): no difference."""
    from witch_amd import _lib
    first = int(np.float32(0.25).view(np.uint32))
    last = int(np.float32(4.0).view(np.uint32)) - 1
    assert last - first + 1 == 4 << 23
    assert _lib.lib().wh_filter_log_differences(first, last) == 0


@pytest.mark.parametrize("name", BIAS_FIXTURES)
def test_bias_stage_outcomes_and_counts_equal_the_binary(name):
    """MSV, bias and Viterbi stage outcomes are the binary's on every fixture pair, at HMMER's default thresholds and at
    (0.3, 0.05, 1e-3), except pairs whose recorded Tb / T2b lies within its own bisection bracket of the F in use (at most
    1 % of a case); the Viterbi sweep ran where the binary's output says it did; the summary's "Passed" counts follow.
    "nocompo" is a model file whose COMPO line was removed (the binary was run on that file)."""
    fx = bias_fixture(name)
    for key in ("default", "alt"):
        rc, stage, bias, msv, vit, cnt = filter_host(fx.paths, fx.res, fx.off, fx.F(key), nobias=BIAS_ON)
        assert rc == 0
        near = fx.near(key)
        assert near.sum() <= MAX_SKIP * fx.nq * fx.H
        for st, bit in ((0, 1), (1, 2), (2, 4)):
            bad = (((stage & bit) != 0) != (fx.expected(key, st) != 0)) & ~near
            assert not bad.any(), (name, key, st, np.argwhere(bad)[:5].tolist())
        known, ran = fx.viterbi_ran(key)
        got_ran = (stage & 8) != 0
        bad = known & ~near & (got_ran != ran)
        assert not bad.any(), (name, key, "ran", np.argwhere(bad)[:5].tolist())
        assert ((vit == -32769) == ~got_ran).all() and not (got_ran & ((stage & 2) == 0)).any()
        # the stage's score is reported exactly where the stage ran: for the pairs past the MSV stage
        assert not bias[(stage & 1) == 0].any()
        if not near.any():
            for h, m in enumerate(fx.models):
                assert [int(((stage[:, h] & b) != 0).sum()) for b in (1, 2, 4)] == m["counts"][key][:3], (name, key, h)
            assert cnt.tolist() == [fx.nq * fx.H] + [int(((stage & b) != 0).sum()) for b in (1, 2, 4)]


def test_the_fixtures_are_decided_by_the_bias_stage():
    """The stage decides on a large share of the pairs of dna_lowcomplexity: the binary's counts with and without --nobias
    differ for every model, and our two pipelines differ on the same pairs."""
    fx = bias_fixture("dna_lowcomplexity")
    assert fx.alphabet == 0 and fx.nq == 303 and sum(n.endswith("_degen") for n in fx.qnames) == 3
    for m in fx.models:
        for key in ("default", "alt"):
            assert m["counts"][key] != m["counts_nobias"][key]
    F = fx.F("alt")
    on = filter_host(fx.paths, fx.res, fx.off, F, nobias=BIAS_ON)[1]
    off = filter_host(fx.paths, fx.res, fx.off, F, nobias=1)[1]
    for h, m in enumerate(fx.models):
        assert int(((off[:, h] & 2) != 0).sum()) == m["counts_nobias"]["alt"][1] > m["counts"]["alt"][1] == int(((on[:, h] & 2) != 0).sum())


@pytest.mark.parametrize("name", ["amino_hmmbuild", "lowcomplexity"])
def test_bias_nats_lie_within_what_the_recorded_p_values_resolve(name):
    """tests/golden/filters records filtersc - null1 for the pairs on which the bias stage's P decides, recovered from the
    bisection bracket Tb of that P: bias = usc - x(P) ln 2 - null1 with usc from the recovered MSV integer and x the
    inverse of the MSV Gumbel.  The bracket's two ends bound the value; ours must lie between them, widened by 4e-6 nat:
    HMMER forms (usc - filtersc) / ln 2 in float32 from float32 terms of magnitude up to 16 nat (one ulp: 1e-6) and 8
    nat (5e-7), and the quotient is rounded once more (up to 25 bits: 2e-6 bit = 1.3e-6 nat)."""
    old, fx = fixture(name), bias_fixture(name)
    assert old.qtext == fx.qtext
    rc, stage, bias, msv, vit, cnt = filter_host(old.paths, old.res, old.off, (1.0, 1.0, 1.0), nobias=BIAS_ON)
    assert rc == 0 and ((stage & 3) == 3).all()
    scale = 3.0 / LOG2
    n, worst = 0, 0.0
    for h, m in enumerate(old.models):
        mu, lam = m["mu_lambda"]["MSV"]
        for q, p in enumerate(m["pairs"]):
            if p.get("bias_nats") is None:
                continue
            L = len(old.seqs[q])
            nullone = L * math.log(L / (L + 1.0)) + math.log(1.0 / (L + 1.0))
            usc = p["msv_int"] / scale - 3.0
            ends = [usc - (mu - math.log(-math.log1p(-math.exp(t))) / lam) * LOG2 - nullone for t in p["Tb"]]
            got = float(bias[q, h])
            assert min(ends) - 4e-6 <= got <= max(ends) + 4e-6, (name, h, q, got, ends)
            worst = max(worst, abs(got - p["bias_nats"]))
            n += 1
    print("%s: %d recorded values, largest |ours - recorded| %.3g nat" % (name, n, worst))
    assert n >= 30


def test_the_opt_in_leaves_nobias_as_it_was_and_refusals_in_place():
    """nobias = 1 runs as before (no bias score, bias passes with MSV) on the raw scores that the stage-on call computes too;
    nobias = 0 is still refused with the message that names the gap, and a value that is neither 1 nor WH_BIAS_FILTER_ON
    is WH_EINVAL."""
    from witch_amd import _lib
    fx = bias_fixture("lowcomplexity")
    F = fx.F("alt")
    rc1, stage1, bias1, msv1, vit1, cnt1 = filter_host(fx.paths, fx.res, fx.off, F, nobias=1)
    rc2, stage2, bias2, msv2, vit2, cnt2 = filter_host(fx.paths, fx.res, fx.off, F, nobias=BIAS_ON)
    assert rc1 == 0 and rc2 == 0
    assert not bias1.any() and (((stage1 & 1) != 0) == ((stage1 & 2) != 0)).all()
    assert (msv1 == msv2).all() and ((stage1 & 1) == (stage2 & 1)).all()
    for h, m in enumerate(fx.models):
        assert [int(((stage1[:, h] & b) != 0).sum()) for b in (1, 2, 4)] == m["counts_nobias"]["alt"][:3]
    both = (vit1 != -32769) & (vit2 != -32769)
    assert both.any() and (vit1[both] == vit2[both]).all()
    assert _lib.BIAS_FILTER_ON == BIAS_ON
    rc = filter_host(fx.paths, fx.res, fx.off, F, nobias=0)[0]
    assert rc == _lib.WH_EINVAL and "bias filter is not implemented" in _lib.lib().wh_last_error().decode()
    for bad in (3, -1):
        rc = filter_host(fx.paths, fx.res, fx.off, F, nobias=bad)[0]
        assert rc == _lib.WH_EINVAL and "WH_BIAS_FILTER_ON" in _lib.lib().wh_last_error().decode()


def test_python_refuses_bias_together_with_nobias():
    from witch_amd import _lib
    from witch_amd.ehmm import EHMM
    with pytest.raises(ValueError):
        EHMM.filter_opts(True, nobias=True, bias=True)
    assert EHMM.filter_opts(True, bias=True).nobias == _lib.BIAS_FILTER_ON
    assert EHMM.filter_opts((0.3, 0.05, 1e-3), nobias=True).nobias == 1
    assert EHMM.filter_opts(True).nobias == 0          # the default is unchanged: the library refuses it


def _server(tmp_path, calls):
    from witch_amd.shim import formats
    from witch_amd.shim.server import Server

    class Backend:
        last_passed = (2, 1, 1, 1)

        def search(self, hmm_path, records, **kw):
            calls.append(kw)
            return formats.hmm_header(hmm_path), [(n, 20.5, 0.1, 1) for n, _ in records][:1]

    (tmp_path / "m.hmm").write_text("HMMER3/f [3.1b2 | February 2015]\nNAME  A_0_7\nLENG  12\nALPH  DNA\n"
                                    "STATS LOCAL FORWARD  -4.2 0.71\nHMM  A C G T\n")
    (tmp_path / "q.fa").write_text(">q1\nACGTACGTAC\n>q2\nACGTTT\n")
    srv = Server.__new__(Server)
    srv.backend = Backend()
    return srv


def test_shim_runs_the_plain_filtered_line_only_with_the_switch(tmp_path, monkeypatch):
    """WITCH_HIP_BIAS_FILTER=1 in the server's environment: the plain filtered line (no --max, no --nobias) is accepted and
    the backend gets bias=True; a --nobias line gets no such keyword; the summary's bias line carries its own count.
    Without the variable the line is refused as before."""
    from witch_amd.shim.server import ArgError
    calls = []
    srv = _server(tmp_path, calls)
    monkeypatch.delenv("WITCH_HIP_BIAS_FILTER", raising=False)
    with pytest.raises(ArgError) as ei:
        srv.run_hmmsearch("--noali -E 99999999 m.hmm q.fa".split(), str(tmp_path))
    assert "bias filter" in str(ei.value) and "--nobias" in str(ei.value) and calls == []
    monkeypatch.setenv("WITCH_HIP_BIAS_FILTER", "1")
    out = srv.run_hmmsearch("--noali -E 99999999 m.hmm q.fa".split(), str(tmp_path))
    srv.run_hmmsearch("--noali --nobias --F1 0.3 -E 99999999 m.hmm q.fa".split(), str(tmp_path))
    srv.run_hmmsearch("--max -E 99999999 m.hmm q.fa".split(), str(tmp_path))
    assert calls == [{"filters": (0.02, 1e-3, 1e-5), "bias": True}, {"filters": (0.3, 1e-3, 1e-5)}, {}]
    lines = out.splitlines()
    i = lines.index("Target sequences:                          2")
    assert lines[i + 1].startswith("Passed MSV filter:                        2 ")
    assert lines[i + 2].startswith("Passed bias filter:                       1 ")


def test_bias_filter_kernels_use_no_scratch():
    """The compiler's own report for wh_filter.hip compiled with the bias stage (no GPU): every instantiation of the filter
    kernel and the long-model kernel keep their state in registers - no scratch."""
    import re
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "witch_amd", "csrc", "wh_filter.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-DWH_FILTER_BIAS=1",
                        "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == 7 and sum("filter_kernelILi" in n for n in names) == 6, names
    assert not any(scratch), list(zip(names, scratch))
