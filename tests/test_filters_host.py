"""hmmsearch's acceleration filters, host side (no GPU): the scalar pipeline of wh_filter_host against the stage outcomes
of the reference's bundled hmmsearch (tests/golden/filters, written by tests/golden/make_golden_filters.py), its error
paths, and the level-0 hmmsearch's filtered command line.

These fixtures' outcomes are those of hmmsearch --nobias.  The bias filter is an explicit opt-in (WH_BIAS_FILTER_ON,
DESIGN.md section 4.11) with fixtures and tests of its own (tests/golden/filters_bias, tests/test_filters_bias_host.py, which
also reads the "Tb" and "bias_nats" recorded here); what is tested below is that nobias = 0 stays refused.  Models at
every size class of wh_filter.hip: tests/test_filters_classes_host.py."""
import os

import numpy as np
import pytest

from tests.filters_common import FIXTURES, MAX_SKIP, filter_host, fixture, msv_tjb


@pytest.mark.parametrize("name", FIXTURES)
def test_stage_outcomes_and_counts_equal_the_binary(name):
    """Stages 1 - 3 have integer scores: wh_filter_host's outcomes are the binary's on every fixture pair, at HMMER's
    default thresholds and at a second triple, except pairs whose recorded threshold lies within its own bisection
    bracket of the F in use (at most 1 % of a case); the summary's "Passed" counts follow."""
    fx = fixture(name)
    for key in ("default", "alt"):
        rc, stage, bias, msv, vit, cnt = filter_host(fx.paths, fx.res, fx.off, fx.F(key))
        assert rc == 0
        near = fx.near(key)
        assert near.sum() <= MAX_SKIP * fx.nq * fx.H
        for st, bit in ((0, 1), (1, 2), (2, 4)):
            got = (stage & bit) != 0
            exp = fx.expected(key, st) != 0
            bad = (got != exp) & ~near
            assert not bad.any(), (name, key, st, np.argwhere(bad)[:5].tolist())
        assert not bias.any()
        if not near.any():
            for h, m in enumerate(fx.models):
                assert [int(((stage[:, h] & b) != 0).sum()) for b in (1, 2, 4)] == m["counts"][key][:3], (name, key, h)
            assert cnt.tolist() == [fx.nq * fx.H] + [int(((stage & b) != 0).sum()) for b in (1, 2, 4)]
        # the Viterbi sweep runs exactly where the pair is past stage 2 and not below F2 already
        ran = (stage & 8) != 0
        assert not (ran & ((stage & 2) == 0)).any()
        assert ((vit == -32769) == ~ran).all()


@pytest.mark.parametrize("name", FIXTURES)
def test_msv_raw_scores_equal_the_recovered_integers(name):
    """Every pair passes at F1 = 1; where the binary's P-value can be inverted (1 - P above 1e-9, no overflow) the fixture
    holds round((usc + 3) scale) = xJ - tjb - base (the inversion lands within 0.25 of an integer, half the distance at
    which rounding would become ambiguous; near P = 1 it loses digits): the scalar filter's own."""
    fx = fixture(name)
    rc, stage, bias, msv, vit, cnt = filter_host(fx.paths, fx.res, fx.off, (1.0, 1.0, 1.0))
    assert rc == 0 and ((stage & 7) == 7).all()
    n = 0
    for h, m in enumerate(fx.models):
        for q, p in enumerate(m["pairs"]):
            if p["msv_int"] is None:
                continue
            assert p["msv_resid"] < 0.25
            assert int(msv[q, h]) - msv_tjb(len(fx.seqs[q])) - 190 == p["msv_int"], (name, h, q)
            n += 1
    assert n >= 5, n


def test_fixtures_hold_degenerate_queries_and_an_overflow():
    """The edge cases are in the fixtures: queries with X / N and an IUPAC pair code, and pairs that overflow the MSV filter
    (they pass at every threshold: T1's bracket is the bisection's floor)."""
    for name, codes in (("amino_hmmbuild", "XB"), ("dna_hmmbuild", "NR")):
        fx = fixture(name)
        degen = [t for n, t in zip(fx.qnames, fx.qtext) if n.endswith("_degen")]
        assert len(degen) == 3 and all(c in t for t in degen for c in codes)
        K = 20 if fx.alphabet == 2 else 4
        assert any((s >= K).any() for s in fx.seqs)
    fx = fixture("dna_hmmbuild")
    rc, stage, bias, msv, vit, cnt = filter_host(fx.paths, fx.res, fx.off, fx.F("default"))
    over = msv == -1
    assert over.any()
    for q, h in np.argwhere(over):
        assert fx.models[h]["pairs"][q]["T1"][1] == fx.g["ln_lo"] and stage[q, h] & 7 == 7 and not stage[q, h] & 8


def test_a_model_without_stats_cannot_be_filtered(tmp_path):
    from witch_amd import _lib
    fx = fixture("dna_synth")
    text = [ln for ln in open(fx.paths[0]) if not ln.startswith("STATS LOCAL VITERBI")]
    p = tmp_path / "nostats.hmm"
    p.write_text("".join(text))
    rc = filter_host([fx.paths[1], str(p)], fx.res, fx.off, (0.02, 1e-3, 1e-5))[0]
    msg = _lib.lib().wh_last_error().decode()
    assert rc == _lib.WH_EINVAL and "nostats.hmm" in msg and "STATS LOCAL VITERBI" in msg


def test_plain_filtered_search_is_refused_with_the_gap_named():
    """The one remaining gap: HMMER's bias filter.  nobias = 0 (and a NULL options pointer, HMMER's defaults) is refused."""
    from witch_amd import _lib
    fx = fixture("dna_synth")
    rc = filter_host(fx.paths, fx.res, fx.off, (0.02, 1e-3, 1e-5), nobias=0)[0]
    assert rc == _lib.WH_EINVAL and "bias filter is not implemented" in _lib.lib().wh_last_error().decode()
    assert _lib.lib().wh_filter(None, None, None, 0, None, None, None, None, None) < 0
    assert _lib.lib().wh_score_filtered(None, None, None, 0, None, None, None, None, None, None) < 0


def test_thresholds_of_one_switch_a_stage_off():
    fx = fixture("lowcomplexity")
    stage = filter_host(fx.paths, fx.res, fx.off, (1.0, 1e-3, 1e-5))[1]
    assert ((stage & 3) == 3).all() and ((stage & 4) == 0).any()
    stage = filter_host(fx.paths, fx.res, fx.off, (0.02, 1.0, 1e-5))[1]
    assert (((stage & 1) != 0) == ((stage & 4) != 0)).all() and not (stage & 8).any()


# ---- the level-0 hmmsearch --------------------------------------------------------------------------------------
def _server(tmp_path, calls):
    from witch_amd.shim import formats
    from witch_amd.shim.server import Server

    class Backend:
        last_passed = (2, 2, 1, 1)

        def search(self, hmm_path, records, **kw):
            calls.append(kw)
            hdr = formats.hmm_header(hmm_path)
            rows = [(n, 20.5, 0.1, 1) for n, _ in records][:1 if kw.get("filters") else None]
            return hdr, rows

    (tmp_path / "m.hmm").write_text("HMMER3/f [3.1b2 | February 2015]\nNAME  A_0_7\nLENG  12\nALPH  DNA\n"
                                    "STATS LOCAL FORWARD  -4.2 0.71\nHMM  A C G T\n")
    (tmp_path / "q.fa").write_text(">q1\nACGTACGTAC\n>q2\nACGTTT\n")
    srv = Server.__new__(Server)
    srv.backend = Backend()
    return srv


def test_shim_accepts_the_filtered_command_line(tmp_path):
    from witch_amd.shim.server import ArgError, check_hmmsearch_options, filter_thresholds, parse_hmmsearch_argv
    opts = parse_hmmsearch_argv("--cpu 1 --noali -E 99999999 --nobias -o o m q".split())[0]
    check_hmmsearch_options(opts)
    assert filter_thresholds(opts) == (0.02, 1e-3, 1e-5)
    opts = parse_hmmsearch_argv("--noali -E 99999999 --nobias --F1 0.3 --F2 0.05 --F3 1e-3 m q".split())[0]
    check_hmmsearch_options(opts)
    assert filter_thresholds(opts) == (0.3, 0.05, 1e-3)
    # with --max the four options are ignored, as in HMMER
    opts = parse_hmmsearch_argv("--max --nobias --F1 0.3 -E 99999999 m q".split())[0]
    check_hmmsearch_options(opts)
    assert filter_thresholds(opts) is None
    # plain filtered search (HMMER's bias filter) stays refused, and the message says why
    with pytest.raises(ArgError) as ei:
        check_hmmsearch_options(parse_hmmsearch_argv("--noali -E 99999999 m q".split())[0])
    assert "bias filter" in str(ei.value) and "--nobias" in str(ei.value)
    for bad in ("--nobias --F1 x m q", "--nobias --F2 -1 m q"):
        with pytest.raises(ArgError):
            check_hmmsearch_options(parse_hmmsearch_argv(bad.split())[0])
    calls = []
    srv = _server(tmp_path, calls)
    out = srv.run_hmmsearch("--nobias --F1 0.3 -E 99999999 m.hmm q.fa".split(), str(tmp_path))
    assert calls == [{"filters": (0.3, 1e-3, 1e-5)}]
    lines = out.splitlines()
    i = lines.index("Target sequences:                          2")
    assert lines[i + 1] == "Passed MSV filter:                        2  (1); expected 0.6 (0.3)"
    assert lines[i + 2] == "Passed bias filter:                       2  (1); expected 0.6 (0.3)"
    assert lines[i + 3] == "Passed Vit filter:                        1  (0.5); expected 0.0 (0.001)"
    assert lines[i + 4] == "Passed Fwd filter:                        1  (0.5); expected 0.0 (1e-05)"
    assert " q1 " in out and " q2 " not in out


def test_shim_output_with_max_is_what_it_was(tmp_path):
    """--max: the backend is called as ever (no filter argument), the filter options change nothing, and the text is the
    writer's unfiltered output byte for byte (no "Passed" lines)."""
    from witch_amd.shim import formats
    calls = []
    srv = _server(tmp_path, calls)
    plain = srv.run_hmmsearch("--max -E 99999999 m.hmm q.fa".split(), str(tmp_path))
    same = srv.run_hmmsearch("--max --nobias --F1 0.5 --F3 1e-9 -E 99999999 m.hmm q.fa".split(), str(tmp_path))
    assert calls == [{}, {}] and plain == same and "Passed" not in plain
    hdr = formats.hmm_header(str(tmp_path / "m.hmm"))
    rows = [("q1", 20.5, 0.1, 1), ("q2", 20.5, 0.1, 1)]
    assert plain == formats.format_hmmsearch(str(tmp_path / "m.hmm"), str(tmp_path / "q.fa"), hdr, rows, 2)
    assert plain.endswith("Target sequences:                          2\n//\n[ok]\n")


def test_filter_kernels_use_no_scratch():
    """The compiler's own report for wh_filter.hip (no GPU): every instantiation of the filter kernel, the long-model
    kernel and the count kernel keep their state in registers - no scratch."""
    import re
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "witch_amd", "csrc", "wh_filter.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-c", src, "-o", os.devnull], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == 8 and sum("filter_kernelILi" in n for n in names) == 6, names
    assert not any(scratch), list(zip(names, scratch))
