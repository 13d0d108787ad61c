"""hmmsearch's bias filter on the device (wh_filter.hip compiled with the stage): wh_filter with WH_BIAS_FILTER_ON against the
scalar pipeline of wh_filter_host bit for bit, against the stage outcomes of the reference's bundled hmmsearch run without
--nobias (tests/golden/filters_bias), wh_score_filtered with the stage on, and the level-0 hmmsearch with WITCH's plain
filtered command line."""
import json
import os

import numpy as np
import pytest

from tests.filters_bias_common import BIAS_FIXTURES, BIAS_ON, bias_fixture
from tests.filters_common import MAX_SKIP, filter_host, pack
from tests.test_filters_gpu import K_OF, _ln_p_forward, _models

pytestmark = pytest.mark.gpu

# one model per register class of the filter kernel (2, 4, 8, 16, 32, 48 cells per lane) and one beyond them (one lane per pair)
CLASS_LENGTHS = [7, 200, 400, 1000, 2048, 3072, 3073]
# the edges of the 64-residue fetch and of the in-order sum of the rows' logarithms
QUERY_LENGTHS = [1, 2, 63, 64, 65, 127, 128, 129, 300]
THRESHOLDS = [(0.02, 1e-3, 1e-5), (0.3, 0.05, 1e-3), (1.0, 1.0, 1.0)]
LOG2 = 0.69314718055994529


def _bias_queries(alphabet, seed):
    """every length three times: random residues, low complexity (80 % from one or two letters), and random with degenerate
    codes (the 'any' code and a pair code) at the first, the last and two adjacent positions"""
    K, Kp = K_OF[alphabet]
    rng = np.random.default_rng(seed)
    seqs = []
    for L in QUERY_LENGTHS:
        seqs.append(rng.integers(0, K, size=L).astype(np.uint8))
        short = rng.choice(K, size=int(rng.integers(1, 3)), replace=False)
        lc = np.where(rng.random(L) < 0.8, rng.choice(short, size=L), rng.integers(0, K, size=L)).astype(np.uint8)
        seqs.append(lc)
        d = rng.integers(0, K, size=L).astype(np.uint8)
        d[0] = Kp - 3
        d[-1] = K + 1
        if L > 4:
            d[L // 2] = Kp - 3
            d[L // 2 + 1] = K + 1
        seqs.append(d)
    return seqs


def _same(e, paths, res, off, F):
    rc, stage, bias, msv, vit, cnt = filter_host(paths, res, off, F, nobias=BIAS_ON)
    assert rc == 0
    g_stage, g_bias, g_msv, g_vit = e.filter(res, off, filters=F, bias=True, want_raw=True)
    for name, a, b in (("msv_raw", g_msv, msv), ("vit_raw", g_vit, vit), ("stage", g_stage, stage)):
        assert (a == b).all(), (name, F, np.argwhere(a != b)[:5].tolist(), a[a != b][:5].tolist(), b[a != b][:5].tolist())
    diff = g_bias.view(np.uint32) != bias.view(np.uint32)
    assert not diff.any(), ("bias_nats", F, np.argwhere(diff)[:5].tolist(), g_bias[diff][:5].tolist(), bias[diff][:5].tolist())
    c = e.last_filter_counts()
    assert [c["pairs"], c["msv"], c["bias"], c["vit"], c["fwd"], c["scored"]] == cnt.tolist() + [0, 0]
    return stage, bias


@pytest.mark.parametrize("alphabet", ["dna", "amino"])
def test_bias_filter_equals_the_scalar_pipeline_on_every_class(alphabet, tmp_path):
    """Device == host, bit for bit: stage byte, filter_bias_nats, both raw scores - one model per register class and one of
    the long-model kernel in the same call, every query length around the 64-residue fetch, at three threshold triples."""
    from witch_amd.ehmm import EHMM
    paths, cons = _models(str(tmp_path), alphabet, CLASS_LENGTHS)
    seqs = _bias_queries(alphabet, 23)
    res, off = pack(seqs)
    e = EHMM(paths)
    try:
        assert e.M.tolist() == CLASS_LENGTHS
        for F in THRESHOLDS:
            stage, bias = _same(e, paths, res, off, F)
        # at F = 1 every pair runs the bias stage, which has a score of its own
        assert ((stage & 3) == 3).all() and (bias != 0).any(axis=0).all()
        # nobias = 1 on the same handle: the kernels without the stage, as before
        g_stage, g_bias = e.filter(res, off, filters=THRESHOLDS[1], nobias=True)
        ref = filter_host(paths, res, off, THRESHOLDS[1], nobias=1)
        assert (g_stage == ref[1]).all() and not g_bias.any()
    finally:
        e.close()


@pytest.mark.parametrize("name", BIAS_FIXTURES)
def test_bias_filter_on_the_fixtures(name):
    """Stage outcomes on the device equal the host's and the binary's, and the counts of wh_last_filter_counts are the
    fixture's "Passed" numbers."""
    from witch_amd.ehmm import EHMM
    fx = bias_fixture(name)
    e = EHMM(fx.paths)
    try:
        for key in ("default", "alt"):
            stage, bias = _same(e, fx.paths, fx.res, fx.off, fx.F(key))
            near = fx.near(key)
            assert near.sum() <= MAX_SKIP * fx.nq * fx.H
            for st, bit in ((0, 1), (1, 2), (2, 4)):
                bad = (((stage & bit) != 0) != (fx.expected(key, st) != 0)) & ~near
                assert not bad.any(), (name, key, st, np.argwhere(bad)[:5].tolist())
            if not near.any():
                c = e.last_filter_counts()
                want = np.sum([m["counts"][key] for m in fx.models], axis=0).tolist()
                assert [c["msv"], c["bias"], c["vit"]] == want[:3]
    finally:
        e.close()


def _record(name, worst):
    """profiles/filters_bias_mi355x.json: forward_stage_largest_ln_p_difference[fixture] (the file's other keys are
    tools/bench_filters.py --bias's, which keeps this one); a tree that cannot be written to is no failure of the test"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "filters_bias_mi355x.json")
    try:
        with open(path) as f:
            d = json.load(f)
    except (OSError, ValueError):
        d = {}
    rec = d.get("forward_stage_largest_ln_p_difference")
    rec = rec if isinstance(rec, dict) else {}
    rec[name] = float("%.3g" % worst)
    d["forward_stage_largest_ln_p_difference"] = rec
    try:
        with open(path, "w") as f:
            f.write(json.dumps(d, indent=1) + "\n")
    except OSError:
        pass


@pytest.mark.parametrize("name", BIAS_FIXTURES)
def test_score_filtered_with_the_bias_filter(name):
    """wh_score_filtered with the stage on: stages 1 - 3 and the Forward stage equal the binary's (pairs whose Tb / T2b /
    T3b lies within its own bracket of the F in use skipped, at most 1 %), survivors carry wh_score's results, rejected
    pairs WH_FLAG_FILTERED, the counts are the fixture's.  The largest |ln P_ours - ln P_recorded| at the Forward stage
    (P against the bias filter's score; T3b's upper end) stays within the 7e-4 of DESIGN.md section 4.11 - the stage adds
    one float32 rounding of bias_nats / ln 2 - and goes into profiles/filters_bias_mi355x.json."""
    from witch_amd import _lib
    from witch_amd.ehmm import EHMM
    fx = bias_fixture(name)
    e = EHMM(fx.paths)
    try:
        deci0, flags0, fwd0 = e.score(fx.res, fx.off, want_fwd=True)
        tau, lam, present = e.evparams()
        assert present.all()
        bias_all = e.filter(fx.res, fx.off, filters=(1.0, 1.0, 1.0), bias=True)[1]
        ours = fwd0 - (bias_all.astype(np.float64) / LOG2).astype(np.float32)
        worst = 0.0
        for h, m in enumerate(fx.models):
            for q, p in enumerate(m["pairs"]):
                hi = p["T3b"][1]
                if hi > fx.floor and hi < -1e-6 and np.isfinite(fwd0[q, h]):
                    worst = max(worst, abs(float(_ln_p_forward(ours[q:q + 1, h], tau[h], lam[h])[0]) - hi))
        print("%s: largest |ln P_ours - ln P_recorded| at the Forward stage, bias filter on: %.3g" % (name, worst))
        _record(name, worst)
        for key in ("default", "alt"):
            F = fx.F(key)
            deci, flags, fwd, stage = e.score(fx.res, fx.off, want_fwd=True, filters=F, bias=True, want_stage=True)
            near = fx.near(key, ("Tb", "T2b", "T3b"))
            assert near.sum() <= MAX_SKIP * near.size
            for st, bit in ((0, 1), (1, 2), (2, 4), (3, 16)):
                bad = (((stage & bit) != 0) != (fx.expected(key, st) != 0)) & ~near
                assert not bad.any(), (name, key, st, np.argwhere(bad)[:5].tolist())
            past3 = (stage & 4) != 0
            got4 = (stage & 16) != 0
            assert not (got4 & ~past3).any()
            assert (deci[got4] == deci0[got4]).all() and (flags[got4] == flags0[got4]).all()
            assert (fwd[got4].view(np.uint32) == fwd0[got4].view(np.uint32)).all()
            assert (flags[~got4] == _lib.FLAG_FILTERED).all() and (deci[~got4] == 0).all()
            c = e.last_filter_counts()
            kept = past3.any(axis=1)
            assert c["pairs"] == fx.nq * fx.H and c["scored"] == int(kept.sum()) * fx.H and c["fwd"] == int(got4.sum())
            assert [c["msv"], c["bias"], c["vit"]] == [int(((stage & b) != 0).sum()) for b in (1, 2, 4)]
            if not near.any():
                want = np.sum([m["counts"][key] for m in fx.models], axis=0).tolist()
                assert [c["msv"], c["bias"], c["vit"], c["fwd"]] == want
        assert worst <= 7e-4, worst
    finally:
        e.close()


def test_level0_hmmsearch_with_the_plain_filtered_line(tmp_path, monkeypatch):
    """The server with WITCH_HIP_BIAS_FILTER=1 and WITCH's filtered command line (no --max, no --nobias) lists exactly the
    binary's sequences on dna_lowcomplexity, and its four "Passed" numbers are the fixture's."""
    from witch_amd.shim.server import GpuBackend, Server
    monkeypatch.setenv("WITCH_HIP_BIAS_FILTER", "1")
    fx = bias_fixture("dna_lowcomplexity")
    h = 1                                     # the model on which the stage rejects most
    fa = tmp_path / "q.fa"
    fa.write_text("".join(">%s\n%s\n" % (n, t) for n, t in zip(fx.qnames, fx.qtext)))
    srv = Server.__new__(Server)
    srv.backend = GpuBackend(0)
    outs = {}
    try:
        for key, extra in (("default", []), ("alt", ["--F1", "0.3", "--F2", "0.05", "--F3", "1e-3"])):
            assert not fx.near(key, ("Tb", "T2b", "T3b"))[:, h].any()
            outs[key] = srv.run_hmmsearch(["--cpu", "1", "--noali", "-E", "99999999"] + extra + [fx.paths[h], str(fa)], str(tmp_path))
        full = srv.run_hmmsearch(["--cpu", "1", "--noali", "-E", "99999999", "--max", fx.paths[h], str(fa)], str(tmp_path))
    finally:
        for _, (_, eh, _) in srv.backend.cache.items():
            eh.close()

    def listed(text):
        names, on = [], False
        for ln in text.splitlines():
            if ln.lstrip().startswith("E-value"):
                on = True
            elif on and (ln.strip().startswith("---") or ln.strip().startswith("[")):
                continue
            elif on and not ln.strip():
                break
            elif on:
                names.append(ln.split()[8])
        return set(names)
    for key, out in outs.items():
        want = {n for n, p in zip(fx.qnames, fx.models[h]["pairs"]) if p["out"][key][3]}
        assert listed(out) == want & listed(full)
        counts = fx.models[h]["counts"][key]
        assert counts[1] < counts[0]
        for label, n in zip(("MSV", "bias", "Vit", "Fwd"), counts):
            assert ("Passed %s filter:" % label).ljust(28) + "%15d" % n in out
    assert "Passed" not in full
