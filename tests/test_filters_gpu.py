"""hmmsearch's acceleration filters on the device (wh_filter.hip): wh_filter against the scalar pipeline wh_filter_host bit
for bit, wh_score_filtered against the stage outcomes of the reference's bundled hmmsearch (tests/golden/filters) and
against wh_score, and the level-0 hmmsearch without --max."""
import math
import os

import numpy as np
import pytest

from tests.filters_common import FIXTURES, filter_host, fixture, pack

pytestmark = pytest.mark.gpu

K_OF = {"dna": (4, 18), "amino": (20, 29)}
# one model per register class of the filter kernel (2, 4, 8, 16, 32, 48 cells per lane: up to 128, 256, 512, 1 024,
# 2 048, 3 072 nodes) and every edge around a lane count
REG_LENGTHS = [1, 2, 63, 64, 65, 128, 129, 256, 512, 1000, 2048, 3072]
RUN_ALL_VIT = (1.0, 1e-12, 1.0)       # every pair passes MSV, and the Viterbi sweep runs unless the MSV filter overflowed


def _models(tmp, alphabet, lengths):
    from witch_amd import synth
    paths, cons = [], []
    for M in lengths:
        fam = synth.make_family(1000 + M, M, 4, alphabet, indel_rate=0.0)
        h = synth.build_hmm(fam, 0, 4, "syn%d" % M)
        assert h.M == M
        p = os.path.join(tmp, "syn_%s_%d.hmm" % (alphabet, M))
        synth.write_hmm(h, p)
        paths.append(p)
        cons.append(np.argmax(h.mat[1:], axis=1).astype(np.uint8))
    return paths, cons


def _queries(alphabet, lengths, seed):
    """random residues of the given lengths, one more of 150 with degenerate codes (the 'any' code and a pair code)"""
    K, Kp = K_OF[alphabet]
    rng = np.random.default_rng(seed)
    seqs = [rng.integers(0, K, size=L).astype(np.uint8) for L in lengths]
    d = rng.integers(0, K, size=150).astype(np.uint8)
    d[3::7] = Kp - 3
    d[5::11] = K + 1
    return seqs + [d]


def _same(e, paths, res, off, F):
    rc, stage, bias, msv, vit, cnt = filter_host(paths, res, off, F)
    assert rc == 0
    g_stage, g_bias, g_msv, g_vit = e.filter(res, off, filters=F, nobias=True, want_raw=True)
    for name, a, b in (("msv_raw", g_msv, msv), ("vit_raw", g_vit, vit), ("stage", g_stage, stage)):
        assert (a == b).all(), (name, F, np.argwhere(a != b)[:5].tolist(), a[a != b][:5].tolist(), b[a != b][:5].tolist())
    assert g_bias.view(np.uint32).tolist() == bias.view(np.uint32).tolist()
    c = e.last_filter_counts()
    assert [c["pairs"], c["msv"], c["bias"], c["vit"], c["fwd"], c["scored"]] == cnt.tolist() + [0, 0]
    return stage, msv, vit


@pytest.mark.parametrize("alphabet", ["dna", "amino"])
def test_filter_equals_the_scalar_pipeline_on_every_register_class(alphabet, tmp_path):
    from witch_amd.ehmm import EHMM
    paths, cons = _models(str(tmp_path), alphabet, REG_LENGTHS)
    seqs = _queries(alphabet, [1, 2, 150, 2000], 7)
    # a long exact copy of a model's consensus overflows its MSV filter
    i128 = REG_LENGTHS.index(128)
    seqs.append(np.tile(cons[i128], 5))
    seqs.append(np.tile(cons[REG_LENGTHS.index(1000)], 2)[:1500])
    res, off = pack(seqs)
    e = EHMM(paths)
    try:
        assert e.M.tolist() == REG_LENGTHS
        for F in ((0.02, 1e-3, 1e-5), RUN_ALL_VIT):
            stage, msv, vit = _same(e, paths, res, off, F)
        assert msv[len(seqs) - 2, i128] == -1 and stage[len(seqs) - 2, i128] == 7       # overflow: passes, no Viterbi sweep
        ran = (stage & 8) != 0
        assert (ran | (msv == -1)).all() and ran.any(axis=0).all()
    finally:
        e.close()


def test_filter_models_beyond_the_register_classes(tmp_path):
    """3 073 nodes: the scalar cores, one lane per pair, rows in HBM - beside a register-class model in the same call."""
    from witch_amd.ehmm import EHMM
    paths, cons = _models(str(tmp_path), "dna", [3073, 129])
    seqs = _queries("dna", [1, 2, 150], 11) + [cons[0][:300].copy()]
    res, off = pack(seqs)
    e = EHMM(paths)
    try:
        for F in ((0.02, 1e-3, 1e-5), RUN_ALL_VIT):
            stage, msv, vit = _same(e, paths, res, off, F)
        assert ((stage[:, 0] & 8) != 0).any()
    finally:
        e.close()


@pytest.mark.parametrize("name", FIXTURES)
def test_filter_equals_the_scalar_pipeline_on_the_fixtures(name):
    from witch_amd.ehmm import EHMM
    fx = fixture(name)
    e = EHMM(fx.paths)
    try:
        for key in ("default", "alt"):
            _same(e, fx.paths, fx.res, fx.off, fx.F(key))
    finally:
        e.close()


def _record_forward_difference(name, worst):
    """profiles/filters_mi355x.json: forward_stage_largest_ln_p_difference[fixture] (the file's other keys are
    tools/bench_filters.py's, which keeps this one); a tree that cannot be written to is no failure of the test"""
    import json
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "filters_mi355x.json")
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


def _ln_p_forward(fwd_bits, tau, lam):
    return np.minimum(0.0, -float(lam) * (fwd_bits.astype(np.float64) - float(tau)))


@pytest.mark.parametrize("name", FIXTURES)
def test_score_filtered_against_the_binary_and_wh_score(name):
    """Stage outcomes 1 - 4 are the binary's, the stage counts are the fixture's, survivors carry wh_score's results and
    rejected pairs WH_FLAG_FILTERED.  Stage 4 compares float32 Forward scores of two programmes: a pair is excluded
    where the recorded ln P lies within tol of ln F3, tol = 10 x (lambda x 1e-4 bit - the project's Forward parity bound -
    + the width of the recorded bracket); at most 2 % of the pairs.  amino_multidomain is the case whose pairs go through
    the multidomain resolver's queue inside the compacted call.  The largest |ln P_ours - ln P_recorded| over the pairs
    with a resolvable recorded P goes into profiles/filters_mi355x.json (forward_stage_largest_ln_p_difference)."""
    from witch_amd import _lib
    from witch_amd.ehmm import EHMM
    fx = fixture(name)
    e = EHMM(fx.paths)
    try:
        deci0, flags0, fwd0 = e.score(fx.res, fx.off, want_fwd=True)
        tau, lam, present = e.evparams()
        assert present.all()
        worst = 0.0
        for key in ("default", "alt"):
            F = fx.F(key)
            deci, flags, fwd, stage = e.score(fx.res, fx.off, want_fwd=True, filters=F, nobias=True, want_stage=True)
            near = fx.near(key)
            for st, bit in ((0, 1), (1, 2), (2, 4)):
                bad = (((stage & bit) != 0) != (fx.expected(key, st) != 0)) & ~near
                assert not bad.any(), (name, key, st, np.argwhere(bad)[:5].tolist())
            # stage 4
            excl = np.zeros_like(near)
            for h, m in enumerate(fx.models):
                for q, p in enumerate(m["pairs"]):
                    lo, hi = p["T3"]
                    tol = 10.0 * (float(lam[h]) * 1e-4 + (hi - lo))
                    if hi > fx.g["ln_lo"] and abs(hi - math.log(F[2])) < tol:
                        excl[q, h] = True
                    if hi > fx.g["ln_lo"] and hi < -1e-6 and np.isfinite(fwd0[q, h]):
                        worst = max(worst, abs(float(_ln_p_forward(fwd0[q:q + 1, h], tau[h], lam[h])[0]) - hi))
            assert excl.sum() <= 0.02 * excl.size
            past3 = (stage & 4) != 0
            got4 = (stage & 16) != 0
            bad = (got4 != (fx.expected(key, 3) != 0)) & ~near & ~excl
            assert not bad.any(), (name, key, "Forward", np.argwhere(bad)[:5].tolist())
            assert not (got4 & ~past3).any()
            # survivors: wh_score's results; rejected: WH_FLAG_FILTERED and no WH_FLAG_REPORTED
            assert (deci[got4] == deci0[got4]).all() and (flags[got4] == flags0[got4]).all()
            assert (fwd[got4].view(np.uint32) == fwd0[got4].view(np.uint32)).all()
            assert (flags[~got4] == _lib.FLAG_FILTERED).all() and (deci[~got4] == 0).all()
            assert ((flags & _lib.FLAG_REPORTED) != 0).sum() == (got4 & ((flags0 & _lib.FLAG_REPORTED) != 0)).sum()
            # counts
            c = e.last_filter_counts()
            kept = past3.any(axis=1)
            assert c["pairs"] == fx.nq * fx.H and c["scored"] == int(kept.sum()) * fx.H and c["fwd"] == int(got4.sum())
            assert [c["msv"], c["bias"], c["vit"]] == [int(((stage & b) != 0).sum()) for b in (1, 2, 4)]
            if not near.any() and not excl.any():
                want = np.sum([m["counts"][key] for m in fx.models], axis=0).tolist()
                assert [c["msv"], c["bias"], c["vit"], c["fwd"]] == want
        print("%s: largest |ln P_ours - ln P_recorded| at the Forward stage: %.3g" % (name, worst))
        _record_forward_difference(name, worst)
    finally:
        e.close()


def test_score_filtered_scatters_back_partial_survivors():
    """H = 4 models and queries that survive on some models only (a surviving query is scored on all four): every pair
    comes back at its own index."""
    from witch_amd import _lib
    from witch_amd.ehmm import EHMM
    fx, lc = fixture("amino_hmmbuild"), fixture("lowcomplexity")
    seqs = fx.seqs + lc.seqs[:80]
    res, off = pack(seqs)
    e = EHMM(fx.paths)
    try:
        assert e.H == 4
        F = (0.3, 0.05, 1e-3)
        deci0, flags0 = e.score(res, off)
        deci, flags, stage = e.score(res, off, filters=F, nobias=True, want_stage=True)
        ref = filter_host(fx.paths, res, off, F)[1]
        assert ((stage & 15) == ref).all()
        got4 = (stage & 16) != 0
        n_surv = got4.sum(axis=1)
        assert ((n_surv > 0) & (n_surv < 4)).any() and (n_surv == 0).any() and (n_surv == 4).any()
        assert (deci[got4] == deci0[got4]).all() and (flags[got4] == flags0[got4]).all()
        assert (flags[~got4] == _lib.FLAG_FILTERED).all()
        # and a call without filters behaves as before
        deci1, flags1 = e.score(res, off)
        assert (deci1 == deci0).all() and (flags1 == flags0).all()
    finally:
        e.close()


def test_level0_hmmsearch_without_max_lists_the_binarys_sequences(tmp_path):
    from witch_amd.shim.server import GpuBackend, Server
    fx = fixture("dna_synth")
    h = 3                                     # the model on which the binary rejects at the MSV and at the Forward stage
    assert not fx.near("default", stages=(0, 2, 3))[:, h].any()
    fa = tmp_path / "q.fa"
    fa.write_text("".join(">%s\n%s\n" % (n, t) for n, t in zip(fx.qnames, fx.qtext)))
    srv = Server.__new__(Server)
    srv.backend = GpuBackend(0)
    try:
        out = srv.run_hmmsearch(["--cpu", "1", "--noali", "-E", "99999999", "--nobias", fx.paths[h], str(fa)], str(tmp_path))
        full = srv.run_hmmsearch(["--cpu", "1", "--noali", "-E", "99999999", "--max", fx.paths[h], str(fa)], str(tmp_path))
    finally:
        for _, (_, eh, _) in srv.backend.cache.items():
            eh.close()

    def listed(text):
        names, on = [], False
        for ln in text.splitlines():
            if ln.lstrip().startswith("E-value"):
                on = True
            elif on and ln.strip().startswith("---"):
                continue
            elif on and not ln.strip():
                break
            elif on:
                names.append(ln.split()[8])
        return set(names)
    want = {n for n, p in zip(fx.qnames, fx.models[h]["pairs"]) if p["out"]["default"][3]}
    assert listed(out) == want & listed(full) and len(want) < len(fx.qnames)
    counts = fx.models[h]["counts"]["default"]
    for label, n in zip(("MSV", "bias", "Vit", "Fwd"), counts):
        assert ("Passed %s filter:" % label).ljust(28) + "%15d" % n in out
    assert "Passed" not in full
