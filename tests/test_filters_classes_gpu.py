"""hmmsearch's acceleration filters on the device, on every model size class of wh_filter.hip, against the reference's
bundled hmmsearch DIRECTLY (tests/golden/filters/classes_*, tests/golden/filters_bias/classes_*; no oracle run here):
seeded models of 1 - 3 073 nodes - every register-class edge, the scalar cores beyond 3 072 nodes, the smallest models and
the variants with the MSV mu at -40 (tests/filters_classes_common.py).  One handle per alphabet holds all of its models;
a call carries the full query x model matrix and the listed pairs are checked against the binary, all of them against the
scalar pipeline wh_filter_host bit for bit."""
import math

import numpy as np
import pytest

from tests.filters_classes_common import CLASSES, LIMIT_LENGTHS, classes_fixture
from tests.filters_common import MAX_SKIP, msv_tjb
from tests.test_filters_bias_gpu import _record as _record_bias
from tests.test_filters_bias_gpu import _same as _same_bias
from tests.test_filters_gpu import _ln_p_forward, _record_forward_difference, _same

pytestmark = pytest.mark.gpu

LOG2 = 0.69314718055994529
KINDS = {"filters": ("T1", "T2", "T3"), "filters_bias": ("Tb", "T2b", "T3b")}


@pytest.fixture(scope="module", params=list(CLASSES))
def handle(request):
    """(fixture name, the alphabet's handle with all of its models)"""
    from witch_amd.ehmm import EHMM
    fx = classes_fixture(request.param)
    e = EHMM(fx.paths)
    assert e.M.tolist() == [m["M"] for m in fx.models]
    yield request.param, e
    e.close()


def _against_the_binary(fx, key, stage, brackets, stages):
    """the listed pairs' outcomes are the binary's outside their own brackets; returns near"""
    near = fx.near(key, brackets)
    assert near.sum() <= MAX_SKIP * fx.npairs
    for st, bit in stages:
        bad = (((stage & bit) != 0) != (fx.expected(key, st) != 0)) & fx.listed & ~near
        assert not bad.any(), (fx.name, fx.kind, key, st, [(fx.models[h]["M"], fx.models[h]["variant"], fx.qnames[q]) for q, h in np.argwhere(bad)[:5]])
    return near


def _passed_counts(fx, key, stage, near, bits):
    """a model none of whose listed pairs is near a bracket has the binary's "Passed" numbers over its listed pairs (the
    limit queries, which the matrix leaves out, taken off)"""
    n = 0
    for h, m in enumerate(fx.models):
        if near[:, h].any():
            continue
        off = [sum(p["out"][key][st] for r, p in zip(fx.pair_q[h], m["pairs"]) if r is None) for st in range(4)]
        got = [int((((stage[:, h] & b) != 0) & fx.listed[:, h]).sum()) for b in bits]
        assert got == [m["counts"][key][st] - off[st] for st in range(len(bits))], (fx.name, fx.kind, key, m["M"], m["variant"])
        n += 1
    assert n >= fx.H // 2


@pytest.mark.parametrize("kind", list(KINDS))
def test_filter_on_every_class_against_the_binary_and_the_scalar_pipeline(handle, kind):
    """wh_filter, with --nobias' pipeline and with the bias filter, at both threshold triples: stage byte, bias_nats, both raw
    scores and the counts equal wh_filter_host's bit for bit on the whole matrix, and the listed pairs' MSV, bias and
    Viterbi outcomes and every model's "Passed" numbers are the binary's."""
    name, e = handle
    fx = classes_fixture(name, kind)
    for key in ("default", "alt"):
        if kind == "filters":
            stage = _same(e, fx.paths, fx.res, fx.off, fx.F(key))[0]
        else:
            stage = _same_bias(e, fx.paths, fx.res, fx.off, fx.F(key))[0]
        near = _against_the_binary(fx, key, stage, KINDS[kind][:2], ((0, 1), (1, 2), (2, 4)))
        _passed_counts(fx, key, stage, near, (1, 2, 4))


def test_msv_raw_on_the_device_is_the_binarys_integer(handle):
    """F = 1: the device's raw MSV score of every listed pair whose P the binary resolves is the recovered integer - the
    empty diagonal of the smallest models and of the mu-lowered variants included (register classes and scalar cores)."""
    name, e = handle
    fx = classes_fixture(name)
    msv = e.filter(fx.res, fx.off, filters=(1.0, 1.0, 1.0), nobias=True, want_raw=True)[2]
    per_model = np.zeros(fx.H, int)
    for q, h, p in fx.pairs():
        if p["msv_int"] is not None:
            assert p["msv_resid"] < 0.25
            assert int(msv[q, h]) - msv_tjb(len(fx.seqs[q])) - 190 == p["msv_int"], (name, fx.models[h]["M"], fx.models[h]["variant"], fx.qnames[q])
            per_model[h] += 1
    assert (per_model >= 5).all(), per_model.tolist()


def test_the_limit_of_the_empty_diagonal_on_the_device():
    """Protein, 3 072 nodes (48 cells per lane), MSV mu at -40, runs of X: 30 000 residues score the empty diagonal,
    45 000 - where tjb + tbm + tec + bias reaches 127 - score below it, as in the binary; device == host bit for bit, and the
    outcomes at both triples, with and without the bias filter, are the binary's.  These queries run on their own model
    alone: on the one-lane-per-pair cores of the 3 073-node model they would take many seconds."""
    from witch_amd.ehmm import EHMM
    fx = classes_fixture("classes_amino")
    (h,) = fx.limit_models()
    assert (fx.models[h]["M"], fx.models[h]["variant"]) == (3072, "mu40")
    e = EHMM([fx.paths[h]])
    try:
        res, off, lens, recs = fx.model_call(h, limit=True)
        assert lens == list(LIMIT_LENGTHS)
        msv = _same(e, [fx.paths[h]], res, off, (1.0, 1.0, 1.0))[1][:, 0]
        ours = [int(msv[i]) - msv_tjb(lens[i]) - 190 for i in range(2)]
        assert ours == [p["msv_int"] for p in recs]
        tbm = int(-round(3.0 / LOG2 * math.log(2.0 / (3072 * 3073.0))))
        empty = [-(2 * msv_tjb(n) + tbm + 3) for n in lens]
        assert ours[0] == empty[0] and ours[1] < empty[1]
        for kind, same, brackets in (("filters", _same, ("T1", "T2")), ("filters_bias", _same_bias, ("Tb", "T2b"))):
            fb = classes_fixture("classes_amino", kind)
            recs = fb.model_call(h, limit=True)[3]
            for key in ("default", "alt"):
                F = fb.F(key)
                stage = same(e, [fb.paths[h]], res, off, F)[0][:, 0]
                for i, p in enumerate(recs):
                    assert not any(p[t][1] > fb.floor and p[t][0] <= math.log(F[j]) <= p[t][1] for j, t in enumerate(brackets))
                    assert [int((stage[i] & b) != 0) for b in (1, 2, 4)] == p["out"][key][:3], (kind, key, lens[i])
    finally:
        e.close()


def _ln_p_worst(fx, bracket, bits, tau, lam, fwd0):
    """the largest |ln P_ours - ln P_recorded| at the Forward stage over the listed pairs with a resolvable recorded P, and
    the pair it belongs to"""
    worst, where = 0.0, None
    for q, h, p in fx.pairs():
        hi = p[bracket][1]
        if fx.floor < hi < -1e-6 and np.isfinite(fwd0[q, h]):
            d = abs(float(_ln_p_forward(bits[q:q + 1, h], tau[h], lam[h])[0]) - hi)
            if d > worst:
                worst, where = d, (fx.models[h]["M"], fx.models[h]["variant"], fx.qnames[q])
    return worst, where


def _survivors(e, fx, stage, deci, flags, fwd, deci0, flags0, fwd0):
    """survivors carry wh_score's bits, rejected pairs WH_FLAG_FILTERED; the counts are the stage bytes'"""
    from witch_amd import _lib
    past3 = (stage & 4) != 0
    got4 = (stage & 16) != 0
    assert not (got4 & ~past3).any()
    assert (deci[got4] == deci0[got4]).all() and (flags[got4] == flags0[got4]).all()
    assert (fwd[got4].view(np.uint32) == fwd0[got4].view(np.uint32)).all()
    assert (flags[~got4] == _lib.FLAG_FILTERED).all() and (deci[~got4] == 0).all()
    assert ((flags & _lib.FLAG_REPORTED) != 0).sum() == (got4 & ((flags0 & _lib.FLAG_REPORTED) != 0)).sum()
    c = e.last_filter_counts()
    kept = past3.any(axis=1)
    assert c["pairs"] == fx.nq * fx.H and c["scored"] == int(kept.sum()) * fx.H and c["fwd"] == int(got4.sum())
    assert [c["msv"], c["bias"], c["vit"]] == [int(((stage & b) != 0).sum()) for b in (1, 2, 4)]
    return got4


def test_score_filtered_against_the_binary_and_wh_score(handle):
    """wh_score_filtered, --nobias' pipeline: stages 1 - 3 of the listed pairs are the binary's; the Forward stage compares
    float32 Forward scores of two programmes, so a pair is excluded where the recorded ln P lies within tol of ln F3,
    tol = 10 x (lambda x 1e-4 bit + the width of the recorded bracket) - at most 2 % of the listed pairs; survivors carry
    wh_score's bits, rejected pairs WH_FLAG_FILTERED.  The largest |ln P_ours - ln P_recorded| over the pairs with a
    resolvable recorded P - the first meeting of the Forward stage of models beyond 3 072 nodes with the binary - goes into
    profiles/filters_mi355x.json (forward_stage_largest_ln_p_difference); no bound is asserted on it here."""
    name, e = handle
    fx = classes_fixture(name)
    deci0, flags0, fwd0 = e.score(fx.res, fx.off, want_fwd=True)
    tau, lam, present = e.evparams()
    assert present.all()
    worst, where = _ln_p_worst(fx, "T3", fwd0, tau, lam, fwd0)
    print("%s: largest |ln P_ours - ln P_recorded| at the Forward stage: %.3g at %s" % (name, worst, where))
    _record_forward_difference(name, worst)
    for key in ("default", "alt"):
        F = fx.F(key)
        deci, flags, fwd, stage = e.score(fx.res, fx.off, want_fwd=True, filters=F, nobias=True, want_stage=True)
        near = _against_the_binary(fx, key, stage, ("T1", "T2"), ((0, 1), (1, 2), (2, 4)))
        excl = np.zeros_like(near)
        for q, h, p in fx.pairs():
            lo, hi = p["T3"]
            if hi > fx.floor and abs(hi - math.log(F[2])) < 10.0 * (float(lam[h]) * 1e-4 + (hi - lo)):
                excl[q, h] = True
        assert excl.sum() <= 0.02 * fx.npairs
        got4 = _survivors(e, fx, stage, deci, flags, fwd, deci0, flags0, fwd0)
        bad = (got4 != (fx.expected(key, 3) != 0)) & fx.listed & ~near & ~excl
        assert not bad.any(), (name, key, "Forward", [(fx.models[h]["M"], fx.models[h]["variant"], fx.qnames[q]) for q, h in np.argwhere(bad)[:5]])
        _passed_counts(fx, key, stage, near | excl, (1, 2, 4, 16))


def test_score_filtered_with_the_bias_filter(handle):
    """The same with the bias filter on: all four stages of the listed pairs are the binary's outside their own brackets
    (Tb, T2b, T3b; at most 1 % skipped).  The largest |ln P_ours - ln P_recorded| at the Forward stage, P against the bias
    filter's score, goes into profiles/filters_bias_mi355x.json; no bound is asserted on it here."""
    name, e = handle
    fx = classes_fixture(name, "filters_bias")
    deci0, flags0, fwd0 = e.score(fx.res, fx.off, want_fwd=True)
    tau, lam, present = e.evparams()
    bias_all = e.filter(fx.res, fx.off, filters=(1.0, 1.0, 1.0), bias=True)[1]
    ours = fwd0 - (bias_all.astype(np.float64) / LOG2).astype(np.float32)
    worst, where = _ln_p_worst(fx, "T3b", ours, tau, lam, fwd0)
    print("%s: largest |ln P_ours - ln P_recorded| at the Forward stage, bias filter on: %.3g at %s" % (name, worst, where))
    _record_bias(name, worst)
    for key in ("default", "alt"):
        deci, flags, fwd, stage = e.score(fx.res, fx.off, want_fwd=True, filters=fx.F(key), bias=True, want_stage=True)
        near = _against_the_binary(fx, key, stage, KINDS["filters_bias"], ((0, 1), (1, 2), (2, 4), (3, 16)))
        _survivors(e, fx, stage, deci, flags, fwd, deci0, flags0, fwd0)
        _passed_counts(fx, key, stage, near, (1, 2, 4, 16))
