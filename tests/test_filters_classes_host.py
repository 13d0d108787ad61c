"""hmmsearch's acceleration filters on every model size class, host side (no GPU): the scalar pipeline wh_filter_host
against the stage outcomes of the reference's bundled hmmsearch on seeded models of 1 - 3 073 nodes - every class edge
of wh_filter.hip, the scalar cores beyond 3 072 nodes, the 1-, 2-, 3- and 5-node models, and variants whose MSV mu is
lowered to -40 so that low MSV scores have a P-value below 1 (tests/golden/filters/classes_*, with the bias filter
tests/golden/filters_bias/classes_*; tests/filters_classes_common.py).

What these fixtures pinned first is the MSV filter's empty diagonal (wh_calibrate.h, calib_msv_floor): before it, the
binary's MSV-stage P was smaller than ours on every query that no node scores well, e.g. ln P -4.211135 against
-2.608351 (DNA, 1 node, query C), -2.126572 against -1.287530 (DNA, 3 nodes, TTTT), -1.524006 against -1.126518
(protein, 5 nodes, W)."""
import math

import numpy as np
import pytest

from tests.filters_bias_common import BIAS_ON
from tests.filters_classes_common import CLASSES, LIMIT_LENGTHS, classes_fixture
from tests.filters_common import MAX_SKIP, filter_host, msv_tjb

LOG2 = 0.69314718055994529
VIT_OVERFLOW, VIT_NOT_RUN = 32768, -32769
RUN_ALL_VIT = (1.0, 1e-12, 1.0)       # every pair passes MSV, and the Viterbi sweep runs unless the MSV filter overflowed
_runs = {}


def _near(fx, p, key, brackets):
    F = fx.F(key)
    return any(p[t][1] > fx.floor and p[t][0] <= math.log(F[i]) <= p[t][1] for i, t in brackets)


def _run(name, kind, h, F, nobias):
    """wh_filter_host on model h alone with every pair the fixture lists for it; computed once per setting"""
    k = (name, kind, h, tuple(F), nobias)
    if k not in _runs:
        fx = classes_fixture(name, kind)
        res, off, lens, recs = fx.model_call(h)
        rc, stage, bias, msv, vit, cnt = filter_host([fx.paths[h]], res, off, F, nobias=nobias)
        assert rc == 0
        _runs[k] = (stage[:, 0], bias[:, 0], msv[:, 0], vit[:, 0], cnt, lens, recs)
    return _runs[k]


@pytest.mark.parametrize("kind", ["filters", "filters_bias"])
@pytest.mark.parametrize("name", list(CLASSES))
def test_stage_outcomes_and_counts_equal_the_binary(name, kind):
    """MSV, bias and Viterbi stage outcomes of every listed pair are the binary's, with --nobias and with the bias filter,
    at HMMER's default thresholds and at (0.3, 0.05, 1e-3) - exact except for pairs whose recorded threshold lies within
    its own bisection bracket of the F in use (at most 1 % of a fixture); a model none of whose pairs is such a one has
    the binary's "Passed" counts.  No model and no variant is exempt."""
    fx = classes_fixture(name, kind)
    nobias, brackets = (1, ((0, "T1"), (1, "T2"))) if kind == "filters" else (BIAS_ON, ((0, "Tb"), (1, "T2b")))
    for key in ("default", "alt"):
        skipped = 0
        for h, m in enumerate(fx.models):
            stage, bias, msv, vit, cnt, lens, recs = _run(name, kind, h, fx.F(key), nobias)
            names = fx.model_names(h)
            near = np.array([_near(fx, p, key, brackets) for p in recs])
            skipped += int(near.sum())
            for st, bit in ((0, 1), (1, 2), (2, 4)):
                exp = np.array([p["out"][key][st] != 0 for p in recs])
                bad = (((stage & bit) != 0) != exp) & ~near
                assert not bad.any(), (name, kind, key, m["M"], m["variant"], st, [names[i] for i in np.argwhere(bad)[:5, 0]])
            ran = (stage & 8) != 0
            assert not (ran & ((stage & 2) == 0)).any() and ((vit == VIT_NOT_RUN) == ~ran).all()
            if kind == "filters":
                assert not bias.any()
            else:
                assert not bias[(stage & 1) == 0].any()
            if not near.any():
                got = [int(((stage & b) != 0).sum()) for b in (1, 2, 4)]
                assert got == m["counts"][key][:3], (name, kind, key, m["M"], m["variant"])
                assert cnt.tolist() == [len(recs)] + got
        assert skipped <= MAX_SKIP * sum(len(m["pairs"]) for m in fx.models)


@pytest.mark.parametrize("name", list(CLASSES))
def test_msv_raw_scores_equal_the_recovered_integers(name):
    """Where the binary's MSV P-value can be inverted (1 - P above 1e-9, no overflow) the fixture holds
    round((usc + 3) scale) = xJ - tjb - base, recovered within 0.25 of an integer: the scalar filter's own, on at least 5
    pairs of every model - the 1-, 2- and 3-node models and the mu-lowered variants like the rest."""
    fx = classes_fixture(name)
    for h, m in enumerate(fx.models):
        stage, bias, msv, vit, cnt, lens, recs = _run(name, "filters", h, (1.0, 1.0, 1.0), 1)
        assert ((stage & 7) == 7).all()
        names = fx.model_names(h)
        n = 0
        for i, p in enumerate(recs):
            if p["msv_int"] is None:
                continue
            assert p["msv_resid"] < 0.25
            assert int(msv[i]) - msv_tjb(lens[i]) - 190 == p["msv_int"], (name, m["M"], m["variant"], names[i])
            n += 1
        assert n >= 5, (name, m["M"], m["variant"], n)


@pytest.mark.parametrize("name", list(CLASSES))
def test_the_empty_diagonal_is_the_binarys_at_every_model_length(name):
    """The mu-lowered variants hold queries that no node scores well ("poor": residues whose best log-odds over the nodes is
    negative, else the 'any' code).  There the binary's integer is the empty diagonal's, -(2 tjb + tbm + tec) - on 1, 2, 3
    and 5 nodes and on 513 alike - and so is ours.  Protein, 3 072 nodes: at 30 000 residues of X it still is; at 45 000,
    where tjb + tbm + tec + bias reaches 127, the binary's lies below it, and so does ours."""
    fx = classes_fixture(name)
    seen = 0
    for h, m in enumerate(fx.models):
        if m["variant"] != "mu40":
            continue
        stage, bias, msv, vit, cnt, lens, recs = _run(name, "filters", h, (1.0, 1.0, 1.0), 1)
        M = m["M"]
        tbm = int(-round(3.0 / LOG2 * math.log(2.0 / (M * (M + 1.0)))))
        n = 0
        for i, qn in enumerate(fx.model_names(h)):
            if not qn.startswith(("poor", "limit")) or recs[i]["msv_int"] is None:
                continue
            ours = int(msv[i]) - msv_tjb(lens[i]) - 190
            empty = -(2 * msv_tjb(lens[i]) + tbm + 3)
            assert ours == recs[i]["msv_int"], (name, M, qn)
            if qn == "limit%d" % LIMIT_LENGTHS[1]:
                assert ours < empty, (name, M, qn)
            else:
                assert ours == empty, (name, M, qn)
            n += 1
        assert n >= 3, (name, M, n)
        seen += 1
    assert seen == len([m for m in fx.models if m["variant"] == "mu40"]) >= 3


@pytest.mark.parametrize("name", list(CLASSES))
def test_overflow_pairs_pass_at_every_threshold(name):
    """A pair whose T1 bracket is the bisection's floor overflowed the MSV filter in the binary: ours returns the overflow
    (and nowhere else), the pair passes stages 1 - 3 at any thresholds and its Viterbi sweep never runs.  A pair whose T2 is
    the floor while T1 is not overflowed the Viterbi filter alone: the sweep runs, returns the overflow and passes.  Every
    model of 5 nodes or more has an MSV overflow, except DNA's 5-node model, on which the filter cannot overflow (the
    generator says why); each alphabet has a Viterbi overflow without an MSV overflow."""
    fx = classes_fixture(name)
    vit_only = 0
    for h, m in enumerate(fx.models):
        for F in (RUN_ALL_VIT, (1e-300, 1e-300, 1e-300), fx.F("default"), fx.F("alt")):
            stage, bias, msv, vit, cnt, lens, recs = _run(name, "filters", h, F, 1)
            over1 = np.array([p["T1"][1] == fx.floor for p in recs])
            over2 = np.array([p["T2"][1] == fx.floor for p in recs]) & ~over1
            assert ((msv == -1) == over1).all(), (name, m["M"], m["variant"], F)
            assert ((stage[over1] & 15) == 7).all() and (vit[over1] == VIT_NOT_RUN).all()
            if F is RUN_ALL_VIT:
                assert ((vit == VIT_OVERFLOW) == over2).all(), (name, m["M"], m["variant"])
                assert ((stage[over2] & 15) == 15).all()
                vit_only += int(over2.sum())
            else:
                assert (((stage[over2] & 2) != 0) == ((stage[over2] & 4) != 0)).all()      # past the MSV stage: past the Viterbi stage
        if m["M"] >= 5:
            assert over1.any() == ((name, m["M"]) != ("classes_dna", 5)), (name, m["M"], m["variant"])
    assert vit_only >= 1
