"""wh_align_pp_len on the GPU: the alignment kernels under a length model of the caller's choice (cfg_len per query), one
test per kernel path that reads it.

The reference is float64 and needs no new oracle code: a query of Ld residues under the length model of L residues is the
query followed by L - Ld gap codes under its own (tests/domains_seqlen_reference.align_under).  Columns are compared for
equality, posteriors within the bound tests/test_align_pp.py holds wh_align_pp to (tol32(Ld) = 2e-4 + 3e-6 Ld for the float32
kernels, 1e-9 plus one rounding to float for the float64 kernel), and against the device's own wh_align_pp on the padded
query: the same kernels computing the same quantity.
"""
import os

import numpy as np
import pytest

from tests import domains_reference as dr
from tests import domains_seqlen_reference as sr
from tests import pp_reference as ppr
from tests.conftest import load_case
from tests.test_align_pp import _need_gpu, tol32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def envelopes():
    """Per alphabet: (model path, [envelope residues], [L of the envelope's sequence], [reference columns], [reference
    posteriors], [whether the path differs from the envelope model's]) - envelopes of model 0 of dna_hmmbuild and
    amino_hmmbuild cut from the fixture's queries: every domain whose path changes under the sequence's model and as many
    that keep theirs, at most 24."""
    out = {}
    for name in ("dna_hmmbuild", "amino_hmmbuild"):
        case = load_case(name)
        seqs, env = dr.case_reference(name)
        _, seq = sr.reference_seqlen(name)
        changed = [(q, t) for q, h, t in sr.changed_domains(name) if h == 0][:12]
        same = [(q, int(r["index"])) for q in range(len(seqs)) for r in env[(q, 0)] if (q, int(r["index"])) not in changed][:len(changed)]
        subs, Ls, cols, pps, diff = [], [], [], [], []
        for q, t in changed + same:
            r = seq[(q, 0)][t]
            subs.append(np.ascontiguousarray(seqs[q][r["env_i"] - 1:r["env_j"]], dtype=np.uint8))
            Ls.append(len(seqs[q]))
            cols.append(r["cols"])
            pps.append(r["pp"])
            diff.append((q, t) in changed)
        if name == "dna_hmmbuild":
            assert any(case.qnames[q] == "rnd01" for q, _ in changed)
        assert any(diff) and not all(diff)
        out[name] = (case.hmm_paths[0], subs, np.array(Ls, dtype=np.int32), cols, pps, diff)
    return out


def _pairs(n):
    return np.arange(n, dtype=np.int64), np.zeros(n, dtype=np.int32)


def _check(tag, got_cols, co, got_pp, want_cols, want_pp, tol_of):
    worst = 0.0
    for p in range(len(want_cols)):
        a, b = int(co[p]), int(co[p + 1])
        assert np.array_equal(got_cols[a:b], want_cols[p]), (tag, p, "columns")
        if got_pp is not None:
            d = np.abs(got_pp[a:b].astype(np.float64) - want_pp[p])
            worst = max(worst, float(d.max()))
            assert np.all(np.isfinite(got_pp[a:b])) and np.all(d <= tol_of(p, b - a)), (tag, p, float(d.max()), tol_of(p, b - a))
    print("%s: %d pairs, largest |pp - ref| %.3g" % (tag, len(want_cols), worst))


# ------------------------------------------------------------------------------------------------ 1. null is identity
@pytest.mark.parametrize("name", ["dna_hmmbuild", "amino_hmmbuild"])
def test_null_and_own_length_are_wh_align_pp_bitwise(envelopes, name):
    """wh_align_pp_len_dev with a null d_cfg_len, and with cfg_len[q] = the query's own length, returns the bytes of
    wh_align_pp_dev; nothing outside the pairs' ranges is written (poisoned buffers with a gap behind every range)."""
    _need_gpu()
    import torch
    from witch_amd._lib import check, lib
    from witch_amd.ehmm import EHMM, pack_queries
    path, subs, Ls, _, _, _ = envelopes[name]
    res, offs = pack_queries(subs)
    lens = np.diff(offs)
    pq, ph = _pairs(len(subs))
    GAP = 3
    co = np.zeros(len(subs) + 1, dtype=np.int64)
    co[1:] = np.cumsum(lens + GAP)
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    res_t, offs_t, pq_t, ph_t, co_t = up(res), up(offs), up(pq), up(ph), up(co)
    e = EHMM([path])
    stream = e._stream()
    outs = []
    for cfg in ("plain", None, lens.astype(np.int32)):
        cols_t = torch.full((int(co[-1]),), -77, dtype=torch.int32, device=dev)
        pp_t = torch.full((int(co[-1]),), float("nan"), dtype=torch.float32, device=dev)
        args = (e._h, res_t.data_ptr(), offs_t.data_ptr(), len(subs), int(offs[-1]), int(lens.max()), pq_t.data_ptr(), ph_t.data_ptr(),
                len(subs), co_t.data_ptr(), cols_t.data_ptr(), pp_t.data_ptr())
        if isinstance(cfg, str):
            check(lib().wh_align_pp_dev(*args, stream), "wh_align_pp_dev")
        else:
            cfg_t = None if cfg is None else up(cfg)
            check(lib().wh_align_pp_len_dev(*args, None if cfg_t is None else cfg_t.data_ptr(), stream), "wh_align_pp_len_dev")
        torch.cuda.synchronize()
        outs.append((cols_t.cpu().numpy(), pp_t.cpu().numpy()))
    e.close()
    (c0, p0), (c1, p1), (c2, p2) = outs
    assert c0.tobytes() == c1.tobytes() == c2.tobytes()
    assert p0.tobytes() == p1.tobytes() == p2.tobytes()
    for p in range(len(subs)):
        a, n = int(co[p]), int(lens[p])
        assert np.all(c0[a + n:a + n + GAP] == -77) and np.all(np.isnan(p0[a + n:a + n + GAP]))
        assert np.all(np.isfinite(p0[a:a + n])) and (c0[a:a + n] >= 0).any()


# ------------------------------------------------------------------------------------------------ 2. the float64 reference
@pytest.fixture(scope="module")
def one_wave(envelopes):
    """The default launch of item 2 on both alphabets: {name: (cols, co, pp)}; the other paths are compared with it."""
    _need_gpu()
    from witch_amd.ehmm import EHMM, pack_queries
    out = {}
    for name, (path, subs, Ls, _, _, _) in envelopes.items():
        e = EHMM([path])
        res, offs = pack_queries(subs)
        out[name] = e.align(res, offs, *_pairs(len(subs)), want_pp=True, cfg_len=Ls)
        out[name + "/paths"] = e.last_align_paths()
        out[name + "/plain"] = e.align(res, offs, *_pairs(len(subs)), want_pp=True)
        # the device's own wh_align_pp on the envelopes padded to their sequences' lengths
        gap = sr.GAP_CODE[e.alphabet]
        pres, poffs = pack_queries([sr.padded(s, L, gap) for s, L in zip(subs, Ls)])
        out[name + "/padded"] = e.align(pres, poffs, *_pairs(len(subs)), want_pp=True)
        e.close()
    return out


@pytest.mark.parametrize("name", ["dna_hmmbuild", "amino_hmmbuild"])
def test_against_the_float64_reference_and_the_padded_envelope(envelopes, one_wave, name):
    path, subs, Ls, want_cols, want_pp, diff = envelopes[name]
    cols, co, pp = one_wave[name]
    _check(name + " cfg_len", cols, co, pp, want_cols, want_pp, lambda p, Ld: tol32(Ld))
    # the cases are worth their name: under its own length the envelope aligns differently where the reference says so
    c0, _, _ = one_wave[name + "/plain"]
    for p, d in enumerate(diff):
        assert np.array_equal(c0[co[p]:co[p + 1]], cols[co[p]:co[p + 1]]) != d, (name, p)
    pc, pco, ppp = one_wave[name + "/padded"]
    for p in range(len(subs)):
        a, n, b = int(co[p]), len(subs[p]), int(pco[p])
        assert np.array_equal(pc[b:b + n], cols[a:a + n]) and np.all(pc[b + n:int(pco[p + 1])] < 0), (name, p)
        assert np.abs(ppp[b:b + n].astype(np.float64) - pp[a:a + n]).max() <= tol32(n), (name, p)


# ------------------------------------------------------------------------------------------------ 3. every kernel path
@pytest.mark.parametrize("alphabet", ["dna", "amino"])
def test_node_window_and_full_width(alphabet, tmp_path):
    """Fragments on a 700-node model (the node window's range; the fixture models are shorter), cfg_len = the fragment's
    length plus 300: aligned on a node window - which must have run - and at full width (WH_NO_WINDOW).  Same columns;
    a window's posteriors are lower bounds of the full-width ones up to the bound, as in tests/test_align_pp.py."""
    _need_gpu()
    from oracle import oracle as orc
    from witch_amd.ehmm import EHMM, pack_queries
    paths, names, seqs = ppr.window_case(alphabet, str(tmp_path))
    seqs = seqs[:6] + seqs[24:28]
    ohm = orc.OracleHMM(paths[0])
    pmodel = ppr.Model(ohm)
    Ls = np.array([len(s) + 300 for s in seqs], dtype=np.int32)
    ref = [sr.align_under(ohm, pmodel, s, int(L)) for s, L in zip(seqs, Ls)]
    e = EHMM(paths[:1])
    res, offs = pack_queries(seqs)
    wc, co, wpp = e.align(res, offs, *_pairs(len(seqs)), want_pp=True, cfg_len=Ls)
    ran = e.last_align_paths()
    e.set_option("WH_NO_WINDOW", "1")
    fc, _, fpp = e.align(res, offs, *_pairs(len(seqs)), want_pp=True, cfg_len=Ls)
    ran_full = e.last_align_paths()
    pc, _, _ = e.align(res, offs, *_pairs(len(seqs)), want_pp=True)
    e.close()
    assert ran["window256"] + ran["window512"] > 0, ran
    assert ran_full["window256"] + ran_full["window512"] == 0, ran_full
    _check(alphabet + " window", wc, co, wpp, [r[0] for r in ref], [r[1] for r in ref], lambda p, Ld: tol32(Ld))
    _check(alphabet + " full width", fc, co, fpp, [r[0] for r in ref], [r[1] for r in ref], lambda p, Ld: tol32(Ld))
    for p in range(len(seqs)):
        assert np.all(wpp[co[p]:co[p + 1]] <= fpp[co[p]:co[p + 1]] + tol32(co[p + 1] - co[p]))
    assert len(pc) == len(wc)


def test_several_waves_per_pair(envelopes, one_wave):
    """WH_FORCE_WIDE=4 (read at load): the several-waves alignment kernel.  Columns equal to the one-wave launch's, posteriors
    within the bound of the reference (so within twice the bound of the one-wave launch's)."""
    _need_gpu()
    from witch_amd.ehmm import EHMM, pack_queries
    path, subs, Ls, want_cols, want_pp, _ = envelopes["dna_hmmbuild"]
    old = os.environ.get("WH_FORCE_WIDE")
    os.environ["WH_FORCE_WIDE"] = "4"
    try:
        e = EHMM([path])
    finally:
        if old is None:
            os.environ.pop("WH_FORCE_WIDE", None)
        else:
            os.environ["WH_FORCE_WIDE"] = old
    res, offs = pack_queries(subs)
    e.set_timing(True)
    cols, co, pp = e.align(res, offs, *_pairs(len(subs)), want_pp=True, cfg_len=Ls)
    launches = e.last_kernel_ms(2)[1]
    e.close()
    c1, co1, p1 = one_wave["dna_hmmbuild"]
    assert launches >= 2, "the several-waves launch did not follow the one-wave one"
    assert cols.tobytes() == c1.tobytes()
    _check("several waves, cfg_len", cols, co, pp, want_cols, want_pp, lambda p, Ld: tol32(Ld))
    assert np.all(np.abs(pp.astype(np.float64) - p1) <= 2 * tol32(np.repeat(np.diff(co), np.diff(co))))


def test_long_query_pass_both_residue_placements(envelopes, one_wave):
    """WH_SCORE_LMAIN at the median envelope length: the longer envelopes go to the any-size float64 kernel, then again with
    the residues in the wave's HBM slab (WH_LONGQ_FORCE).  Columns equal to the one-wave launch's; the float64 kernel's
    posteriors within 1e-9 plus one rounding to float of the reference; the two placements bitwise equal."""
    _need_gpu()
    from witch_amd.ehmm import EHMM, pack_queries
    path, subs, Ls, want_cols, want_pp, _ = envelopes["dna_hmmbuild"]
    lens = np.array([len(s) for s in subs])
    lmain = int(np.median(lens))
    long_pair = lens > lmain
    e = EHMM([path])
    res, offs = pack_queries(subs)
    e.set_option("WH_SCORE_LMAIN", str(lmain))
    cols, co, pp = e.align(res, offs, *_pairs(len(subs)), want_pp=True, cfg_len=Ls)
    n_long = e.last_long_align()[0]
    e.set_option("WH_LONGQ_FORCE", "1")
    cols2, _, pp2 = e.align(res, offs, *_pairs(len(subs)), want_pp=True, cfg_len=Ls)
    n_long2 = e.last_long_align()[0]
    e.close()
    assert n_long == n_long2 == int(long_pair.sum()) > 0
    assert cols.tobytes() == cols2.tobytes() == one_wave["dna_hmmbuild"][0].tobytes()
    assert pp.tobytes() == pp2.tobytes()
    _check("long-query pass, cfg_len", cols, co, pp, want_cols, want_pp, lambda p, Ld: 1e-9 + 2.0 ** -25 if long_pair[p] else tol32(Ld))


def test_log_space_instantiation_and_its_float64_hand_over(tmp_path):
    """A multi-copy query on the 1 900-node model leaves float32 range (tests/test_align_pp.py selects it so): without PP
    it is redone by the float32 log-space instantiation, with PP by the float64 kernel's log-space code.  Both under
    cfg_len = L + 2 000 give the reference's columns, and the float64 posteriors stay within that test's bound."""
    _need_gpu()
    from oracle import oracle as orc
    from witch_amd.ehmm import EHMM, pack_queries
    fx = ppr.load_fixture("long_model")
    fam, hp = ppr.long_model(fx["spec"], str(tmp_path))
    names, seqs, kinds = ppr.long_queries(fx["spec"], fam)
    s = min((x for x, k in zip(seqs, kinds) if k == "multicopy"), key=len)
    L = len(s)
    ohm = orc.OracleHMM(hp)
    want_cols, want_pp = sr.align_under(ohm, ppr.Model(ohm), s, L + 2000)
    cfg = np.array([L + 2000], dtype=np.int32)
    e = EHMM([hp])
    res, offs = pack_queries([s])
    one = (np.zeros(1, np.int64), np.zeros(1, np.int32))
    c0, co = e.align(res, offs, *one, cfg_len=cfg)
    n_log0 = e.last_align_status()[0]
    c1, _, pp = e.align(res, offs, *one, want_pp=True, cfg_len=cfg)
    n_log1 = e.last_align_status()[0]
    e.close()
    assert n_log0 > 0 and n_log1 > 0, "the pair stayed in float32 range"
    assert np.array_equal(c0, want_cols), "float32 log-space pass"
    assert np.array_equal(c1, want_cols), "float64 kernel"
    tol = 3 * L * 2.0 ** -53 * 1.39 * L + 2.0 ** -25
    d = np.abs(pp.astype(np.float64) - want_pp)
    print("log space: %d residues, largest |pp - ref| %.3g (bound %.3g)" % (L, float(d.max()), tol))
    assert d.max() <= tol
