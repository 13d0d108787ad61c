"""Models of any length: no node ceiling at load, the 48-cell several-waves-per-pair scoring class (12 289 - 24 576
nodes, wh_score_wide.hip), the float64 kernels beyond it, and the per-call refusal of a workspace that cannot fit.
Everything is checked against the CPU oracle; run on a real MI355X with ``pytest -m gpu``.

The oracle is slow on models this long (about a second per 150-residue query on a 20 000-node model), so the query
sets are small: short fragments, a fragment in random flanks and a query with two copies of the family (a multidomain region: the resolver runs on
these models too)."""
import os

import numpy as np
import pytest

from tests.test_gpu_parity import LONG_EPS, _check_decibits, _need_gpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def _queries(fam, seed):
    """Two 150-residue fragments, one 180-residue fragment in background flanks, and two 150-residue fragments of the
    family joined by 80 background residues."""
    from witch_amd import synth
    rng = np.random.default_rng(seed)
    bg = synth.background(fam.alphabet)
    K = len(bg)
    _, frag = synth.make_queries(fam, seed, 5, 150)
    _, mid = synth.make_queries(fam, seed + 1, 1, 180)
    seqs = [frag[0], frag[1]]
    a = int(rng.integers(20, 60))
    seqs.append(np.concatenate([rng.choice(K, size=a, p=bg), mid[0], rng.choice(K, size=80 - a, p=bg)]))
    seqs.append(np.concatenate([frag[2], rng.choice(K, size=80, p=bg), frag[3]]))
    return [s_.astype(np.uint8) for s_ in seqs]


class _Long:
    def __init__(self, seed, root_len, alphabet, outdir):
        from witch_amd import synth
        self.fam = synth.make_family(seed, root_len, 4, alphabet, 0.03, 1e-4)
        self.eh = synth.make_ehmm(self.fam, 1, outdir, witch_layout=False)
        self.M = self.eh.hmms[0].M
        self.seqs = _queries(self.fam, seed)


@pytest.fixture(scope="module")
def long_models(tmp_path_factory):
    d = tmp_path_factory.mktemp("long_models")
    return {name: _Long(seed, n, alph, str(d / name)) for name, seed, n, alph in
            [("dna13k", 13001, 13000, "dna"), ("dna20k", 20001, 20000, "dna"),
             ("dna33k", 33001, 33000, "dna"), ("amino17k", 17001, 17000, "amino")]}


def _score(paths, seqs, env=None):
    from witch_amd.ehmm import EHMM, pack_queries
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        e = EHMM(paths, hmm_index=list(range(len(paths))), nseq=[4] * len(paths))
        e.set_timing(True)
        res, offs = pack_queries(seqs)
        deci, flags, fwd = e.score(res, offs, want_fwd=True)
        launches = e.last_score_launches()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return e, res, offs, deci, flags, fwd, launches


def _check_scores(ctx, deci, flags, fwd, od, of, ofwd, osc):
    assert np.max(np.abs(fwd - ofwd)) <= 1e-3, (ctx, float(np.max(np.abs(fwd - ofwd))))
    assert np.array_equal(flags & 3, of & 3), ctx
    _check_decibits(deci, od, osc, (of & 1) == 1, ctx, LONG_EPS)


@pytest.mark.parametrize("name", ["dna20k", "dna33k", "amino17k"])
def test_models_beyond_16384_nodes_load_score_and_align(name, long_models, orc):
    """Models beyond the old 16 384-node ceiling (the DNA model of ~33 000 nodes also beyond a 16-bit node index): the
    load succeeds, and flags, Forward, deci-bits and aligned columns equal the oracle's."""
    _need_gpu()
    lm = long_models[name]
    assert lm.M > 16384
    e, res, offs, deci, flags, fwd, _ = _score(lm.eh.paths, lm.seqs)
    ohm = [orc.OracleHMM(p) for p in lm.eh.paths]
    od, of, ofwd, osc = orc.score_batch(ohm, res, offs)
    _check_scores(name, deci, flags, fwd, od, of, ofwd, osc)
    assert (of[:, 0] & 1).sum() >= 3, name            # the fragments are reported
    assert (of[3, 0] & 2) != 0, name                   # the two-copy query is a multidomain region (resolver)
    # alignment of the fragment in flanks (float64 kernel; the oracle's alignment is the slow part: seconds per pair)
    pq, ph = [2], [0]
    cols, co = e.align(res, offs, pq, ph)
    for p in range(len(pq)):
        want = ohm[0].align(lm.seqs[pq[p]])
        assert np.array_equal(cols[co[p]:co[p + 1]], want), (name, pq[p])
    e.close()


def test_models_of_12289_to_24576_nodes_take_the_48_cell_wide_class(long_models, orc):
    """Models of ~13 000 and ~20 000 nodes are scored by the several-waves-per-pair kernel with 48 cells per lane (kind
    3, cells_per_lane = 48 x waves: 5 and 7 waves), with the oracle's numbers; every Forward row stored (WH_WIDE_DENSE)
    gives the same numbers as the sparse spill."""
    _need_gpu()
    a, b = long_models["dna13k"], long_models["dna20k"]
    paths = a.eh.paths + b.eh.paths
    seqs = a.seqs + b.seqs
    e, res, offs, deci, flags, fwd, launches = _score(paths, seqs)
    e.close()
    wide = sorted((c, ms) for c, kind, ms in launches if kind == 3)
    assert [c for c, _ in wide] == [48 * 5, 48 * 7], launches
    assert not any(kind == 2 for _, kind, _ in launches), launches
    ohm = [orc.OracleHMM(p) for p in paths]
    od, of, ofwd, osc = orc.score_batch(ohm, res, offs)
    _check_scores("48-cell class", deci, flags, fwd, od, of, ofwd, osc)
    e2, _, _, deci2, flags2, fwd2, _ = _score(paths, seqs, {"WH_WIDE_DENSE": "1"})
    e2.close()
    assert np.array_equal(fwd2, fwd)
    assert np.array_equal(flags2 & 7, flags & 7)
    single = (flags & 2) == 0
    assert np.max(np.abs(deci2[single].astype(np.int64) - deci[single])) <= 1
    assert np.array_equal(deci2[~single], deci[~single])


def test_48_cell_wide_class_on_the_golden_cases(orc):
    """WH_FORCE_WIDE=48 (read at load) routes every model of the golden cases through the 48-cell class (one or two
    waves per pair; alignment stays on the one-wave kernels): Forward, flags and deci-bits against the oracle."""
    _need_gpu()
    from tests.conftest import load_case
    for name in ("dna_synth", "dna_hmmbuild", "amino_hmmbuild", "example_sub30"):
        case = load_case(name)
        from witch_amd.ehmm import EHMM
        e0 = EHMM(case.hmm_paths[:1], hmm_index=case.hmm_index[:1], nseq=case.nseq[:1])
        seqs = [e0.digitize(s_) for s_ in case.qseqs]
        e0.close()
        e, res, offs, deci, flags, fwd, launches = _score(case.hmm_paths, seqs, {"WH_FORCE_WIDE": "48"})
        e.close()
        assert launches and all(kind == 3 and c % 48 == 0 for c, kind, _ in launches), (name, launches)
        ohm = [orc.OracleHMM(p) for p in case.hmm_paths]
        od, of, ofwd, osc = orc.score_batch(ohm, res, offs)
        fin = np.isfinite(ofwd)
        assert np.max(np.abs(fwd[fin] - ofwd[fin])) <= 1e-4, (name, float(np.max(np.abs(fwd[fin] - ofwd[fin]))))
        assert np.array_equal(flags & 7, of & 7), name
        multi = (of & 2) != 0
        _check_decibits(np.where(multi, od, deci), od, osc, (of & 1) == 1, name)
        _check_decibits(np.where(multi, deci, od), od, osc, (of & 1) == 1, name + " (multidomain)", LONG_EPS)


def test_a_workspace_that_cannot_fit_is_refused_and_the_handle_stays_usable(long_models):
    """An alignment call whose ONE wave's float64 slab is larger than the device's memory (a 10^6-residue query on a
    ~20 000-node model: ~480 GB per wave) is refused with WH_ENOMEM before anything is launched (timing mode: no kernel
    interval, no launch), and the error names the model length, the query length cap and the figures; so is a scoring
    call on the same query (the float64 front end's slab); the next calls on the same handle succeed."""
    _need_gpu()
    import torch
    from witch_amd._lib import WitchHipError
    from witch_amd.ehmm import EHMM, pack_queries
    lm = long_models["dna20k"]
    total = torch.cuda.get_device_properties(0).total_memory
    Lhuge = 1_000_000
    slab = (Lhuge + 4) * (3 * ((-(-lm.M // 64) + 3) // 4 * 4) * 64) * 8
    assert slab > total
    e = EHMM(lm.eh.paths, hmm_index=[0], nseq=[4])
    e.set_timing(True)
    rng = np.random.default_rng(5)
    huge = rng.integers(0, 4, size=Lhuge).astype(np.uint8)
    res, offs = pack_queries([lm.seqs[0], huge])
    with pytest.raises(WitchHipError) as ei:
        e.align(res, offs, [1], [0])
    msg = str(ei.value)
    assert "(-6)" in msg, msg                                     # WH_ENOMEM
    assert str(lm.M) in msg and str(Lhuge) in msg and "bytes free" in msg, msg
    assert e.last_kernel_ms(2) == (0.0, 0)                        # nothing was launched
    with pytest.raises(WitchHipError) as ei:
        e.score(res, offs)
    msg = str(ei.value)
    assert "(-6)" in msg and str(lm.M) in msg and str(Lhuge) in msg and "bytes free" in msg, msg
    assert e.last_kernel_ms(0) == (0.0, 0) and e.last_score_launches() == []
    res1, offs1 = pack_queries([lm.seqs[0]])
    cols, co = e.align(res1, offs1, [0], [0])
    assert co[1] - co[0] == len(lm.seqs[0]) and (cols[co[0]:co[1]] >= 0).any()
    assert e.last_kernel_ms(2)[1] > 0
    deci, flags = e.score(res1, offs1)[:2]
    assert flags[0, 0] & 1 and e.last_kernel_ms(0)[1] > 0
    e.close()


def test_models_in_ten_wide_classes_score_in_one_call(tmp_path, orc):
    """One eHMM with a model in each of ten several-waves-per-pair classes (12 cells x 5..8 waves, 16 x 7..8, 24 x 6..8,
    48 x 5: 3 500 - 13 000 nodes), as a large backbone's eHMM has: one call scores them all, one launch per class,
    with the oracle's numbers."""
    _need_gpu()
    from witch_amd import synth
    sizes = [3500, 4200, 5000, 5800, 6600, 7600, 8800, 10000, 11500, 13000]
    fams, paths = [], []
    for t, n in enumerate(sizes):
        fam = synth.make_family(31000 + t, n, 4, "dna", 0.03, 1e-4)
        paths += synth.make_ehmm(fam, 1, str(tmp_path / ("m%d" % t)), witch_layout=False).paths
        fams.append(fam)
    seqs = []
    for t in (0, 4, 7, 9):
        _, q = synth.make_queries(fams[t], 700 + t, 1, 150)
        seqs.append(q[0].astype(np.uint8))
    seqs += _queries(fams[8], 800)[2:]                  # a fragment in flanks and a two-copy query (resolver)
    e, res, offs, deci, flags, fwd, launches = _score(paths, seqs)
    e.close()
    wide = sorted(c for c, kind, _ in launches if kind == 3)
    assert wide == [12 * 5, 12 * 6, 12 * 7, 12 * 8, 16 * 7, 16 * 8, 24 * 6, 24 * 7, 24 * 8, 48 * 5], launches
    ohm = [orc.OracleHMM(p) for p in paths]
    od, of, ofwd, osc = orc.score_batch(ohm, res, offs)
    _check_scores("ten wide classes", deci, flags, fwd, od, of, ofwd, osc)
