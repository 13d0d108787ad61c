"""GPU parity tests: the HIP path (through the C ABI of libwitch_hip.so) against the CPU
oracle on the same inputs, and against the committed HMMER / reference-Python golden
vectors.  Run on a real MI355X with ``pytest -m gpu``.

Tolerances (BASELINE.json north_star / SURVEY.md section 8.0):
  * Forward log-odds: |GPU - oracle(float64)| <= 1e-4 bit
  * region/envelope coordinates, reported mask, multidomain flag: identical
  * deci-bit scores: identical, except where the oracle's float32 score lies within
    BOUNDARY_EPS bit of a "%6.1f" rounding boundary (then at most one deci-bit apart)
  * top-k models, order, n_used: identical; weights rel 1e-12 vs the numpy restatement
  * aligned columns: identical
"""
import os

import numpy as np
import pytest

from witch_amd._lib import WH_MAX_ENVELOPES

pytestmark = pytest.mark.gpu

BOUNDARY_EPS = 2e-3   # bits; float32 ulp at 100+ bits is 8e-6, null2 sums differ by a few ulp


def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def _load(case):
    from witch_amd.ehmm import EHMM, pack_queries
    e = EHMM(case.hmm_paths, hmm_index=case.hmm_index, nseq=case.nseq)
    seqs = [e.digitize(s) for s in case.qseqs]
    res, offs = pack_queries(seqs)
    return e, seqs, res, offs


def _near_boundary(score):
    frac = abs(float(score)) * 10.0
    return abs((frac % 1.0) - 0.5) < BOUNDARY_EPS * 10.0


LONG_EPS = 0.02       # bits; SURVEY.md D-8's gate ("0 whenever the float64 restatement is >= 0.02 bit from a
                      # rounding boundary"): used where the envelopes are hundreds to thousands of rows long and
                      # the float32 null2 sums differ from the float64 oracle by more than a few ulp


def _near_boundary_eps(score, eps):
    frac = abs(float(score)) * 10.0
    return abs((frac % 1.0) - 0.5) < eps * 10.0


def _check_decibits(deci, od, osc, rep, ctx, eps=BOUNDARY_EPS):
    """deci-bit scores equal the oracle's, except that a pair whose float score
    lies within <eps> bit of a "%6.1f" rounding boundary may differ by exactly one unit."""
    bad = np.argwhere((deci != od) & rep)
    for qi, hj in bad:
        assert abs(int(deci[qi, hj]) - int(od[qi, hj])) == 1, (ctx, int(qi), int(hj), int(deci[qi, hj]), int(od[qi, hj]))
        assert _near_boundary_eps(osc[qi, hj], eps), (ctx, int(qi), int(hj), float(osc[qi, hj]), int(deci[qi, hj]), int(od[qi, hj]))
    return len(bad)


def _check_one_decibit(got, want, float_score, ctx, eps=BOUNDARY_EPS):
    """The same rule for ONE pair: equal, or one unit apart with the oracle's float score at a rounding boundary."""
    if int(got) != int(want):
        assert abs(int(got) - int(want)) == 1, (ctx, int(got), int(want))
        assert _near_boundary_eps(float_score, eps), (ctx, float(float_score), int(got), int(want))
        return 1
    return 0


def test_score_against_oracle_and_golden(golden_case, orc):
    _need_gpu()
    case = golden_case
    e, seqs, res, offs = _load(case)
    deci, flags, fwd, det = e.score(res, offs, want_fwd=True, want_detail=True)
    ohm = [orc.OracleHMM(p) for p in case.hmm_paths]
    od, of, ofwd, osc = orc.score_batch(ohm, res, offs)
    # Forward log-odds within 1e-4 bit of the float64 restatement
    finite = np.isfinite(ofwd)
    # (the output is a float32: above 1024 bits - amino_multidomain - its own spacing exceeds 1e-4; two ulps there)
    tol = np.maximum(1e-4, 2.0 * np.spacing(np.abs(ofwd[finite]).astype(np.float32)).astype(np.float64))
    assert np.all(np.abs(fwd[finite] - ofwd[finite]) <= tol), np.max(np.abs(fwd[finite] - ofwd[finite]) / tol)
    # reported / multidomain / override flags identical
    mism = np.argwhere((flags & 7) != (of & 7))
    assert len(mism) == 0, (case.name, mism[:5], flags[tuple(mism[0])], of[tuple(mism[0])])
    # envelopes identical (stage-by-stage detail)
    H = e.H
    for qi in range(len(seqs)):
        for hj in range(H):
            r = ohm[hj].score(seqs[qi])
            d = det[qi * H + hj]
            assert d.nregions == r.nregions, (case.name, qi, hj)
            assert d.nenv == min(r.nenv, WH_MAX_ENVELOPES), (case.name, qi, hj, d.nenv, r.nenv, r.flags)
            for t in range(d.nenv):
                assert (d.env_i[t], d.env_j[t]) == (r.env_i[t], r.env_j[t]), (case.name, qi, hj, t)
                assert abs(d.envsc[t] - r.envsc[t]) <= 2e-4 * max(1.0, abs(r.envsc[t]) / 50), (case.name, qi, hj, d.envsc[t], r.envsc[t])
                # (a sum of float32 logs over the envelope: the bound grows with its length - 600-residue protein envelopes)
                len_t = max(1.0, (r.env_j[t] - r.env_i[t] + 1) / 250.0)
                assert abs(d.domcorr[t] - r.domcorr[t]) <= (2e-2 if r.env_multi[t] else 1e-3 * len_t), (case.name, qi, hj, d.domcorr[t], r.domcorr[t])
    # deci-bits
    rep = (of & 1) == 1
    diff = (deci != od) & rep
    n_diff = int(diff.sum())
    for qi, hj in np.argwhere(diff):
        assert abs(int(deci[qi, hj]) - int(od[qi, hj])) == 1, (case.name, qi, hj, deci[qi, hj], od[qi, hj])
        assert _near_boundary_eps(osc[qi, hj], LONG_EPS if of[qi, hj] & 2 else BOUNDARY_EPS), (case.name, qi, hj, osc[qi, hj], deci[qi, hj], od[qi, hj])
    # and directly against HMMER's printed scores: every pair, the multidomain class (HMMER's stochastic
    # resolver, reproduced by resolve_kernel) included
    n_exact = n_pairs = n_multi = n_multi_exact = n_multi_noise = n_multi_two = 0
    for hj, hf in enumerate(case.hmm_files):
        S = case.g["search"][hf]
        for qi, qn in enumerate(case.qnames):
            multi = bool(flags[qi, hj] & 2)
            assert bool(flags[qi, hj] & 1) == (qn in S), (case.name, hf, qn, "multidomain" if multi else "single")
            if qn in S:
                n_pairs += 1
                n_multi += multi
                g = int(round(S[qn]["score"] * 10))
                if g == deci[qi, hj]:
                    n_exact += 1
                    n_multi_exact += multi
                elif multi and not _near_boundary_eps(osc[qi, hj], LONG_EPS):
                    # the stochastic class away from a rounding boundary: the float64 ensemble (device == oracle, checked
                    # above) against HMMER's float32 one - a flipped decision desynchronises the later traces of the
                    # region (tests/test_oracle_golden.py): bounded like the oracle's own residual
                    assert abs(g - int(deci[qi, hj])) <= 2, (case.name, hf, qn, g, deci[qi, hj])
                    n_multi_noise += 1
                    n_multi_two += abs(g - int(deci[qi, hj])) == 2
                else:
                    assert abs(g - int(deci[qi, hj])) == 1 and _near_boundary_eps(osc[qi, hj], LONG_EPS if multi else BOUNDARY_EPS), (case.name, hf, qn, g, deci[qi, hj])
    print("\n[%s] GPU vs oracle: %d/%d reported pairs differ (all at a rounding boundary); "
          "GPU vs HMMER print: %d/%d exact (multidomain class %d/%d)" % (case.name, n_diff, int(rep.sum()), n_exact, n_pairs, n_multi_exact, n_multi))
    assert n_exact >= 0.98 * n_pairs
    assert n_multi_noise <= n_multi // 50 and n_multi_two <= n_multi // 100, (n_multi_noise, n_multi_two, n_multi)
    e.close()


def test_topk_against_restatement_and_reference(golden_case, orc):
    _need_gpu()
    case = golden_case
    e, seqs, res, offs = _load(case)
    deci, flags = e.score(res, offs)
    k = case.k
    idx, w, nk, nu = e.topk(deci, flags, k)
    size_of = dict(zip(case.hmm_index, case.nseq))
    for qi, qn in enumerate(case.qnames):
        ranked = orc.rank_bitscores(case.hmm_index, deci[qi], flags[qi] & 1)
        if not ranked:
            assert nk[qi] == 0 and nu[qi] == 0
            continue
        idxs = [r[0] for r in ranked]
        bits = [r[1] for r in ranked]
        ref = orc.calculate_weights(idxs, bits, [size_of[i] for i in idxs], k)
        assert nk[qi] == len(ref)
        got_w = w[qi, :nk[qi]]
        ref_w = np.array([x[1] for x in ref])
        assert np.allclose(got_w, ref_w, rtol=1e-12, atol=0), (case.name, qn, got_w, ref_w)
        # identical order except inside groups of weights equal to 1e-12 (float64 noise in numpy's formula)
        got_i = idx[qi, :nk[qi]].tolist()
        ref_i = [x[0] for x in ref]
        if got_i != ref_i:
            for a, b, wa, wb in zip(got_i, ref_i, got_w, ref_w):
                if a != b:
                    assert abs(wa - wb) <= 1e-12 * max(wa, wb), (case.name, qn, got_i, ref_i)
        assert nu[qi] == orc.adaptive_cut(list(zip(got_i, got_w))), (case.name, qn)
    e.close()


def test_align_against_oracle_and_reference(golden_case, orc):
    _need_gpu()
    case = golden_case
    e, seqs, res, offs = _load(case)
    pos_of = {idx: i for i, idx in enumerate(case.hmm_index)}
    pq, ph, gold = [], [], []
    for qi, qn in enumerate(case.qnames):
        if qn not in case.g["align"]:
            continue
        for idx, cols in case.g["align"][qn]["cols"].items():
            pq.append(qi)
            ph.append(pos_of[int(idx)])
            gold.append(cols)
    # plus every (query, model 0) pair, including unrelated / very short queries
    for qi in range(len(seqs)):
        pq.append(qi)
        ph.append(0)
        gold.append(None)
    cols, co = e.align(res, offs, pq, ph)
    ohm = [orc.OracleHMM(p) for p in case.hmm_paths]
    n_gold = n_bad = 0
    for p in range(len(pq)):
        got = cols[co[p]:co[p + 1]].tolist()
        want = ohm[ph[p]].align(seqs[pq[p]]).tolist()
        assert got == want, (case.name, "vs oracle", pq[p], ph[p], [(i, a, b) for i, (a, b) in enumerate(zip(got, want)) if a != b][:5])
        if gold[p] is not None:
            n_gold += 1
            n_bad += got != gold[p]
    assert n_bad == 0, (case.name, n_bad, n_gold)
    e.close()


def test_device_tensor_entry_points_match_host_entry_points():
    _need_gpu()
    import torch
    from tests.conftest import load_case
    case = load_case("dna_synth")
    e, seqs, res, offs = _load(case)
    deci, flags = e.score(res, offs)
    rt = torch.from_numpy(res).cuda()
    ot = torch.from_numpy(offs).cuda()
    maxlen = int(np.max(np.diff(offs)))
    d2, f2 = e.score_t(rt, ot, maxlen)
    torch.cuda.synchronize()
    assert np.array_equal(d2.cpu().numpy(), deci) and np.array_equal(f2.cpu().numpy(), flags)
    idx, w, nk, nu = e.topk(deci, flags, 3)
    i2, w2, nk2, nu2 = e.topk_t(d2, f2, 3)
    torch.cuda.synchronize()
    assert np.array_equal(i2.cpu().numpy(), idx) and np.array_equal(w2.cpu().numpy(), w)
    assert np.array_equal(nk2.cpu().numpy(), nk) and np.array_equal(nu2.cpu().numpy(), nu)
    e.close()


def test_edge_cases_empty_and_ragged():
    _need_gpu()
    from tests.conftest import load_case
    from witch_amd.ehmm import EHMM, pack_queries
    case = load_case("dna_synth")
    e = EHMM(case.hmm_paths)
    # no queries at all
    d, f = e.score(np.zeros(0, np.uint8), np.zeros(1, np.int64))
    assert d.shape == (0, e.H)
    # an empty query between two normal ones: HMMER silently skips length-0 sequences
    seqs = [e.digitize(case.qseqs[0]), np.zeros(0, np.uint8), e.digitize(case.qseqs[1])]
    res, offs = pack_queries(seqs)
    d, f = e.score(res, offs)
    assert f[1].sum() == 0 and d[1].sum() == 0
    d0, f0 = e.score(*pack_queries([seqs[0]]))
    assert np.array_equal(d[0], d0[0]) and np.array_equal(f[0], f0[0])
    idx, w, nk, nu = e.topk(d, f, 4)
    assert nk[1] == 0 and nu[1] == 0 and (idx[1] == -1).all()
    cols, co = e.align(res, offs, [1, 0], [0, 0])
    assert co.tolist() == [0, 0, len(seqs[0])]
    # illegal residue codes are rejected loudly
    with pytest.raises(Exception):
        e.score(np.array([200], np.uint8), np.array([0, 1], np.int64))
    e.close()


@pytest.mark.parametrize("case_name,lengths", [("amino_hmmbuild", (900, 2000)), ("dna_synth", (1200, 3000))])
def test_long_queries_keep_special_states_in_hbm(case_name, lengths, orc):
    """Queries too long for the per-wave LDS block (BASELINE config 5: up to 2000 aa) switch the
    kernels to the HBM-resident special-state rows; results must still match the oracle."""
    _need_gpu()
    from tests.conftest import load_case
    from witch_amd import synth
    from witch_amd.ehmm import EHMM, pack_queries
    case = load_case(case_name)
    e = EHMM(case.hmm_paths, hmm_index=case.hmm_index, nseq=case.nseq)
    rng = np.random.default_rng(3)
    K = 20 if case.alphabet == "amino" else 4
    bg = synth.background(case.alphabet)
    # long queries: a real query embedded in random background flanks (+ one pure background)
    seqs = []
    for t in range(5):
        L = int(rng.integers(lengths[0], lengths[1] + 1))
        core = e.digitize(case.qseqs[t])
        s = rng.choice(K, size=L, p=bg).astype(np.uint8)
        if t < 4:
            at = int(rng.integers(0, L - len(core)))
            s[at:at + len(core)] = core
        seqs.append(s)
    res, offs = pack_queries(seqs)
    deci, flags, fwd = e.score(res, offs, want_fwd=True)
    ohm = [orc.OracleHMM(p) for p in case.hmm_paths]
    od, of, ofwd, osc = orc.score_batch(ohm, res, offs)
    assert np.max(np.abs(fwd - ofwd)) <= 2e-4, np.max(np.abs(fwd - ofwd))   # float32 ulp at ~2000 rows
    assert np.array_equal(flags & 3, of & 3)
    rep = (of & 1) == 1
    for qi, hj in np.argwhere((deci != od) & rep):
        assert abs(int(deci[qi, hj]) - int(od[qi, hj])) == 1 and _near_boundary(osc[qi, hj]), (qi, hj, deci[qi, hj], od[qi, hj], osc[qi, hj])
    pq = [q for q in range(len(seqs)) for _ in range(2)]
    ph = [h % e.H for q in range(len(seqs)) for h in (0, 1)]
    cols, co = e.align(res, offs, pq, ph)
    for p in range(len(pq)):
        want = ohm[ph[p]].align(seqs[pq[p]])
        got = cols[co[p]:co[p + 1]]
        assert np.array_equal(got, want), (case_name, pq[p], ph[p], int((got != want).sum()))
    e.close()


def test_consensus_merge_against_oracle_and_reference(golden_case):
    """Next row #1: the witch-ng weighted consensus DP (aligner.py:376-495) on the GPU,
    end to end through the reference-shaped functions; bit-exact float64 arithmetic, so the
    aligned strings must equal the reference's own alignSubQueriesNew output."""
    _need_gpu()
    from oracle import consensus as ocons
    from witch_amd import gcmm
    case = golden_case
    g = case.g
    if not g.get("merged"):
        pytest.skip("case has no backbone alignment")

    class _Sub:
        def __init__(self, path, n):
            self.hmm_model_path, self.num_taxa = path, n
    index_to_hmm = {i: _Sub(p, n) for i, p, n in zip(case.hmm_index, case.hmm_paths, case.nseq)}
    retained = {int(k): v for k, v in g["retained"].items()}
    nongaps = {int(k): v for k, v in g["nongaps"].items()}
    eng = gcmm.install(gcmm.QueryAlignmentEngine.run(
        index_to_hmm, list(zip(case.qnames, case.qseqs)), case.k,
        subset_to_retained_columns=retained, subset_to_nongaps_per_column=nongaps,
        backbone_length=g["backbone_length"]))
    ranked = gcmm.rankBitscores(index_to_hmm, {})
    weights = gcmm.writeWeights(index_to_hmm, ranked)
    n_ref = n_orc = 0
    for q, (qn, qs) in enumerate(zip(case.qnames, case.qseqs)):
        if qn not in weights:
            continue
        query, _, _ = gcmm.alignSubQueriesNew("bb", g["backbone_length"], index_to_hmm, None, 120, qn, qs, weights[qn], q)
        got = query[qn]
        # oracle on the GPU path's own inputs (same top-k order and weights)
        _, wmap, cols = gcmm.getBackbones(index_to_hmm, qn, q, qs, "p", weights[qn], ".", ".", use_gcm=False)
        codes, _ = ocons.consensus_trace(len(qs), list(cols.items()), wmap, retained, nongaps, g["backbone_length"])
        assert got == ocons.trace_to_string(qs, codes, g["backbone_length"]), (case.name, qn)
        n_orc += 1
        # and the reference's own output, whenever the reference's tie order among equal weights
        # did not pick a different (equally weighted) set of HMMs
        want = g["merged"].get(qn)
        gold_w = g["weights"].get(qn)      # absent: HMMER reported no HMM (multidomain class)
        tied = gold_w is None or len(set(x[1] for x in gold_w)) < len(gold_w)
        same_hmms = gold_w is not None and [i for i, _ in gold_w] == [i for i, _ in weights[qn]]
        if want is not None and not tied and same_hmms:
            assert got == want, (case.name, qn)
            n_ref += 1
        labels = query._col_labels
        assert sum(1 for x in labels if x >= 0) == g["backbone_length"] and len(labels) == len(got)
    assert n_orc > 0 and n_ref > 0


@pytest.mark.parametrize("root_len", [1700, 2574, 2950])
def test_long_models_use_the_pass_synchronous_kernels(root_len, orc, tmp_path):
    """Models beyond 1536 nodes (the reference's example backbone has up to 2574 match
    columns) run with one transition orientation resident in LDS; parity with the oracle."""
    _need_gpu()
    from witch_amd import synth
    from witch_amd.ehmm import EHMM, pack_queries
    fam = synth.make_family(77 + root_len, root_len, 8, "dna", 0.03, 0.001)
    eh = synth.make_ehmm(fam, 3, str(tmp_path), witch_layout=False)
    assert max(h.M for h in eh.hmms) > 1536
    names, seqs = synth.make_queries(fam, 5, 6, (80, 160))
    rng = np.random.default_rng(1)
    seqs.append(rng.integers(0, 4, size=120).astype(np.int8))     # unrelated
    seqs = [s.astype(np.uint8) for s in seqs]
    e = EHMM(eh.paths, hmm_index=eh.index, nseq=eh.nseq)
    res, offs = pack_queries(seqs)
    deci, flags, fwd = e.score(res, offs, want_fwd=True)
    ohm = [orc.OracleHMM(p) for p in eh.paths]
    od, of, ofwd, osc = orc.score_batch(ohm, res, offs)
    assert np.max(np.abs(fwd - ofwd)) <= 1e-4, np.max(np.abs(fwd - ofwd))
    assert np.array_equal(flags & 3, of & 3)
    rep = (of & 1) == 1
    for qi, hj in np.argwhere((deci != od) & rep):
        assert abs(int(deci[qi, hj]) - int(od[qi, hj])) == 1 and _near_boundary(osc[qi, hj])
    pq = [q for q in range(len(seqs)) for _ in range(e.H)]
    ph = [h for q in range(len(seqs)) for h in range(e.H)]
    cols, co = e.align(res, offs, pq, ph)
    for p in range(len(pq)):
        want = ohm[ph[p]].align(seqs[pq[p]])
        assert np.array_equal(cols[co[p]:co[p + 1]], want), (root_len, pq[p], ph[p])
    e.close()


def test_long_protein_queries_with_several_hits(orc, tmp_path):
    """Queries of 500-2000 residues that hold several unequal hits to the family (one envelope
    can span two of them): the envelope Backward sweep must keep the best path's cells in float32
    range (mirrored Forward scaling, wh_device.h) - an earlier build lost their posterior mass and
    produced NaN null2 corrections here."""
    _need_gpu()
    from witch_amd import synth
    from witch_amd.ehmm import EHMM, pack_queries
    fam = synth.make_family(20251206, 600, 64, "amino", 0.03, 1e-4)
    eh = synth.make_ehmm(fam, 6, str(tmp_path), witch_layout=False)
    names, seqs = synth.make_queries(fam, 20251207, 16, (500, 2000), flank_frac=0.3)
    seqs = [s.astype(np.uint8) for s in seqs]
    e = EHMM(eh.paths, hmm_index=eh.index, nseq=eh.nseq)
    res, offs = pack_queries(seqs)
    deci, flags, fwd, det = e.score(res, offs, want_fwd=True, want_detail=True)
    ohm = [orc.OracleHMM(p) for p in eh.paths]
    od, of, ofwd, osc = orc.score_batch(ohm, res, offs)
    assert np.max(np.abs(fwd - ofwd)) <= 2e-4 * np.maximum(1.0, np.abs(ofwd) / 1000).max()
    assert np.array_equal(flags & 3, of & 3)
    assert ((of & 2) != 0).sum() > 0          # the case does contain multi-hit envelopes
    assert not ((flags & 16) != 0).any()      # and none needed the dense redo
    for d in det:
        for t in range(d.nenv):
            assert np.isfinite(d.domcorr[t]) and np.isfinite(d.envsc[t])
    n_bad = _check_decibits(deci, od, osc, (of & 1) == 1, "long protein", LONG_EPS)
    print("\n[long protein] %d of %d reported pairs one deci-bit off (all within %.2f bit of a boundary); %d multidomain pairs"
          % (n_bad, int(((of & 1) == 1).sum()), LONG_EPS, int(((of & 2) != 0).sum())))
    # alignment of the same queries: where the best hit is not the first one the scaled float32
    # sweeps cannot represent it (HMMER's Decoding overflows there and hmmalign switches to its
    # log-space code); the kernel detects the same condition and redoes those pairs in log space
    # (wh_align_log.h).  Every pair must equal the oracle; before this fallback a quarter did not.
    pq = [q for q in range(8) for _ in range(e.H)]
    ph = [h for q in range(8) for h in range(e.H)]
    cols, co = e.align(res, offs, pq, ph)
    for p in range(len(pq)):
        want = ohm[ph[p]].align(seqs[pq[p]])
        assert np.array_equal(cols[co[p]:co[p + 1]], want), (pq[p], ph[p])
    e.close()


def test_level0_shims_reproduce_hmmer_outputs(tmp_path):
    """WITCH's own plug-in boundary (hmmsearchpath / hmmalignpath): the C clients + the resident
    GPU server, driven with the reference's exact command lines, against HMMER's golden results
    parsed the way the reference parses them."""
    _need_gpu()
    import os
    import subprocess
    import threading
    from tests.conftest import load_case, ROOT
    from tests.refparse import evalHMMSearchOutput
    from witch_amd.shim import formats
    from witch_amd.shim.server import Server, GpuBackend
    bindir = os.path.join(ROOT, "witch_amd", "shim", "bin")
    subprocess.run(["make", "-C", os.path.join(ROOT, "witch_amd", "shim")], check=True, stdout=subprocess.DEVNULL)
    sock = str(tmp_path / "gpu.sock")
    srv = Server(GpuBackend(0), sock)
    ready = threading.Event()
    threading.Thread(target=srv.serve_forever, args=(ready,), daemon=True).start()
    assert ready.wait(10)
    env = dict(os.environ, WITCH_HIP_SOCKET=sock)
    case = load_case("dna_hmmbuild")
    fa = os.path.join(case.dir, "queries.fasta")
    n_scores = n_aln = 0
    for hf, hp in list(zip(case.hmm_files, case.hmm_paths))[:4]:
        out = str(tmp_path / ("hmmsearch.results." + os.path.basename(hf)))
        r = subprocess.run([os.path.join(bindir, "hmmsearch"), "--cpu", "1", "--noali", "-E", "99999999", "-o", out,
                            "--max", hp, fa], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        got = evalHMMSearchOutput(out)
        want = case.g["search"][hf]
        multi = {q for q, v in want.items() if len(v.get("dom", [0])) != 1}     # stochastic multidomain class
        # sequences whose only regions are multidomain (HMMER resolves those stochastically) may be
        # reported on one side only: the same tolerance class as test_score_against_oracle_and_golden
        assert len(set(got) ^ set(want)) <= max(1, len(want) // 20), (hf, set(got) ^ set(want))
        for q, (ev, sc) in got.items():
            if q in multi or q not in want:
                continue
            assert abs(sc - want[q]["score"]) <= 0.1001, (hf, q, sc, want[q]["score"])
            n_scores += sc == want[q]["score"]
    seqs = dict(zip(case.qnames, case.qseqs))
    procs = []
    for qn, a in list(case.g["align"].items())[:12]:
        one = tmp_path / (qn + ".fa")
        one.write_text(">%s\n%s\n" % (qn, seqs[qn]))
        for idx, cols in a["cols"].items():
            hp = case.hmm_paths[case.hmm_index.index(int(idx))]
            out = str(tmp_path / ("hmmalign.%s.%s.out" % (qn, idx)))
            procs.append((subprocess.Popen([os.path.join(bindir, "hmmalign"), "-o", out, hp, str(one)], env=env), out, qn, cols))
    for p, out, qn, cols in procs:
        assert p.wait() == 0
        row = "".join(l.split()[1] for l in open(out) if l.strip() and not l.startswith("#") and l.strip() != "//")
        assert formats.decode_stockholm_row(row) == list(cols), (qn, out)
        n_aln += 1
    assert n_scores > 50 and n_aln > 10


def test_long_queries_on_20_and_24_cell_models(orc, tmp_path):
    """Models of 1025-1536 nodes with queries too long for the LDS special-state rows: the
    phase-call kernel's HBM mode at 20 / 24 cells per lane (an older fused variant hung there)."""
    _need_gpu()
    from witch_amd import synth
    from witch_amd.ehmm import EHMM, pack_queries
    for root_len in (1200, 1450):
        fam = synth.make_family(31 + root_len, root_len, 16, "dna", 0.03, 1e-4)
        eh = synth.make_ehmm(fam, 3, str(tmp_path / ("m%d" % root_len)), witch_layout=False)
        names, seqs = synth.make_queries(fam, 9, 6, (700, root_len - 50))
        seqs = [s.astype(np.uint8) for s in seqs]
        e = EHMM(eh.paths, hmm_index=eh.index, nseq=eh.nseq)
        assert 1024 < int(e.M.max()) <= 1536
        res, offs = pack_queries(seqs)
        deci, flags, fwd = e.score(res, offs, want_fwd=True)
        ohm = [orc.OracleHMM(p) for p in eh.paths]
        od, of, ofwd, osc = orc.score_batch(ohm, res, offs)
        assert np.max(np.abs(fwd - ofwd)) <= 2e-4
        assert np.array_equal(flags & 3, of & 3)
        _check_decibits(deci, od, osc, (of & 1) == 1, ("20/24-cell long", root_len), LONG_EPS)
        e.close()


@pytest.mark.parametrize("root_len", [200, 450, 700, 950])
def test_every_kernel_instantiation_against_the_oracle(root_len, orc, tmp_path):
    """4/8/12/16 cells per lane x query lengths that select 12 waves with LDS special states,
    fewer waves (the 512-thread build) and the HBM special-state mode: scores and flags against
    the oracle for every scoring-kernel instantiation the planner can pick for these models."""
    _need_gpu()
    from witch_amd import synth
    from witch_amd.ehmm import EHMM, pack_queries
    fam = synth.make_family(900 + root_len, root_len, 16, "dna", 0.03, 1e-4)
    eh = synth.make_ehmm(fam, 3, str(tmp_path), witch_layout=False)
    e = EHMM(eh.paths, hmm_index=eh.index, nseq=eh.nseq)
    ohm = [orc.OracleHMM(p) for p in eh.paths]
    rng = np.random.default_rng(root_len)
    bg = synth.background("dna")
    for qlen in (120, 330, 520, 1100):
        names, seqs = synth.make_queries(fam, 7 + qlen, 6, min(qlen, root_len - 20))
        out = []
        for s_ in seqs:                       # embed the window in random flanks up to the wanted length
            s_ = s_.astype(np.uint8)
            pad = qlen - len(s_)
            if pad > 0:
                a = int(rng.integers(0, pad + 1))
                s_ = np.concatenate([rng.choice(4, size=a, p=bg), s_, rng.choice(4, size=pad - a, p=bg)]).astype(np.uint8)
            out.append(s_)
        res, offs = pack_queries(out)
        deci, flags, fwd = e.score(res, offs, want_fwd=True)
        od, of, ofwd, osc = orc.score_batch(ohm, res, offs)
        assert np.max(np.abs(fwd - ofwd)) <= 2e-4, (root_len, qlen)
        assert np.array_equal(flags & 3, of & 3), (root_len, qlen)
        _check_decibits(deci, od, osc, (of & 1) == 1, (root_len, qlen), BOUNDARY_EPS if qlen <= 330 else LONG_EPS)
    e.close()


@pytest.mark.parametrize("root_len", [200, 450, 700, 950, 1300])
def test_resolver_on_every_forward_class(root_len, orc, tmp_path):
    """Queries that hold two or three copies of the family (multidomain regions: HMMER's stochastic
    resolver) on models of 4/8/12/16 nodes per lane - the resolver's register-resident
    Forward (wh_resolve.hip gforward_reg<4..16>) - and of 24 (its slab version): the resolved scores
    against the oracle's, which runs the same 200 seeded tracebacks in float64."""
    _need_gpu()
    from witch_amd import synth
    from witch_amd.ehmm import EHMM, pack_queries
    fam = synth.make_family(7100 + root_len, root_len, 16, "dna", 0.03, 1e-4)
    eh = synth.make_ehmm(fam, 2, str(tmp_path), witch_layout=False)
    names, seqs = synth.make_queries(fam, 23 + root_len, 8, (2 * root_len, 3 * root_len), flank_frac=0.3)
    seqs = [s_.astype(np.uint8) for s_ in seqs]
    e = EHMM(eh.paths, hmm_index=eh.index, nseq=eh.nseq)
    res, offs = pack_queries(seqs)
    deci, flags, fwd = e.score(res, offs, want_fwd=True)
    ohm = [orc.OracleHMM(p) for p in eh.paths]
    od, of, ofwd, osc = orc.score_batch(ohm, res, offs)
    assert int(((flags & 2) != 0).sum()) >= 3, "the case is meant to have multidomain pairs"
    assert np.array_equal(flags & 3, of & 3), root_len
    assert np.max(np.abs(fwd - ofwd)) <= 2e-4 * max(1.0, root_len / 500.0), root_len
    _check_decibits(deci, od, osc, (of & 1) == 1, root_len, LONG_EPS)
    e.close()


@pytest.mark.parametrize("root_len,alphabet", [(3300, "dna"), (5200, "dna"), (3200, "amino")])
def test_models_beyond_3072_nodes_take_the_any_size_kernels(root_len, alphabet, orc, tmp_path):
    """Models the register-resident kernels cannot hold (wh_generic.hip: float64, rows in HBM): scores, flags and
    aligned columns against the oracle - short fragments, fragments in random flanks, and queries with two copies
    of the family (multidomain regions: front end + resolver)."""
    _need_gpu()
    from witch_amd import synth
    from witch_amd.ehmm import EHMM, pack_queries
    fam = synth.make_family(9100 + root_len, root_len, 16, alphabet, 0.03, 1e-4)
    eh = synth.make_ehmm(fam, 2, str(tmp_path), witch_layout=False)
    # one more model of ordinary size: the two paths share a call
    fam2 = synth.make_family(9200 + root_len, 400, 16, alphabet, 0.03, 1e-4)
    eh2 = synth.make_ehmm(fam2, 1, str(tmp_path / "small"), witch_layout=False)
    paths = eh.paths + eh2.paths
    e = EHMM(paths, hmm_index=list(range(len(paths))), nseq=eh.nseq + eh2.nseq)
    assert int(e.M.max()) > 3072
    rng = np.random.default_rng(root_len)
    bg = synth.background(alphabet)
    K = len(bg)
    _, short = synth.make_queries(fam, 5, 4, 150)
    _, mid = synth.make_queries(fam, 6, 3, 600)
    _, multi = synth.make_queries(fam, 7, 3, (root_len + 500, 2 * root_len), flank_frac=0.3)
    _, other = synth.make_queries(fam2, 8, 2, 200)
    seqs = [s_.astype(np.uint8) for s_ in short]
    for s_ in mid:
        a = int(rng.integers(10, 80))
        seqs.append(np.concatenate([rng.choice(K, size=a, p=bg), s_, rng.choice(K, size=90 - a, p=bg)]).astype(np.uint8))
    seqs += [s_.astype(np.uint8) for s_ in multi] + [s_.astype(np.uint8) for s_ in other]
    res, offs = pack_queries(seqs)
    deci, flags, fwd = e.score(res, offs, want_fwd=True)
    ohm = [orc.OracleHMM(p) for p in paths]
    od, of, ofwd, osc = orc.score_batch(ohm, res, offs)
    assert np.max(np.abs(fwd - ofwd)) <= 1e-3, np.max(np.abs(fwd - ofwd))
    assert np.array_equal(flags & 3, of & 3)
    _check_decibits(deci, od, osc, (of & 1) == 1, root_len, LONG_EPS)
    # round 4: the several-waves-per-pair kernel stores only the lanes of an envelope's Forward rows that matter (per-row
    # lane masks, posterior-mass certificate) and, up to 6 144 nodes, reads its emission rows from LDS: with every row
    # stored / the rows read from L2 (environment, read per call) the scores are the same numbers
    for knob in ("WH_WIDE_DENSE", "WH_WIDE_NO_EM_LDS"):
        os.environ[knob] = "1"
        try:
            deci2, flags2, fwd2 = e.score(res, offs, want_fwd=True)
        finally:
            os.environ.pop(knob, None)
        assert np.array_equal(fwd2, fwd), knob
        assert np.array_equal(flags2 & 7, flags & 7), knob
        single = (flags & 2) == 0          # (multidomain pairs: the resolver's float64 path, unchanged by the knobs but checked above)
        assert np.max(np.abs(deci2[single].astype(np.int64) - deci[single])) <= (1 if knob == "WH_WIDE_DENSE" else 0), knob
        assert np.array_equal(deci2[~single], deci[~single]), knob
    # alignment, every pair: the two-copy queries hold two hits of thousands of bits each in ONE unihit alignment,
    # beyond the range of a scaled double - the oracle switches to long double there, hmmalign to log space, the
    # any-size kernel to its log-space twins
    pq = [q for q in range(len(seqs)) for _ in range(e.H)]
    ph = [h for q in range(len(seqs)) for h in range(e.H)]
    cols, co = e.align(res, offs, pq, ph)
    for p in range(len(pq)):
        if not (of[pq[p], ph[p]] & 1):
            continue
        want = ohm[ph[p]].align(seqs[pq[p]])
        assert np.array_equal(cols[co[p]:co[p + 1]], want), (pq[p], ph[p])
    e.close()


@pytest.mark.parametrize("ehmm_source", ["model_files", "wh_hmmbuild"])
def test_level1_chain_with_a_backbone_of_more_than_3072_columns(tmp_path, ehmm_source):
    """The reference-shaped functions end to end on a family whose models have ~3 300 nodes: engine (scores, top-k,
    alignment, consensus), the per-query strings and both mergers.  Every query row of the merged alignment spells its
    query, and the device merge writes the host merger's bytes."""
    _need_gpu()
    from witch_amd import gcmm, synth
    fam = synth.make_family(4711, 3300, 16, "dna", 0.03, 1e-4)
    se = synth.make_ehmm(fam, 3, str(tmp_path), witch_layout=True)
    assert min(h.M for h in se.hmms) > 3072
    names, seqs = synth.make_queries(fam, 31, 24, (150, 500))

    class _Sub:
        def __init__(self, path, n):
            self.hmm_model_path, self.num_taxa = path, n

    index_to_hmm = {i: _Sub(p, n) for i, p, n in zip(se.index, se.paths, se.nseq)}
    retained = {i: (h.map_cols[1:] - 1).tolist() for i, h in zip(se.index, se.hmms)}
    nongaps = {i: h.nongaps.tolist() for i, h in zip(se.index, se.hmms)}
    B = fam.msa.shape[1]
    if ehmm_source == "wh_hmmbuild":
        # the same three subsets built from the backbone rows by the hmmbuild equivalent (no model file from elsewhere)
        sym = "ACGT"
        rows = ["".join(sym[c] if c >= 0 else "-" for c in fam.msa[i]) for i in range(fam.msa.shape[0])]
        subsets = [("A_0_%d" % idx, list(range(lo, hi))) for idx, (lo, hi) in enumerate(synth.bfs_subsets(fam.n_leaves, 3))]
        built = gcmm.build_ehmm(list(fam.names), rows, subsets, "dna", str(tmp_path / "built"))
        index_to_hmm = {idx: _Sub(b[0], len(subsets[idx][1])) for idx, b in enumerate(built)}
        retained = {idx: list(b[2]) for idx, b in enumerate(built)}
        nongaps = {idx: list(b[3]) for idx, b in enumerate(built)}
    texts = [synth.to_text(s_, "dna") for s_ in seqs]
    bpath = str(tmp_path / "backbone.fasta")
    synth.write_msa_fasta(bpath, fam, 0, 16)
    eng = gcmm.install(gcmm.QueryAlignmentEngine.run(index_to_hmm, list(zip(names, texts)), 3, subset_to_retained_columns=retained,
                                                     subset_to_nongaps_per_column=nongaps, backbone_length=B))
    ranked = gcmm.rankBitscores(index_to_hmm, {})
    weights = gcmm.writeWeights(index_to_hmm, ranked)
    assert len(weights) == len(names)
    queries = [gcmm.alignSubQueriesNew(bpath, B, index_to_hmm, None, 0, t, s_, weights[t], i)[0]
               for i, (t, s_) in enumerate(zip(names, texts))]
    out_host, out_dev = str(tmp_path / "out.fasta"), str(tmp_path / "out_dev.fasta")
    gcmm.mergeAlignmentsCollapsed(bpath, queries, {}, None, output_path=out_host)
    gcmm.mergeAlignmentsDevice(bpath, {}, output_path=out_dev, taxa=list(names))
    assert open(out_host, "rb").read() == open(out_dev, "rb").read()
    rows = {}
    name = None
    for line in open(out_host):
        line = line.strip()
        if line.startswith(">"):
            name = line[1:]
            rows[name] = []
        elif name is not None:
            rows[name].append(line)
    width = {len("".join(v)) for v in rows.values()}
    assert len(width) == 1
    for t, s_ in zip(names, texts):
        row = "".join(rows[t])
        assert row.replace("-", "").upper() == s_.upper(), t
        assert sum(1 for ch in row if ch.isupper()) > 0.8 * len(s_), t      # a family member: mostly match columns
    assert eng is not None


def test_multihit_queries_on_a_long_model_align_like_hmmalign(orc, tmp_path):
    """1900-node models (pass-synchronous kernels) with queries that hold two or three copies of
    the family: the pairs leave float32 range and go through the log-space pass."""
    _need_gpu()
    from witch_amd import synth
    from witch_amd.ehmm import EHMM, pack_queries
    fam = synth.make_family(4242 + 1900, 1900, 16, "dna", 0.03, 1e-4)
    eh = synth.make_ehmm(fam, 2, str(tmp_path), witch_layout=False)
    names, seqs = synth.make_queries(fam, 17, 4, (2100, 4200), flank_frac=0.3)
    seqs = [s.astype(np.uint8) for s in seqs]
    e = EHMM(eh.paths, hmm_index=eh.index, nseq=eh.nseq)
    assert int(e.M.max()) > 1536
    res, offs = pack_queries(seqs)
    ohm = [orc.OracleHMM(p) for p in eh.paths]
    pq = [q for q in range(len(seqs)) for _ in range(e.H)]
    ph = [h for q in range(len(seqs)) for h in range(e.H)]
    cols, co = e.align(res, offs, pq, ph)
    for p in range(len(pq)):
        want = ohm[ph[p]].align(seqs[pq[p]])
        assert np.array_equal(cols[co[p]:co[p + 1]], want), (pq[p], ph[p])
    e.close()


@pytest.mark.parametrize("seed", [11, 12, 13, 14, 15, 16])
def test_randomised_small_cases(seed, orc, tmp_path):
    """Random families (both alphabets, 20-400 nodes), ragged query lengths from 1 residue up,
    degenerate residue codes, unrelated sequences: scores, flags and aligned columns against the
    oracle through the C ABI."""
    _need_gpu()
    from witch_amd import synth
    from witch_amd.ehmm import EHMM, pack_queries
    rng = np.random.default_rng(seed)
    alph = "amino" if seed % 2 else "dna"
    root = int(rng.integers(20, 400))
    fam = synth.make_family(1000 + seed, root, 8, alph, 0.05, 2e-3)
    eh = synth.make_ehmm(fam, 3, str(tmp_path), witch_layout=False)
    e = EHMM(eh.paths, hmm_index=eh.index, nseq=eh.nseq)
    K = 20 if alph == "amino" else 4
    Kp = 29 if alph == "amino" else 18
    bg = synth.background(alph)
    seqs = []
    for t in range(14):
        L = int(rng.choice([1, 2, 3, 7, 25, 60, 150, 333, 401]))
        if t % 3 == 0:
            s_ = rng.choice(K, size=L, p=bg).astype(np.uint8)                 # unrelated
        else:
            _, w = synth.make_queries(fam, seed * 100 + t, 1, min(L, root - 1) if root > 2 else 1)
            s_ = w[0].astype(np.uint8)
        if t % 4 == 1 and len(s_) > 4:                                       # degenerate codes (not gap/*/~)
            pos = rng.integers(0, len(s_), size=max(1, len(s_) // 10))
            lo = K
            hi = Kp - 3
            s_ = s_.copy()
            s_[pos] = rng.integers(lo, hi, size=len(pos)).astype(np.uint8)
        seqs.append(s_)
    res, offs = pack_queries(seqs)
    deci, flags, fwd = e.score(res, offs, want_fwd=True)
    ohm = [orc.OracleHMM(p) for p in eh.paths]
    od, of, ofwd, osc = orc.score_batch(ohm, res, offs)
    fin = np.isfinite(ofwd)
    assert np.array_equal(np.isfinite(fwd), fin)
    assert np.max(np.abs(fwd[fin] - ofwd[fin])) <= 1e-4
    assert np.array_equal(flags & 3, of & 3)
    _check_decibits(deci, od, osc, (of & 1) == 1, ("random", seed))
    pq = [q for q in range(len(seqs)) for _ in range(e.H)]
    ph = [h for q in range(len(seqs)) for h in range(e.H)]
    cols, co = e.align(res, offs, pq, ph)
    for p in range(len(pq)):
        want = ohm[ph[p]].align(seqs[pq[p]])
        assert np.array_equal(cols[co[p]:co[p + 1]], want), (seed, pq[p], ph[p], len(seqs[pq[p]]))
    e.close()


def test_bench_line_contract(tmp_path):
    """bench.py --full prints ONE JSON line with the driver's keys, the roofline object and the CPU baseline."""
    _need_gpu()
    import json
    import os
    import subprocess
    import sys
    from tests.conftest import ROOT
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--nq", "192", "--nh", "6", "--steps", "1", "--warmup", "0", "--full"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    j = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in j, k
    assert j["n_gpus"] == 1 and j["steps"] == 1 and j["warmup"] == 0 and j["higher_is_better"] is True
    assert j["value"] > 0 and j["unit"] == "queries/s" and j["dtype"] == "f32" and j["data"] == "synthetic"
    assert "workload" in j["config"] and "model" not in j["config"]
    rf = j["roofline"]
    assert rf["bound"] == "valu" and rf["unit"] == "TFLOP/s" and rf["peak"] == 157.3
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3 and "traffic" in rf
    assert rf["spill_bytes_stored_per_step_live"] > 0                       # the live device counter of the Forward-row spill
    assert abs(rf["achieved"] - rf["cells_per_launch"] * 77 / (rf["kernel_ms_avg"] * 1e-3) / 1e12) < 0.02 * rf["achieved"] + 0.01
    ra = j["roofline_align"]
    assert ra["bound"] == "hbm" and ra["unit"] == "GB/s" and abs(ra["frac"] - ra["achieved"] / 8000.0) < 1e-3
    assert set(j["distributions"]) >= {"n_used", "multidomain_frac", "regions_per_pair"}
    assert j["extra_stage_ms"]["consensus_rank0"] > 0
    cb = j["cpu_baseline"]
    assert cb["kind"] in ("port", "reference") and cb["cores"] >= 1 and cb["value"] > 0 and cb["sample"]


def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """A plain bench.py run times the hot path only: --steps timed steps, the headline keys and ms_per_step, none of
    what --full adds.  --dump-outputs writes the last step's results as float32 / float64 .npy files within 64 MB,
    and a second run with the same arguments writes the same arrays."""
    _need_gpu()
    import json
    import os
    import subprocess
    import sys
    from tests.conftest import ROOT
    dumps = []
    for run in range(2):
        d = tmp_path / ("out%d" % run)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--nq", "192", "--nh", "6", "--steps", "3",
                            "--warmup", "1", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        j = json.loads(lines[0])
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config"):
            assert k in j, k
        assert j["steps"] == 3 and j["warmup"] == 1 and j["unit"] == "queries/s" and j["dtype"] == "f32"
        assert j["ms_per_step"] > 0 and abs(j["value"] - 192 * 1e3 / j["ms_per_step"]) < 0.01 * j["value"]
        for k in ("roofline", "roofline_align", "distributions", "extra_stage_ms", "level1_e2e", "also", "cpu_baseline"):
            assert k not in j, k
        files = sorted(os.listdir(d))
        assert "topk_index.npy" in files and "align_cols_sample.npy" in files
        assert sum(os.path.getsize(d / f) for f in files) <= 64e6
        arrays = {f[:-len(".npy")]: np.load(d / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert arrays["topk_index"].shape == (192, j["config"]["k"])
        assert int(arrays["topk_n_used"].sum()) == j["config"]["aligned_pairs_per_step"]
        dumps.append(arrays)
    assert dumps[0].keys() == dumps[1].keys()
    for f in dumps[0]:
        assert np.array_equal(dumps[0][f], dumps[1][f]), f


def test_ab_slot_kernel_agrees(golden_case):
    """The A/B slot (the phase-call kernel compiled a second time, option WH_SCORE_KERNEL=8) and the
    development knobs that change the launch plan give the default kernel's results."""
    _need_gpu()
    case = golden_case
    e, seqs, res, offs = _load(case)
    d0, f0 = e.score(res, offs)
    for name, value in (("WH_SCORE_KERNEL", "8"), ("WH_SCORE_KERNEL", "9"), ("WH_MAX_WAVES", "4"), ("WH_FORCE_SPECG", "1")):
        unbanded = value == "9" or name == "WH_FORCE_SPECG"
        if unbanded:            # the two-query kernel and the long-query sweeps store their envelope rows without the lane-block band (spill_band, wh_score7.hip)
            e.set_option("WH_SPILL_BAND", "0")
            d0, f0 = e.score(res, offs)
        e.set_option(name, value)
        d1, f1 = e.score(res, offs)
        e.set_option(name, "")
        assert np.array_equal(f0, f1), (case.name, name)
        assert np.array_equal(d0, d1), (case.name, name)
        if unbanded:
            e.set_option("WH_SPILL_BAND", "")
            d0, f0 = e.score(res, offs)
    with pytest.raises(Exception):
        e.set_option("WH_SCORE_KERNEL", "2")      # removed experiment kernels are refused, not ignored
    e.close()


def test_scoring_on_a_node_window_equals_the_full_width_sweeps(tmp_path):
    """The envelope Backward sweep of the scoring kernel (unihit Backward + posterior accumulation -> null2) on a node
    window against the same sweep at full width (WH_NO_WINDOW): 2 048 headline queries x 200 HMMs.  Flags identical;
    deci-bits identical or one unit apart with the full-width float score at a "%6.1f" rounding boundary;
    and the exported path counters prove that the window ran in one call and did not in the other."""
    _need_gpu()
    import bench
    from witch_amd.ehmm import EHMM, pack_queries
    fam, se, names, seqs, k = bench.make_workload("dna_100k_x200", str(tmp_path), 2048, None)
    e = EHMM(se.paths, hmm_index=se.index, nseq=se.nseq)
    res, offs = pack_queries([s_.astype(np.uint8) for s_ in seqs])
    d_w, f_w, det_w = e.score(res, offs, want_detail=True)
    p_w = e.last_score_paths()
    e.set_option("WH_NO_WINDOW", "1")
    d_f, f_f, det_f = e.score(res, offs, want_detail=True)
    p_f = e.last_score_paths()
    e.set_option("WH_NO_WINDOW", "")
    # the window path ran: most envelopes of a 150-nt fragment fit 256 or 512 nodes.  Every envelope ends in one accepted
    # sweep - a window, or a full-width sweep (directly, or after its window was rejected); a dense redo (rare) adds one
    # more full-width sweep in either run
    n_w = p_w["window256"] + p_w["window512"]
    assert n_w > 0.8 * (n_w + p_w["full_width"]) and n_w > 300000, p_w
    assert p_w["window_rejected"] < 0.01 * n_w, p_w
    assert p_f["window256"] == 0 and p_f["window512"] == 0 and p_f["window_rejected"] == 0, p_f
    assert abs(p_f["full_width"] - (n_w + p_w["full_width"])) <= 16, (p_w, p_f)      # the same envelopes in both runs
    assert np.array_equal(f_w & 15, f_f & 15)
    H = e.H
    sc_f = np.array([d.seq_score for d in det_f], dtype=np.float64).reshape(len(seqs), H)
    moved = _check_decibits(d_w, d_f, sc_f, (f_f & 1) == 1, "scoring window vs full width")
    assert moved <= 8, moved                      # round 3 measured 2 of 1.6 million
    # the Forward side is untouched by the window
    assert all(a.fwd_bits == b.fwd_bits for a, b in zip(det_w[:4096], det_f[:4096]))
    e.close()


def test_envelope_rows_stored_on_a_band_of_lane_blocks_equal_the_unbanded_store(tmp_path):
    """An envelope's Forward sweep stores only the lane blocks around the dominant path of the pair's multihit Forward sweep
    (spill_band, wh_score7.hip) - what the band cuts is posterior mass, and the mass certificate (held to the
    float32 noise band, as for a window) sends an envelope it fails to the dense redo.  Against WH_SPILL_BAND=0 on 2 048
    headline queries x 200 HMMs, on SURVEY's family sketch and on ragged / unrelated / two-copy queries: reported /
    multidomain / override / truncation flags identical, envelopes identical, deci-bits identical or one unit apart at a
    "%6.1f" rounding boundary of the unbanded float score; the live counter proves the band stored less than half the bytes
    on the headline fragments.  An envelope whose band fails the certificate is stored as in round 4 next (every lane block
    that passes the keep rule) and only then densely, so the band adds NO dense redo (WH_FLAG_EXACT identical)."""
    _need_gpu()
    import bench
    from witch_amd.ehmm import EHMM, pack_queries
    rng = np.random.default_rng(23)
    for wl, nq, nh, max_bytes in (("dna_100k_x200", 2048, None, 0.5), ("dna_100k_x200_m1000", 1024, 40, 0.6), ("dna_m1250", 192, 6, 1.0)):
        fam, se, names, seqs, k = bench.make_workload(wl, str(tmp_path / wl), nq, nh)
        e = EHMM(se.paths, hmm_index=se.index, nseq=se.nseq)
        base = [s_.astype(np.uint8) for s_ in seqs]
        extra = []
        if wl != "dna_100k_x200":
            extra = [s_[: int(rng.integers(12, len(s_) + 1))] for s_ in base[:100]]
            extra += [rng.integers(0, 4, size=int(n)).astype(np.uint8) for n in rng.integers(5, 150, size=40)]
            extra += [np.concatenate([s_[:70], s_[:70]]).astype(np.uint8) for s_ in base[:40]]
        res, offs = pack_queries(base + extra)
        d_b, f_b, det_b = e.score(res, offs, want_detail=True)
        bytes_b = e.last_score_spill_bytes()
        e.set_option("WH_SPILL_BAND", "0")
        d_a, f_a, det_a = e.score(res, offs, want_detail=True)
        bytes_a = e.last_score_spill_bytes()
        e.set_option("WH_SPILL_BAND", "")
        assert 0 < bytes_b <= max_bytes * bytes_a, (wl, bytes_b, bytes_a)
        assert np.array_equal(f_b, f_a), wl
        H = e.H
        nall = len(base) + len(extra)
        sc_a = np.array([d.seq_score for d in det_a], dtype=np.float64).reshape(nall, H)
        moved = _check_decibits(d_b, d_a, sc_a, (f_a & 1) == 1, "banded store vs unbanded (%s)" % wl)
        assert moved <= 8, (wl, moved)
        xb, xa = np.ctypeslib.as_array(det_b), np.ctypeslib.as_array(det_a)
        for name in ("nenv", "nregions"):
            assert np.array_equal(xb[name], xa[name]), (wl, name)
        used = np.arange(xa["domcorr"].shape[1])[None, :] < xa["nenv"][:, None]
        for name in ("env_i", "env_j"):
            assert np.array_equal(xb[name][used], xa[name][used]), (wl, name)
        # the Forward side is untouched by what is stored
        assert np.array_equal(xb["fwd_bits"].view(np.uint32), xa["fwd_bits"].view(np.uint32)), wl
        assert np.array_equal(xb["envsc"][used].view(np.uint32), xa["envsc"][used].view(np.uint32)), wl
        assert np.all(np.abs(xb["domcorr"] - xa["domcorr"])[used] <= 1e-3), (wl, float(np.abs(xb["domcorr"] - xa["domcorr"])[used].max()))
        e.close()


def test_multihit_backward_on_a_node_window_gives_the_full_width_regions(tmp_path):
    """The multihit Backward sweep (domain decoding) on a node window: its posteriors are lower bounds with a
    measured slack, and the region scan keeps a window's regions only when every threshold decision is beyond that
    slack - so regions, multidomain flags, envelopes and everything after them must be IDENTICAL to the full-width
    sweep's (WH_NO_P2WIN), pair by pair: headline fragments, ragged and unrelated queries, two-copy queries (real
    multidomain regions), on models of 8-24 cells per lane.  The counters prove which path ran."""
    _need_gpu()
    import bench
    from witch_amd import synth
    from witch_amd.ehmm import EHMM, pack_queries
    rng = np.random.default_rng(11)
    for wl, nq, nh in (("dna_100k_x200", 1536, 24), ("dna_m700", 256, 6), ("dna_m1250", 192, 6), ("dna_m1450", 128, 4)):
        fam, se, names, seqs, k = bench.make_workload(wl, str(tmp_path / wl), nq, nh)
        e = EHMM(se.paths, hmm_index=se.index, nseq=se.nseq)
        base = [s_.astype(np.uint8) for s_ in seqs]
        ragged = [s_[: int(rng.integers(12, len(s_) + 1))] for s_ in base[:200]]
        junk = [rng.integers(0, 4, size=int(n)).astype(np.uint8) for n in rng.integers(5, 150, size=60)]
        twice = [np.concatenate([s_[:70], junk[i % len(junk)][:20], s_[:70]]).astype(np.uint8) for i, s_ in enumerate(base[:60])]
        res, offs = pack_queries(base + ragged + junk + twice)
        d_w, f_w, det_w = e.score(res, offs, want_detail=True)
        p_w = e.last_score_paths()
        e.set_option("WH_NO_P2WIN", "1")
        d_f, f_f, det_f = e.score(res, offs, want_detail=True)
        p_f = e.last_score_paths()
        e.set_option("WH_NO_P2WIN", "")
        assert p_f["p2_window"] == 0 and p_f["p2_window_in_doubt"] == 0, p_f
        if int(e.M.max()) <= 1024:          # (20- and 24-cell models keep twelve waves instead of the window's three extra rows in LDS)
            assert p_w["p2_window"] > 0.4 * (len(offs) - 1) * e.H, (wl, p_w)      # the window is the common path on family fragments
        assert np.array_equal(f_w, f_f), wl
        assert np.array_equal(d_w, d_f), wl
        for a_, b_ in zip(det_w, det_f):
            assert a_.nregions == b_.nregions and a_.nenv == b_.nenv
            assert list(a_.env_i[:a_.nenv]) == list(b_.env_i[:b_.nenv]) and list(a_.env_j[:a_.nenv]) == list(b_.env_j[:b_.nenv])
        e.close()


def test_queries_with_more_than_eight_regions_lose_none(orc, tmp_path):
    """HMMER has no limit on the domains of a sequence; the scoring kernels list up to 16 regions per pair (more: the
    long-list pass, next test).  Queries of ten to fourteen copies of a family fragment, random sequence
    between them: every region is found and scored, nothing is flagged, scores and envelopes equal the oracle's - on a
    small model (one-query kernel) and through the pass-synchronous kernel (1 900 nodes)."""
    _need_gpu()
    from witch_amd import synth
    from witch_amd.ehmm import EHMM, pack_queries
    rng = np.random.default_rng(77)
    for root_len in (180, 1900):
        fam = synth.make_family(3100 + root_len, root_len, 16, "dna", 0.03, 1e-4)
        eh = synth.make_ehmm(fam, 2, str(tmp_path / str(root_len)), witch_layout=False)
        e = EHMM(eh.paths, hmm_index=eh.index, nseq=eh.nseq)
        _, frags = synth.make_queries(fam, 5, 14, 60)
        seqs = []
        for copies in (10, 12, 14):
            parts = []
            for c in range(copies):
                parts.append(frags[c % len(frags)].astype(np.uint8))
                parts.append(rng.integers(0, 4, size=int(rng.integers(25, 40))).astype(np.uint8))
            seqs.append(np.concatenate(parts))
        res, offs = pack_queries(seqs)
        deci, flags, det = e.score(res, offs, want_detail=True)
        ohm = [orc.OracleHMM(p) for p in eh.paths]
        od, of, ofwd, osc = orc.score_batch(ohm, res, offs)
        assert (flags & 8).sum() == 0, "an envelope was dropped"
        assert max(d.nregions for d in det) > 8, [d.nregions for d in det]       # the case this test is about
        assert np.array_equal(flags & 3, of & 3)
        _check_decibits(deci, od, osc, (of & 1) == 1, ("many regions", root_len), LONG_EPS)
        for q in range(len(seqs)):
            for h in range(e.H):
                r = ohm[h].score(seqs[q])
                d = det[q * e.H + h]
                assert d.nregions == r.nregions, (root_len, q, h, d.nregions, r.nregions)
        e.close()


def test_pairs_with_more_regions_than_a_kernel_lists_are_scored_in_full(orc, tmp_path):
    """HMMER has no limit on the regions of a sequence (hmmsearch as called at witch_msa/gcmm/algorithm.py:526-532).
    The scoring kernels list WH_MAX_ENVELOPES regions per pair; a pair with more is scored again inside the same call by
    the long-list pass (float64 front end, region list in HBM, its own resolver launch).  Queries of 20 to 56 copies of a
    family fragment - random spacers between them, some copies back to back (multidomain candidates) - on a small model
    (one-query kernel) and on 1 900 nodes (pass-synchronous kernel): nothing is flagged WH_FLAG_TRUNC, every region is
    counted, flags and deci-bits equal the oracle's (whose own list holds 256), the detail record lists the first
    WH_MAX_ENVELOPES envelopes; with WH_NO_LONG_LIST the same pairs come back flagged (what the pass is for), and the
    pairs of an ordinary query in the same batch are bitwise what they are without the long ones."""
    _need_gpu()
    from witch_amd import synth
    from witch_amd.ehmm import EHMM, pack_queries
    rng = np.random.default_rng(4077)
    for root_len in (180, 1900):
        fam = synth.make_family(3100 + root_len, root_len, 16, "dna", 0.03, 1e-4)
        eh = synth.make_ehmm(fam, 2, str(tmp_path / str(root_len)), witch_layout=False)
        e = EHMM(eh.paths, hmm_index=eh.index, nseq=eh.nseq)
        _, frags = synth.make_queries(fam, 5, 14, 60)
        seqs = [frags[0].astype(np.uint8)]                       # an ordinary query
        for copies, touch in ((20, True), (24, False), (34, True), (56, True)):
            parts = []
            for c in range(copies):
                parts.append(frags[c % len(frags)].astype(np.uint8))
                if not (touch and c % 7 == 3):                   # (touch: every seventh copy runs straight into the next)
                    parts.append(rng.integers(0, 4, size=int(rng.integers(25, 40))).astype(np.uint8))
            seqs.append(np.concatenate(parts))
        seqs.append(np.zeros(0, dtype=np.uint8))                 # and an empty one
        res, offs = pack_queries(seqs)
        deci, flags, det = e.score(res, offs, want_detail=True)
        n_long = e.last_long_list_pairs()
        ohm = [orc.OracleHMM(p) for p in eh.paths]
        od, of, ofwd, osc = orc.score_batch(ohm, res, offs)
        assert (flags & 8).sum() == 0, ("an envelope was dropped", root_len, flags)
        nreg = np.array([d.nregions for d in det]).reshape(len(seqs), e.H)
        nreg[[len(s_) == 0 for s_ in seqs], :] = 0                             # (an empty query has no detail record)
        assert nreg.max() > 2 * WH_MAX_ENVELOPES, nreg                         # the case this test is about
        assert n_long == int((nreg > WH_MAX_ENVELOPES).sum()) and n_long >= 3, (n_long, nreg)
        assert np.array_equal(flags & 3, of & 3), (root_len, flags, of)
        _check_decibits(deci, od, osc, (of & 1) == 1, ("long list", root_len), LONG_EPS)
        for q in range(len(seqs)):
            for h in range(e.H):
                if len(seqs[q]) == 0:
                    continue
                r = ohm[h].score(seqs[q])
                d = det[q * e.H + h]
                assert d.nregions == r.nregions, (root_len, q, h, d.nregions, r.nregions)
                assert d.nenv == min(r.nenv, WH_MAX_ENVELOPES), (root_len, q, h, d.nenv, r.nenv)
                if not (r.flags & 2):                                          # (multidomain regions: the stochastic class)
                    assert list(d.env_i[:d.nenv]) == list(r.env_i[:d.nenv]) and list(d.env_j[:d.nenv]) == list(r.env_j[:d.nenv]), (root_len, q, h)
        # without the pass the same pairs are flagged, the others untouched
        e.set_option("WH_NO_LONG_LIST", "1")
        deci0, flags0, _ = e.score(res, offs, want_detail=True)
        e.set_option("WH_NO_LONG_LIST", "")
        assert e.last_long_list_pairs() == 0
        assert np.array_equal((flags0 & 8) != 0, nreg > WH_MAX_ENVELOPES), (flags0, nreg)
        keep = nreg <= WH_MAX_ENVELOPES
        assert np.array_equal(deci0[keep], deci[keep]) and np.array_equal(flags0[keep], flags[keep])
        # the ordinary query alone: bitwise the same result as inside the batch
        r1, o1 = pack_queries(seqs[:1])
        d1, f1, _ = e.score(r1, o1, want_detail=True)
        assert np.array_equal(d1[0], deci[0]) and np.array_equal(f1[0], flags[0])
        e.close()
        if root_len == 180:
            # the same pairs found by the several-waves-per-pair kernels (their own 16-entry list; WH_FORCE_WIDE, read at load)
            old = os.environ.get("WH_FORCE_WIDE")
            os.environ["WH_FORCE_WIDE"] = "4"
            try:
                ew = EHMM(eh.paths, hmm_index=eh.index, nseq=eh.nseq)
                dw, fw, _ = ew.score(res, offs, want_detail=True)
                assert ew.last_long_list_pairs() == n_long
                assert (fw & 8).sum() == 0 and np.array_equal(fw & 3, of & 3)
                _check_decibits(dw, od, osc, (of & 1) == 1, ("long list, several waves per pair", root_len), LONG_EPS)
                ew.close()
            finally:
                if old is None:
                    os.environ.pop("WH_FORCE_WIDE", None)
                else:
                    os.environ["WH_FORCE_WIDE"] = old


def test_one_region_with_up_to_28_domains(orc, tmp_path):
    """Tandem repeats: 6 to 28 copies of a family fragment back to back are ONE region that HMMER's stochastic resolver
    splits into as many envelopes.  The resolver keeps up to 8 192 sampled segments per region (200 traces x
    32 domains fit), clusters them with its vertex stacks in LDS up to 2 048 segments and in HBM beyond (12 copies and
    more), and lists up to 64 significant clusters: nothing is flagged WH_FLAG_TRUNC, the envelope count, the flags and the
    deci-bit scores equal the oracle's - DNA on a small model, protein on a 12-cell model."""
    _need_gpu()
    from witch_amd import synth
    from witch_amd.ehmm import EHMM, pack_queries
    for alph, root_len, flen in (("dna", 180, 60), ("amino", 700, 45)):
        fam = synth.make_family(5200 + root_len, root_len, 16, alph, 0.03, 1e-4)
        eh = synth.make_ehmm(fam, 2, str(tmp_path / alph), witch_layout=False)
        e = EHMM(eh.paths, hmm_index=eh.index, nseq=eh.nseq)
        _, frags = synth.make_queries(fam, 5, 14, flen)
        seqs = [np.concatenate([frags[c % len(frags)].astype(np.uint8) for c in range(copies)]) for copies in (6, 12, 20, 28)]
        res, offs = pack_queries(seqs)
        deci, flags, det = e.score(res, offs, want_detail=True)
        ohm = [orc.OracleHMM(p) for p in eh.paths]
        od, of, ofwd, osc = orc.score_batch(ohm, res, offs)
        assert (flags & 8).sum() == 0, ("WH_FLAG_TRUNC", alph, flags)
        assert np.array_equal(flags & 3, of & 3), (alph, flags, of)
        _check_decibits(deci, od, osc, (of & 1) == 1, ("tandem repeats", alph), LONG_EPS)
        most = 0
        for q in range(len(seqs)):
            for h in range(e.H):
                r = ohm[h].score(seqs[q])
                d = det[q * e.H + h]
                most = max(most, r.nenv)
                assert d.nregions == r.nregions and d.nenv == min(r.nenv, WH_MAX_ENVELOPES), (alph, q, h, d.nregions, r.nregions, d.nenv, r.nenv)
        assert most > WH_MAX_ENVELOPES, most                                   # the case this test is about
        e.close()


def test_two_queries_per_wave_kernel_equals_the_one_query_kernel(tmp_path):
    """wh_score9.hip (two queries of one model per wavefront, option WH_SCORE_KERNEL=9) does per query what the
    one-query sweeps do, operation by operation: scores, flags and Forward log-odds are identical BITWISE - on
    equal-length queries, on queries of different lengths sharing a wave (odd counts included), and on a query set
    with empty, multidomain and unrelated queries."""
    _need_gpu()
    import bench
    from witch_amd import synth
    from witch_amd.ehmm import EHMM, pack_queries
    fam, se, names, seqs, k = bench.make_workload("dna_100k_x200", str(tmp_path), 1025, 12)
    e = EHMM(se.paths, hmm_index=se.index, nseq=se.nseq)
    e.set_option("WH_SPILL_BAND", "0")       # (the two-query Forward sweep has no lane-block band: compare like with like)
    rng = np.random.default_rng(5)
    ragged = [s_.astype(np.uint8)[: int(rng.integers(20, 151))] for s_ in seqs[:301]]
    junk = [rng.integers(0, 4, size=int(n)).astype(np.uint8) for n in rng.integers(1, 150, size=40)]
    twice = [np.concatenate([s_[:70], s_[:70]]).astype(np.uint8) for s_ in seqs[:40]]       # two copies: multidomain candidates
    for batch in ([s_.astype(np.uint8) for s_ in seqs], ragged, ragged[:7] + [np.zeros(0, dtype=np.uint8)] + junk + twice):
        res, offs = pack_queries(batch)
        d7, f7, w7 = e.score(res, offs, want_fwd=True)
        p7 = e.last_score_paths()
        e.set_option("WH_SCORE_KERNEL", "9")
        d9, f9, w9 = e.score(res, offs, want_fwd=True)
        p9 = e.last_score_paths()
        e.set_option("WH_SCORE_KERNEL", "")
        assert np.array_equal(f7, f9)
        assert np.array_equal(d7, d9)
        assert np.array_equal(w7.view(np.uint32), w9.view(np.uint32))
        env = ("window256", "window512", "window_rejected", "full_width")       # (the pair kernel has no window for the multihit sweep)
        assert [p7[t] for t in env] == [p9[t] for t in env], (p7, p9)
    e.close()


@pytest.mark.gpu
def test_staged_launches_equal_the_fused_kernel(tmp_path):
    """wh_staged.hip (round 5; WH_SCORE_KERNEL=10: P1 | P2 on a window + certified scan | P2 at full width | envelopes as
    launches of their own over batches of pairs; 11: P3 | P4 window | P4 full | dense redo | assembly split as well, one
    Forward slab per envelope) calls the fused kernel's own sweep functions on the same inputs: deci-bits, flags, Forward
    log-odds and EVERY field of the per-pair detail record are identical bitwise, the path counters of the envelope sweeps
    too - on 1 024 x 200 headline pairs, on ragged / empty / unrelated / two-copy queries, with the resolver and without
    it (multidomain regions as one envelope), with a batch size that forces several batches, and with too few envelope
    units (the pass is repeated with the fused kernel and says so).  The per-pair path bytes (wh_set_path_buffer) agree
    with the counters."""
    _need_gpu()
    import torch
    import bench
    from witch_amd.ehmm import EHMM, pack_queries
    fam, se, names, seqs, k = bench.make_workload("dna_100k_x200", str(tmp_path), 1024, None)
    e = EHMM(se.paths, hmm_index=se.index, nseq=se.nseq)
    rng = np.random.default_rng(7)
    ragged = [s_.astype(np.uint8)[: int(rng.integers(20, 151))] for s_ in seqs[:301]]
    junk = [rng.integers(0, 4, size=int(n)).astype(np.uint8) for n in rng.integers(1, 150, size=40)]
    twice = [np.concatenate([s_[:70], s_[:70]]).astype(np.uint8) for s_ in seqs[:60]]
    mixed = ragged[:7] + [np.zeros(0, dtype=np.uint8)] + junk + twice

    def run(batch, kernel, **opts):
        res, offs = pack_queries(batch)
        e.set_option("WH_SCORE_KERNEL", kernel)
        for k_, v_ in opts.items():
            e.set_option(k_, v_)
        try:
            d, f, w, det = e.score(res, offs, want_fwd=True, want_detail=True)
            paths, reruns = e.last_score_paths(), e.last_queue_reruns()
        finally:
            e.set_option("WH_SCORE_KERNEL", "")
            for k_ in opts:
                e.set_option(k_, "")
        return d, f, w, np.ctypeslib.as_array(det).copy(), paths, reruns

    def same(a, b, what):
        assert np.array_equal(a[1], b[1]), what
        assert np.array_equal(a[0], b[0]), what
        assert np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32)), what
        for name in a[3].dtype.names:
            x, y = a[3][name], b[3][name]
            assert np.array_equal(x.view(np.int32) if x.dtype.kind == "f" else x, y.view(np.int32) if y.dtype.kind == "f" else y), (what, name)
        env = ("window256", "window512", "window_rejected", "full_width")
        assert [a[4][t] for t in env] == [b[4][t] for t in env], (what, a[4], b[4])

    full = [s_.astype(np.uint8) for s_ in seqs]
    # (queries of 300-900 nt: too long for the staged kernels' LDS plans at this model size - the class is then left to the
    # fused kernel without an error - or served by them where they fit; the same results either way)
    longq = [np.concatenate([s_] * int(rng.integers(2, 7))).astype(np.uint8) for s_ in seqs[:48]]
    for batch, tag in ((full, "headline"), (ragged, "ragged"), (mixed, "mixed"), (longq, "long")):
        ref = run(batch, "7")
        for kern in ("10", "11"):
            got = run(batch, kern)
            same(ref, got, (tag, kern))
            assert got[5] == 0
        if tag == "mixed":
            assert int(((ref[1] & 2) != 0).sum()) > 0                          # the resolver's class is present
            same(run(batch, "7", WH_NO_RESOLVE="1"), run(batch, "10", WH_NO_RESOLVE="1"), (tag, "no resolver"))
            same(run(batch, "7", WH_NO_WINDOW="1"), run(batch, "11", WH_NO_WINDOW="1"), (tag, "no window"))
    # WH_SCORE_KERNEL=12: four envelopes per Backward sweep (sweep_backward_null2_quad: one envelope per quarter of the wave,
    # 16 cells per lane).  The per-cell arithmetic is the window sweep's, the sums over a row are formed in another order:
    # flags, regions, envelopes, Forward log-odds and envelope scores identical, the null2 correction equal to float32
    # rounding (within the 1e-3 nats every sweep is held to against the oracle), deci-bits under the rounding-boundary rule (on the kernel's own float scores).
    for batch, tag in ((full, "headline"), (ragged, "ragged"), (mixed, "mixed")):
        ref, got = run(batch, "7"), run(batch, "12")
        assert np.array_equal(ref[1], got[1]) and np.array_equal(ref[2].view(np.uint32), got[2].view(np.uint32)), tag
        for name in ("fwd_bits", "nregions", "nenv", "env_i", "env_j", "envsc"):
            x, y = ref[3][name], got[3][name]
            assert np.array_equal(x.view(np.int32) if x.dtype.kind == "f" else x, y.view(np.int32) if y.dtype.kind == "f" else y), (tag, name)
        assert np.max(np.abs(ref[3]["domcorr"] - got[3]["domcorr"])) <= 1e-3, tag                  # (the oracle comparison allows the same)
        dd = np.nonzero(ref[0] != got[0])
        assert len(dd[0]) <= max(2, ref[0].size // 100000), (tag, len(dd[0]))
        for q_, h_ in zip(*dd):
            sc = float(ref[3]["seq_score"][q_ * e.H + h_])
            assert abs(int(ref[0][q_, h_]) - int(got[0][q_, h_])) == 1 and _near_boundary_eps(sc, BOUNDARY_EPS), (tag, int(q_), int(h_), sc)
        if tag == "headline":
            assert got[4]["window256"] > 0.8 * ref[4]["window256"]             # ... and the quarter-wave sweep did serve them
    # several batches (units for ~1/6 of the pairs at a time), and too few units for even one work item's envelopes
    ref = run(full, "7")
    got = run(full, "11", WH_ST_UNITS="40000")
    same(ref, got, "several batches")
    got = run(mixed, "11", WH_ST_UNITS="16")
    same(run(mixed, "7"), got, "unit overflow")
    assert got[5] >= 1                                                         # ... repeated with the fused kernel
    # per-pair path bytes: every reported pair of the headline batch went through one kind of P2 and its envelopes through P4
    res, offs = pack_queries(full)
    paths_t = torch.zeros((len(full), e.H), dtype=torch.uint8, device="cuda")
    e.set_path_buffer(paths_t)
    e.set_option("WH_SCORE_KERNEL", "10")
    d, f = e.score(res, offs)
    cnt = e.last_score_paths()
    e.set_option("WH_SCORE_KERNEL", "")
    e.set_path_buffer(None)
    pb = paths_t.cpu().numpy()
    rep = (f & 1) != 0
    assert np.array_equal(d, ref[0]) and np.array_equal(f, ref[1])
    assert np.all(((pb[rep] & 1) != 0) ^ ((pb[rep] & 2) != 0))                 # P2: window kept XOR full width
    assert int(((pb & 1) != 0).sum()) == cnt["p2_window"]
    e.close()


def test_null2_by_trace_from_prefix_sums_equals_the_row_sums():
    """Round 4: the resolver forms the null2 vector of a sampled domain from float64 prefix sums of the emission odds over
    the nodes (a dozen row differences per domain) instead of adding one table row per residue in float32
    (WH_RES_NULL2_GATHER, environment, read per call: the path it replaced).  Same terms, different rounding of the sum:
    flags identical, every single-domain pair identical, and a multidomain pair at most one deci-bit apart - rarely
    (46 of 255 725 on a slice of config 5; here on the golden protein case with 422 multidomain pairs)."""
    _need_gpu()
    from tests.conftest import load_case
    from witch_amd.ehmm import EHMM, pack_queries
    case = load_case("amino_multidomain")
    e = EHMM(case.hmm_paths, hmm_index=case.hmm_index, nseq=case.nseq)
    res, offs = pack_queries([e.digitize(s_) for s_ in case.qseqs])
    deci, flags = e.score(res, offs)
    os.environ["WH_RES_NULL2_GATHER"] = "1"
    try:
        deci2, flags2 = e.score(res, offs)
    finally:
        os.environ.pop("WH_RES_NULL2_GATHER", None)
    e.close()
    assert np.array_equal(flags & 7, flags2 & 7)
    multi = (flags & 2) != 0
    assert int(multi.sum()) > 300
    assert np.array_equal(deci[~multi], deci2[~multi])
    d = np.abs(deci.astype(np.int64) - deci2)
    assert d.max() <= 1 and int((d != 0).sum()) <= 4, (int(d.max()), int((d != 0).sum()))


def test_resolver_queue_overflow_repeats_the_scoring_pass(golden_case):
    """The queue of pairs with a multidomain region is sized by estimate; a call that needs more slots than it got
    counts them, grows the queue and scores again.  Forced here with a queue of 3 slots: same results as the
    default sizing, and the re-run is reported."""
    _need_gpu()
    case = golden_case
    e, seqs, res, offs = _load(case)
    d0, f0 = e.score(res, offs)
    n_multi = int(((f0 & 2) != 0).sum())
    assert e.last_queue_reruns() == 0
    e.set_option("WH_RQUEUE_CAP", "3")
    d1, f1 = e.score(res, offs)
    reruns = e.last_queue_reruns()
    e.set_option("WH_RQUEUE_CAP", "")
    assert np.array_equal(d0, d1) and np.array_equal(f0, f1), case.name
    assert reruns == (1 if n_multi > 3 else 0), (case.name, n_multi, reruns)
    e.close()


@pytest.mark.parametrize("root_len", [900, 1100, 1400, 1800])
def test_large_protein_models(root_len, orc, tmp_path):
    """Protein models of 16 / 20 / 24 / 32 cells per lane: 20 emission rows no longer fit in LDS
    beside both table orientations from 20 cells on, so those go to the pass-synchronous kernels;
    at 32 cells the emission rows stay in L2 (short and long queries, scoring and alignment)."""
    _need_gpu()
    from witch_amd import synth
    from witch_amd.ehmm import EHMM, pack_queries
    fam = synth.make_family(555 + root_len, root_len, 8, "amino", 0.03, 1e-4)
    eh = synth.make_ehmm(fam, 2, str(tmp_path), witch_layout=False)
    e = EHMM(eh.paths, hmm_index=eh.index, nseq=eh.nseq)
    assert root_len - 50 < int(e.M.max()) <= 2048
    ohm = [orc.OracleHMM(p) for p in eh.paths]
    for qlen in (150, 900):
        names, seqs = synth.make_queries(fam, 3 + qlen, 4, qlen)
        seqs = [s.astype(np.uint8) for s in seqs]
        res, offs = pack_queries(seqs)
        deci, flags, fwd = e.score(res, offs, want_fwd=True)
        od, of, ofwd, osc = orc.score_batch(ohm, res, offs)
        assert np.max(np.abs(fwd - ofwd)) <= 2e-4
        assert np.array_equal(flags & 3, of & 3)
        _check_decibits(deci, od, osc, (of & 1) == 1, ("large protein", root_len, qlen), BOUNDARY_EPS if qlen <= 330 else LONG_EPS)
        pq = [q for q in range(len(seqs)) for _ in range(e.H)]
        ph = [h for q in range(len(seqs)) for h in range(e.H)]
        cols, co = e.align(res, offs, pq, ph)
        for p in range(len(pq)):
            assert np.array_equal(cols[co[p]:co[p + 1]], ohm[ph[p]].align(seqs[pq[p]])), (qlen, pq[p], ph[p])
    e.close()


def test_headline_size_properties(orc, tmp_path):
    """BASELINE.json's headline configuration at full size (100 000 queries x 200 HMMs): properties
    that do not need the oracle at that size - determinism of the scoring kernel, structure of the
    top-k table and of the aligned columns - plus an oracle spot check on a random sample."""
    _need_gpu()
    import torch
    import bench
    from witch_amd.ehmm import EHMM, pack_queries
    fam, se, names, seqs, k = bench.make_workload("dna_100k_x200", str(tmp_path), None, None)
    e = EHMM(se.paths, hmm_index=se.index, nseq=se.nseq)
    res, offs = pack_queries([s_.astype(np.uint8) for s_ in seqs])
    res_t, off_t = torch.from_numpy(res).cuda(), torch.from_numpy(offs).cuda()
    maxlen = int(np.max(np.diff(offs)))
    d1, f1 = e.score_t(res_t, off_t, maxlen)
    d2, f2 = e.score_t(res_t, off_t, maxlen)
    assert torch.equal(d1, d2) and torch.equal(f1, f2)                    # idempotent / deterministic
    deci, flags = d1.cpu().numpy(), f1.cpu().numpy()
    assert deci.shape == (100000, 200)
    rep = (flags & 1) == 1
    assert (deci[~rep] == 0).all() and rep.mean() > 0.99
    idx, w, nk, nu = [t.cpu().numpy() for t in e.topk_t(d1, f1, k)]
    assert ((nu >= 1) & (nu <= nk) & (nk <= k)).all()
    assert (np.diff(w, axis=1) <= 1e-15).all() and (w >= 0).all() and (w.sum(1) <= 1 + 1e-9).all()
    cum = np.cumsum(w, axis=1)
    reached = cum[np.arange(len(nu)), nu - 1] >= 0.999
    assert (reached | (nu == nk)).all()                                   # 0.999 prefix rule (aligner.py:58-63)
    first_short = (nu > 1) & (cum[np.arange(len(nu)), np.maximum(nu - 2, 0)] >= 0.999)
    assert not first_short.any()                                          # and not one model more than needed
    valid = idx[:, 0] >= 0
    assert valid.all()
    srt = np.sort(idx, axis=1)
    assert ((np.diff(srt, axis=1) != 0) | (srt[:, 1:] < 0)).all()         # no model twice per query
    # align the first 20 000 queries' kept models: columns strictly increasing inside [0, M)
    nq_a = 20000
    ar = np.arange(k)[None, :]
    keep = ar < nu[:nq_a, None]
    pq = np.nonzero(keep)[0]
    ph = np.array([e.pos_of_index[int(x)] for x in idx[:nq_a][keep]], dtype=np.int32)
    cols, co = e.align(res, offs, pq, ph)
    M = e.M
    lens = np.diff(co)
    pair_of = np.repeat(np.arange(len(pq)), lens)
    ok = cols >= 0
    assert (cols[ok] < M[ph][pair_of[ok]]).all()
    for p in np.random.default_rng(0).choice(len(pq), size=2000, replace=False):     # monotone columns, sampled
        c = cols[co[p]:co[p + 1]]
        c = c[c >= 0]
        assert (np.diff(c) > 0).all()
    assert (flags & 8).sum() == 0                                         # no pair lost an envelope (WH_FLAG_TRUNC)
    # ---- oracle evidence at this size, STRATIFIED BY CODE PATH.  The staged launches (WH_SCORE_KERNEL=11) run the same
    # sweep functions and record per pair which path it took; their results are asserted identical to the default
    # kernel's at full size (all 2e7 pairs, bitwise), so the strata describe the numbers checked above.  From every class
    # a sample goes through the float64 oracle: reported / multidomain flags identical, Forward log-odds within 1e-4 bit,
    # deci-bits under the rounding-boundary rule of SURVEY 8.0.
    paths_t = torch.zeros((100000, e.H), dtype=torch.uint8, device="cuda")
    e.set_path_buffer(paths_t)
    e.set_option("WH_SCORE_KERNEL", "11")
    d3, f3, w3 = e.score_t(res_t, off_t, maxlen, want_fwd=True)
    e.set_option("WH_SCORE_KERNEL", "")
    e.set_path_buffer(None)
    assert e.last_queue_reruns() == 0
    assert torch.equal(d3, d1) and torch.equal(f3, f1)
    pb, fwd = paths_t.cpu().numpy(), w3.cpu().numpy()
    strata = {
        "p2 window kept, p4 on 256 nodes": ((pb & 1) != 0) & ((pb & 4) != 0) & ((pb & (8 | 16 | 32 | 64 | 128)) == 0),
        "p2 window in doubt -> full width": (pb & 2) != 0,
        "p4 on 512 nodes": (pb & 8) != 0,
        "p4 window rejected -> full width": (pb & 16) != 0,
        "p4 full width from the start": ((pb & 32) != 0) & ((pb & 16) == 0),
        "dense redo": (pb & 64) != 0,
        "multidomain (resolver)": (pb & 128) != 0,
        "not reported": ~rep,
    }
    want = {"p2 window kept, p4 on 256 nodes": 7000, "p2 window in doubt -> full width": 4000, "p4 on 512 nodes": 3000,
            "p4 window rejected -> full width": 2500, "p4 full width from the start": 3000, "dense redo": 500,
            "multidomain (resolver)": 1000, "not reported": 500}
    rng = np.random.default_rng(1)
    pq, ph, tags = [], [], []
    for name, mask in strata.items():
        where = np.argwhere(mask)
        if name not in ("dense redo", "not reported"):
            assert len(where) > 100, (name, len(where))                    # the class exists at this size
        take = where[rng.choice(len(where), size=min(want[name], len(where)), replace=False)] if len(where) else where
        pq += [int(x) for x in take[:, 0]]
        ph += [int(x) for x in take[:, 1]]
        tags += [name] * len(take)
    assert len(pq) >= 20000, len(pq)
    ohm = [None] * e.H
    for h in set(ph):
        ohm[h] = orc.OracleHMM(se.paths[h])
    od, of, ofwd, osc = orc.score_pairs(ohm, res, offs, pq, ph)
    pq, ph = np.array(pq), np.array(ph)
    gd, gf, gw = deci[pq, ph], flags[pq, ph], fwd[pq, ph]
    bad = np.nonzero((gf & 3) != (of & 3))[0]
    assert len(bad) == 0, [(tags[i], int(pq[i]), int(ph[i]), int(gf[i]), int(of[i])) for i in bad[:5]]
    fin = np.isfinite(ofwd)
    assert np.all(np.abs(gw[fin] - ofwd[fin]) <= 1e-4), float(np.max(np.abs(gw[fin] - ofwd[fin])))
    n_off = {}
    for i in np.nonzero(gd != od)[0]:
        eps = 0.02 if of[i] & 2 else BOUNDARY_EPS
        n_off[tags[i]] = n_off.get(tags[i], 0) + _check_one_decibit(gd[i], od[i], osc[i], ("headline", tags[i], int(pq[i]), int(ph[i])), eps)
    print("headline oracle sample: %d pairs in %d strata; one deci-bit off at a rounding boundary: %s" % (len(pq), len(strata), n_off))
    e.close()


def test_survey_family_sketch_every_size_class_against_the_oracle(orc, tmp_path):
    """SURVEY 8(d)'s own sketch of config 3 (`dna_100k_x200_m1000`: root 1 000 nt, 0.2 % indels per branch - models of
    996-2 996 nodes in FIVE cells-per-lane classes: 16, 20, 24 on the one-wave kernels, 32 and 48 on the pass-synchronous
    kernel) at 2 000 queries: a sample of at least 400 pairs from EVERY class through the float64 oracle - flags,
    Forward log-odds within 1e-4 bit, deci-bits under the rounding-boundary rule."""
    _need_gpu()
    import bench
    from witch_amd.ehmm import EHMM, pack_queries
    fam, se, names, seqs, k = bench.make_workload("dna_100k_x200_m1000", str(tmp_path), 2000, None)
    seqs = [s_.astype(np.uint8) for s_ in seqs]
    e = EHMM(se.paths, hmm_index=se.index, nseq=se.nseq)
    res, offs = pack_queries(seqs)
    deci, flags, fwd = e.score(res, offs, want_fwd=True)
    assert (flags & 8).sum() == 0
    cls = np.maximum(4, (-(-e.M // 64) + 3) // 4 * 4)                      # cells per lane of every model (wh_hmm.cpp choose_Q)
    classes = sorted(set(int(c) for c in cls))
    assert set(classes) >= {16, 20, 24} and max(classes) >= 32, classes
    rng = np.random.default_rng(3)
    pq, ph, tags = [], [], []
    for c in classes:
        models = np.nonzero(cls == c)[0]
        n = max(400, 2000 // len(classes))
        pq += [int(x) for x in rng.integers(0, len(seqs), size=n)]
        ph += [int(x) for x in rng.choice(models, size=n)]
        tags += [c] * n
    ohm = [None] * e.H
    for h in set(ph):
        ohm[h] = orc.OracleHMM(se.paths[h])
    od, of, ofwd, osc = orc.score_pairs(ohm, res, offs, pq, ph)
    pq, ph = np.array(pq), np.array(ph)
    gd, gf, gw = deci[pq, ph], flags[pq, ph], fwd[pq, ph]
    bad = np.nonzero((gf & 3) != (of & 3))[0]
    assert len(bad) == 0, [(tags[i], int(pq[i]), int(ph[i]), int(gf[i]), int(of[i])) for i in bad[:5]]
    fin = np.isfinite(ofwd)
    assert np.all(np.abs(gw[fin] - ofwd[fin]) <= 1e-4), float(np.max(np.abs(gw[fin] - ofwd[fin])))
    n_off = {}
    for i in np.nonzero(gd != od)[0]:
        eps = 0.02 if of[i] & 2 else BOUNDARY_EPS
        n_off[tags[i]] = n_off.get(tags[i], 0) + _check_one_decibit(gd[i], od[i], osc[i], ("m1000", tags[i], int(pq[i]), int(ph[i])), eps)
    print("[dna_100k_x200_m1000] %d pairs over the classes %s; one deci-bit off at a rounding boundary per class: %s; multidomain pairs in the sample: %d"
          % (len(pq), classes, n_off, int(((of & 2) != 0).sum())))
    e.close()


def _oracle_topk_and_pairs(orc, hmm_index, nseq, od, of, k):
    """rank -> calculateWeights -> 0.999 prefix with the numpy restatement (oracle side)."""
    size_of = dict(zip(hmm_index, nseq))
    tables, pairs = [], []
    for qi in range(od.shape[0]):
        ranked = orc.rank_bitscores(hmm_index, od[qi], of[qi] & 1)
        if not ranked:
            tables.append(([], 0))
            continue
        idxs = [r[0] for r in ranked]
        w = orc.calculate_weights(idxs, [r[1] for r in ranked], [size_of[i] for i in idxs], k)
        nu = orc.adaptive_cut(w)
        tables.append((w, nu))
        pairs += [(qi, i) for i, _ in w[:nu]]
    return tables, pairs


def test_config2_dna_1k_x10_at_its_stated_size(orc, tmp_path):
    """BASELINE.json configs[1] in full: 1 000 synthetic 150-nt queries x 10-HMM ensemble, k = 4 - flags,
    deci-bits (rounding-boundary rule), top-k tables and every aligned column against the oracle."""
    _need_gpu()
    import bench
    from witch_amd.ehmm import EHMM, pack_queries
    fam, se, names, seqs, k = bench.make_workload("dna_1k_x10", str(tmp_path))
    assert len(seqs) == 1000 and len(se.paths) == 10 and k == 4
    seqs = [s_.astype(np.uint8) for s_ in seqs]
    e = EHMM(se.paths, hmm_index=se.index, nseq=se.nseq)
    res, offs = pack_queries(seqs)
    deci, flags, fwd = e.score(res, offs, want_fwd=True)
    ohm = [orc.OracleHMM(p) for p in se.paths]
    od, of, ofwd, osc = orc.score_batch(ohm, res, offs, nthreads=16)
    assert np.max(np.abs(fwd - ofwd)) <= 1e-4
    assert np.array_equal(flags & 7, of & 7)
    assert (flags & 8).sum() == 0                                         # WH_FLAG_TRUNC: no envelope dropped
    n_off = _check_decibits(deci, od, osc, (of & 1) == 1, "dna_1k_x10")
    idx, w, nk, nu = e.topk(deci, flags, k)
    tables, _ = _oracle_topk_and_pairs(orc, se.index, se.nseq, deci, flags, k)     # same scores in: tables must be identical
    for qi, (ow, onu) in enumerate(tables):
        assert nk[qi] == len(ow) and nu[qi] == onu, qi
        assert idx[qi, :nk[qi]].tolist() == [i for i, _ in ow], qi
        assert np.allclose(w[qi, :nk[qi]], [x for _, x in ow], rtol=1e-12, atol=0), qi
    pq = [q for q in range(len(seqs)) for _ in range(int(nu[q]))]
    ph = [e.pos_of_index[int(idx[q, j])] for q in range(len(seqs)) for j in range(int(nu[q]))]
    cols, co = e.align(res, offs, pq, ph)
    ocols, oco = orc.align_batch(ohm, res, offs, pq, ph, nthreads=16)
    assert np.array_equal(co, oco) and np.array_equal(cols, ocols), int((cols != ocols).sum())
    print("\n[dna_1k_x10] %d pairs scored, %d one deci-bit off at a rounding boundary, %d pairs aligned identically"
          % (deci.size, n_off, len(pq)))
    e.close()


@pytest.fixture(scope="module")
def config5_case(tmp_path_factory):
    """The 500-model protein eHMM of BASELINE configs[4] with its first 2 000 queries, loaded once for both blocks below
    (writing 500 model files and parsing them twice - GPU handle and oracle - takes over a minute)."""
    _need_gpu()
    import bench
    from oracle import oracle as orc_
    wd = tmp_path_factory.mktemp("config5")
    fam, se, names, seqs, k = bench.make_workload("aa_50k_x500", str(wd), 2000, None)
    assert len(se.paths) == 500 and k == 10
    ohm = [orc_.OracleHMM(p_) for p_ in se.paths]
    # (the GPU handle is NOT shared: its workspace for 2 000-residue protein queries - envelope slabs and the resolver's float64
    # matrices of every resident wave - is ~100 GB, and a handle that lives to the end of the module left the two-rank
    # rehearsal below with 300 GB of demands on a 288 GB device: its ranks then hung inside the driver, unkillable)
    yield se, [s_.astype(np.uint8) for s_ in seqs], k, ohm


_CONFIG5_ORACLE_S = {}     # block -> seconds the float64 oracle took to score it on this box
CONFIG5_SLOW_BOX_S = float(os.environ.get("WH_TEST_CONFIG5_SLOW_S", "240"))   # seconds; a block 0 slower than this (the boxes of the pool differ by more than 2 x in host speed:
                           # 150-160 s on most, > 280 s observed) and blocks 1 / 2 are skipped WITH that reason, so that
                           # the suite stays inside its time on any box; block 0 always runs in full


@pytest.mark.parametrize("block", [0, 1, 2])
def test_config5_shape_all_500_hmms(orc, config5_case, block):
    """BASELINE.json configs[4] shape (aa_50k_x500): ALL 500 protein HMMs (more than 256 candidates per
    query: the multi-slot path of the top-k kernel) x 192 mixed-length queries (50-2000 residues, three blocks) against
    the oracle, then the structural properties of the top-k table and the aligned columns at 2 000 queries
    (a quarter of these pairs hold several hits: each goes through the 200-trace resolver)."""
    _need_gpu()
    import torch
    from witch_amd.ehmm import EHMM, pack_queries
    se, seqs, k, ohm = config5_case
    if block != 0 and _CONFIG5_ORACLE_S.get(0, 0.0) > CONFIG5_SLOW_BOX_S:
        pytest.skip("the oracle took %.0f s for block 0 on this box (> %d s): blocks 1 and 2 of the config-5 slice are left out here"
                    % (_CONFIG5_ORACLE_S[0], CONFIG5_SLOW_BOX_S))
    e = EHMM(se.paths, hmm_index=se.index, nseq=se.nseq)
    # ---- 192 queries x 500 HMMs against the oracle (round 5: 64 until then), in three blocks of 64: the float64 oracle needs
    # 100-160 s per block on the box's cores (by box: blocks of 96 took 200-240 s on one box and more than 420 s on another),
    # and a test that prints nothing for seven minutes is taken for hung
    NSUB = 64
    sub = seqs[block * NSUB:(block + 1) * NSUB]
    assert min(len(s_) for s_ in sub) < 400 and max(len(s_) for s_ in sub) > 1500
    res, offs = pack_queries(sub)
    deci, flags, fwd = e.score(res, offs, want_fwd=True)
    import time
    t_or = time.time()
    od, of, ofwd, osc = orc.score_batch(ohm, res, offs, nthreads=os.cpu_count() or 16)
    _CONFIG5_ORACLE_S[block] = time.time() - t_or
    fin = np.isfinite(ofwd)
    assert np.max(np.abs(fwd[fin] - ofwd[fin]) / np.maximum(1.0, np.abs(ofwd[fin]) / 1000)) <= 2e-4
    assert np.array_equal(flags & 3, of & 3)
    assert (flags & 8).sum() == 0                                         # WH_FLAG_TRUNC: no envelope dropped
    n_off = _check_decibits(deci, od, osc, (of & 1) == 1, "aa_50k_x500", LONG_EPS)
    idx, w, nk, nu = e.topk(deci, flags, k)
    tables, _ = _oracle_topk_and_pairs(orc, se.index, se.nseq, deci, flags, k)
    for qi, (ow, onu) in enumerate(tables):
        assert nk[qi] == len(ow) and nu[qi] == onu, qi
        got_i, ref_i = idx[qi, :nk[qi]].tolist(), [i for i, _ in ow]
        assert np.allclose(w[qi, :nk[qi]], [x for _, x in ow], rtol=1e-12, atol=0), qi
        for a, b, wa, wb in zip(got_i, ref_i, w[qi], [x for _, x in ow]):     # order identical up to 1e-12 weight ties
            assert a == b or abs(wa - wb) <= 1e-12 * max(wa, wb), (qi, got_i, ref_i)
    pq = [q for q in range(len(sub)) for _ in range(int(nu[q]))]
    ph = [e.pos_of_index[int(idx[q, j])] for q in range(len(sub)) for j in range(int(nu[q]))]
    cols, co = e.align(res, offs, pq, ph)
    ocols, oco = orc.align_batch(ohm, res, offs, pq, ph, nthreads=os.cpu_count() or 16)
    assert np.array_equal(cols, ocols), int((cols != ocols).sum())
    print("\n[aa_50k_x500] block %d, %d x 500 pairs (oracle %.0f s):" % (block, NSUB, _CONFIG5_ORACLE_S[block]), end=" ")
    print(" %d single-domain pairs one deci-bit off (boundary), %d multidomain pairs, %d pairs aligned identically"
          % (n_off, int(((of & 2) != 0).sum()), len(pq)))
    if block != 0:
        e.close()
        return
    # ---- 2 000 queries x 500 HMMs: size-independent properties
    res, offs = pack_queries(seqs)
    res_t, off_t = torch.from_numpy(res).cuda(), torch.from_numpy(offs).cuda()
    maxlen = int(np.max(np.diff(offs)))
    d1, f1 = e.score_t(res_t, off_t, maxlen)
    d2, f2 = e.score_t(res_t, off_t, maxlen)
    assert torch.equal(d1, d2) and torch.equal(f1, f2)
    assert torch.equal(d1[:NSUB].cpu(), torch.from_numpy(deci)) and torch.equal(f1[:NSUB].cpu(), torch.from_numpy(flags))   # batch-size independent (block 0)
    idx, w, nk, nu = [t.cpu().numpy() for t in e.topk_t(d1, f1, k)]
    fl = f1.cpu().numpy()
    assert (fl & 8).sum() == 0                                            # nor at 2 000 queries
    rep_n = ((fl & 1) == 1).sum(1)
    assert (nk == np.minimum(rep_n, k)).all()
    has = nk > 0
    assert ((nu >= 1) & (nu <= nk))[has].all() and (nu[~has] == 0).all()
    assert (np.diff(w, axis=1) <= 1e-15).all() and (w >= 0).all() and (w.sum(1) <= 1 + 1e-9).all()
    cum = np.cumsum(w, axis=1)
    rows = np.nonzero(has)[0]
    assert ((cum[rows, nu[rows] - 1] >= 0.999) | (nu[rows] == nk[rows])).all()
    srt = np.sort(idx, axis=1)
    assert ((np.diff(srt, axis=1) != 0) | (srt[:, 1:] < 0)).all()
    dd = d1.cpu().numpy()
    pos = np.array([e.pos_of_index.get(int(x), 0) for x in idx[:, 0]])
    best = np.where((fl & 1) == 1, dd, -10**9)
    # the first model has the largest weight n_i 2^{s_i}: no reported model may beat it on both score and size
    top_s = dd[np.arange(len(pos)), pos]
    assert ((best.max(1) - top_s)[has] <= 10 * np.log2(e.nseq.max() / e.nseq.min()) + 1).all()
    nq_a = 1500
    keep = np.arange(k)[None, :] < nu[:nq_a, None]
    pq = np.nonzero(keep)[0]
    ph = np.array([e.pos_of_index[int(x)] for x in idx[:nq_a][keep]], dtype=np.int32)
    cols, co = e.align(res, offs, pq, ph)
    lens = np.diff(co)
    pair_of = np.repeat(np.arange(len(pq)), lens)
    ok = cols >= 0
    assert (cols[ok] < e.M[ph][pair_of[ok]]).all()
    for p in np.random.default_rng(0).choice(len(pq), size=min(1000, len(pq)), replace=False):
        c = cols[co[p]:co[p + 1]]
        assert (np.diff(c[c >= 0]) > 0).all()
    e.close()
    del d1, d2, f1, f2, res_t, off_t
    torch.cuda.empty_cache()


@pytest.mark.parametrize("ranks", [2, 4])
def test_multi_rank_rehearsal_equals_one_rank(tmp_path, ranks):
    """BASELINE.json configs[3] rehearsed on one GPU: bench.py under torch.distributed.run with two and with four ranks
    (WITCH_BENCH_REHEARSAL=1: all on cuda:0, gloo gather) must gather exactly the 1-rank top-k table.  Four is the
    largest rank count a one-GPU box admits beside the test runner and the launcher (at most six processes may hold the
    card: a six-rank attempt was killed by the box's process guard); the eight-way shard arithmetic and the packed
    gather at world 8 run on the CPU (tests/test_distributed_gloo.py)."""
    _need_gpu()
    import json
    import os
    import socket
    import subprocess
    import sys
    from tests.conftest import ROOT
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    common = ["--steps", "1", "--warmup", "0", "--nq", "3001", "--nh", "12", "--full", "--no-cpu-baseline"]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r1 = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + common,
                        capture_output=True, text=True, timeout=900, env=env)
    assert r1.returncode == 0, r1.stderr[-2000:]
    env2 = dict(env, WITCH_BENCH_REHEARSAL="1")
    r2 = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks),
                         "--master-addr", "127.0.0.1", "--master-port", str(port),
                         os.path.join(ROOT, "bench.py"), "--gpus", str(ranks)] + common,
                        capture_output=True, text=True, timeout=900, env=env2)
    assert r2.returncode == 0, r2.stderr[-2000:]
    j1 = json.loads([l for l in r1.stdout.splitlines() if l.startswith("{")][0])
    j2 = json.loads([l for l in r2.stdout.splitlines() if l.startswith("{")][0])
    assert j2["n_gpus"] == ranks and j2["config"]["sharding"] == "queries/%d" % ranks
    assert j1["config"]["topk_crc32"] == j2["config"]["topk_crc32"]
    assert j1["distributions"]["n_used"] == j2["distributions"]["n_used"]


def test_single_pair_launches_match_the_batch(orc):
    """One (query, model) pair per call: the planner then picks launch shapes a batch never sees (e.g.
    5 waves per workgroup for a 311-residue query on a 20-cell model).  A build of this round returned
    a score without the null1 term for exactly that shape (a value lost across the non-inlined sweep
    calls), so every pair of the example case is also scored alone and must equal the batch result."""
    _need_gpu()
    from tests.conftest import load_case
    from witch_amd.ehmm import EHMM, pack_queries
    case = load_case("example_sub30")
    e = EHMM(case.hmm_paths, hmm_index=case.hmm_index, nseq=case.nseq)
    seqs = [e.digitize(s_) for s_ in case.qseqs[:40]]
    res, offs = pack_queries(seqs)
    deci, flags = e.score(res, offs)
    ohm = orc.OracleHMM(case.hmm_paths[0])
    for qi, s_ in enumerate(seqs):
        d1, f1 = e.score(*pack_queries([s_]))
        assert (int(d1[0, 0]), int(f1[0, 0])) == (int(deci[qi, 0]), int(flags[qi, 0])), (qi, len(s_))
        r = ohm.score(s_)
        assert (int(f1[0, 0]) & 3) == (r.flags & 3), qi
        _check_one_decibit(d1[0, 0], r.decibits, r.seq_score, ("single pair", qi), LONG_EPS if (r.flags & 2) else BOUNDARY_EPS)
    e.close()


@pytest.mark.parametrize("ehmm_source", ["hmmbuild_files", "wh_hmmbuild"])
def test_end_to_end_example_against_the_reference_pipeline(tmp_path, ehmm_source):
    """north_star: "identical final merged alignment".  The reference's example data (500-row backbone of
    2574 columns, 500 fragments) against a 15-HMM eHMM of the backbone: the GPU chain
    score -> top-k -> align -> consensus -> transitive merge writes the two FASTA files the reference's own
    functions wrote when tests/golden/make_golden_e2e.py chained them (gcmm.py:219-248).  Differences are
    listed per query, not hidden; the multidomain class (HMMER's stochastic resolver) is included."""
    _need_gpu()
    import gzip
    import hashlib
    from tests.conftest import load_case
    from witch_amd import gcmm
    case = load_case("example_e2e")
    g = case.g

    class _Sub:
        def __init__(self, path, n):
            self.hmm_model_path, self.num_taxa = path, n
    index_to_hmm = {i: _Sub(p, n) for i, p, n in zip(case.hmm_index, case.hmm_paths, case.nseq)}
    retained = {int(k): v for k, v in g["retained"].items()}
    nongaps = {int(k): v for k, v in g["nongaps"].items()}
    B = g["backbone_length"]
    bpath = str(tmp_path / "backbone.fasta")
    with gzip.open(os.path.join(case.dir, "backbone.fasta.gz"), "rt") as f, open(bpath, "w") as o:
        o.write(f.read())
    if ehmm_source == "wh_hmmbuild":
        # NO HMMER anywhere: the eHMM itself comes from wh_hmmbuild, built from the reduced subset
        # alignments as the reference builds them, with the tuples it returns
        from witch_amd import synth
        names, rows = [], []
        for line in open(bpath):
            line = line.strip()
            if line.startswith(">"):
                names.append(line[1:].split()[0]); rows.append("")
            elif line:
                rows[-1] += line
        subs = synth.bfs_subsets(len(rows), len(case.hmm_index))
        built = gcmm.build_ehmm(names, rows, [("A_0_%d" % i, list(range(lo, hi))) for i, (lo, hi) in enumerate(subs)],
                                "dna", str(tmp_path / "tree_decomp"))
        index_to_hmm = {i: _Sub(b[0], n) for i, b, n in zip(case.hmm_index, built, case.nseq)}
        retained = {i: list(b[2]) for i, b in zip(case.hmm_index, built)}
        nongaps = {i: list(b[3]) for i, b in zip(case.hmm_index, built)}
    eng = gcmm.install(gcmm.QueryAlignmentEngine.run(
        index_to_hmm, list(zip(case.qnames, case.qseqs)), case.k,
        subset_to_retained_columns=retained, subset_to_nongaps_per_column=nongaps, backbone_length=B))
    # ---- search: reported sets and printed scores of all 15 x 500 pairs against HMMER's
    n_pairs = n_mask = n_score = 0
    for col, hf in enumerate(case.hmm_files):
        S = g["search"][hf]
        for row, qn in enumerate(case.qnames):
            rep = bool(eng.flags[row, col] & 1)
            n_pairs += 1
            if rep != (qn in S):
                n_mask += 1
            elif rep and int(round(S[qn]["score"] * 10)) != int(eng.decibits[row, col]):
                n_score += 1
                assert abs(int(round(S[qn]["score"] * 10)) - int(eng.decibits[row, col])) == 1, (hf, qn)
    multi = int(((eng.flags & 2) != 0).sum())
    # ---- weights / top-k / strings per query
    ranked = gcmm.rankBitscores(index_to_hmm, {})
    weights = gcmm.writeWeights(index_to_hmm, ranked)
    d_set = d_order = d_w = d_str = 0
    queries, differing = [], []
    for q, (qn, qs) in enumerate(zip(case.qnames, case.qseqs)):
        gold_w = g["weights"].get(qn)
        if qn not in weights:
            assert gold_w is None or qn in g["ignored"], qn
            continue
        got = weights[qn]
        if gold_w is None:
            d_set += 1
            differing.append((qn, "reported by the GPU path only"))
        elif [i for i, _ in got] != [i for i, _ in gold_w]:
            if sorted(i for i, _ in got) != sorted(i for i, _ in gold_w):
                d_set += 1
                differing.append((qn, "top-k set"))
            else:
                d_order += 1
                differing.append((qn, "top-k order"))
        elif not np.allclose([x for _, x in got], [x for _, x in gold_w], rtol=1e-9, atol=0):
            d_w += 1
            differing.append((qn, "weights (a score one deci-bit off)"))
        query, _, _ = gcmm.alignSubQueriesNew(bpath, B, index_to_hmm, None, 120, qn, qs, got, q)
        queries.append(query)
        if len(query) and g["merged"].get(qn) is not None and query[qn] != g["merged"][qn]:
            d_str += 1
            if not differing or differing[-1][0] != qn:
                differing.append((qn, "consensus string only"))
    out = str(tmp_path / "witch.fasta")
    o, m = gcmm.mergeAlignmentsCollapsed(bpath, queries, {}, None, output_path=out)
    same_full = hashlib.sha256(open(o, "rb").read()).hexdigest() == g["final_sha256"]["full"]
    same_masked = hashlib.sha256(open(m, "rb").read()).hexdigest() == g["final_sha256"]["masked"]
    print("\n[example_e2e] %d pairs (%d multidomain): %d reported-mask differences, %d scores one deci-bit off; "
          "queries: %d top-k set, %d order, %d weight, %d string differences of %d; final files identical: full %s, masked %s"
          % (n_pairs, multi, n_mask, n_score, d_set, d_order, d_w, d_str, len(case.qnames), same_full, same_masked))
    for qn, why in differing:
        print("   differs: %s (%s)" % (qn, why))
    # observed on MI355X (rounds 2-4, both eHMM sources): 2 mask differences, 1 score, 4 queries with a different low-weight
    # tail (HMMER's stochastic class, SURVEY finding 3) - and BOTH FINAL FILES IDENTICAL to the reference pipeline's.
    # The gate is the observed state plus one; the north-star property itself is asserted unconditionally.
    assert n_mask <= 3 and n_score <= 2, (n_mask, n_score)
    assert d_set + d_order + d_w <= 5, (d_set, d_order, d_w)
    assert d_str == 0, d_str
    assert same_full and same_masked, (same_full, same_masked)
    assert (eng.flags & 8).sum() == 0 and not eng.truncated_pairs and not eng.unaligned_pairs
    # ---- a1 / f4 on the same run: the result files gcmm.search writes (the reference's chunk layout), weights.txt and
    # the checkpoint file, each read back; the merge fed from the checkpoint (the reference's resume path,
    # gcmm.py:205-217) writes the same two files
    import ast
    dirs = {i: str(tmp_path / "tree_decomp" / "root" / ("A_0_%d" % i)) for i in case.hmm_index}
    files, _ = gcmm.search(dirs, num_cpus=4)
    assert len(files) == len(case.hmm_index) * gcmm.num_chunks_for(len(case.hmm_index), 4)
    for col, i in enumerate(case.hmm_index):
        seen = {}
        for f_ in sorted(os.listdir(dirs[i])):
            if f_.startswith("hmmsearch.results."):
                seen.update(ast.literal_eval(open(os.path.join(dirs[i], f_)).read()))
        want = {qn: (0.0, eng.decibits[row, col] / 10.0) for row, qn in enumerate(case.qnames) if eng.flags[row, col] & 1}
        assert seen == want, i
    wpath = str(tmp_path / "weights.txt")
    gcmm.writeWeightsToLocal(weights, wpath)
    back = gcmm.readWeightsFromLocal(wpath)
    assert {t: [(i, float(x)) for i, x in v] for t, v in back.items()} == {t: [(i, float(x)) for i, x in v] for t, v in weights.items()}
    cpath = str(tmp_path / "checkpoint_alignments.txt.gz")
    assert gcmm.writeCheckpointAlignments(queries, cpath) == sum(1 for q_ in queries if len(q_) == 1)
    resumed = gcmm.readCheckpointAlignments(cpath)
    o2, m2 = gcmm.mergeAlignmentsCollapsed(bpath, [resumed[next(iter(q_))] for q_ in queries if len(q_) == 1], {}, None,
                                           output_path=str(tmp_path / "resumed.fasta"))
    assert open(o2, "rb").read() == open(o, "rb").read() and open(m2, "rb").read() == open(m, "rb").read()
    if d_str == 0 and not differing:
        assert same_full and same_masked
    else:
        # the files differ only in the rows of the listed queries (and the gap columns their insertions open)
        def rows(path):
            out_, name = {}, None
            op = gzip.open if path.endswith(".gz") else open
            for line in op(path, "rt"):
                line = line.rstrip("\n")
                if line.startswith(">"):
                    name = line[1:]
                    out_[name] = ""
                else:
                    out_[name] += line
            return out_
        got_rows, want_rows = rows(m), rows(os.path.join(case.dir, "merged.masked.fasta.gz"))
        assert got_rows.keys() == want_rows.keys()
        bad = {n for n in got_rows if got_rows[n] != want_rows[n]}
        assert bad <= {qn for qn, _ in differing}, sorted(bad - {qn for qn, _ in differing})[:5]


@pytest.mark.gpu
def test_a_call_of_two_to_the_31_pairs_is_refused():
    """One scoring call serves fewer than 2^31 pairs.  Until round 4 a larger call ran WITHOUT the multidomain resolver and
    said nothing (a different reported set); now it is refused before anything is touched, and the engine's chunks
    (20 000 queries per call, the reference's hmmsearch chunk) keep every call far below the limit."""
    _need_gpu()
    import torch
    from tests.conftest import load_case
    from witch_amd._lib import lib, WH_ERANGE
    from witch_amd.ehmm import EHMM
    case = load_case("dna_synth")
    e = EHMM(case.hmm_paths, hmm_index=case.hmm_index, nseq=case.nseq)
    dummy = torch.zeros(16, dtype=torch.int64, device="cuda")
    nq = (1 << 31) // e.H + 1
    rc = lib().wh_score_dev(e._h, dummy.data_ptr(), dummy.data_ptr(), nq, 0, 150, dummy.data_ptr(), dummy.data_ptr(), None, None, None)
    assert rc == WH_ERANGE, rc
    assert b"chunks" in lib().wh_last_error()
    e.close()


@pytest.mark.gpu
def test_chunked_engine_run_equals_the_one_pass_run(tmp_path):
    """QueryAlignmentEngine.run feeds the GPU in chunks of at most 20 000 queries like the reference feeds hmmsearch
    (algorithm.py:209,280-284), so nothing on the device grows with the query count.  Chunks are independent, so a run
    in chunks of 257 on the reference's example data (500 fragments x 15 HMMs) gives the tables of the one-pass run -
    scores, flags, top-k records, aligned columns, consensus codes - and the device merge writes the same two files,
    whose sha256 are the reference pipeline's.  With keep_scores=False the score table is dropped and says so."""
    _need_gpu()
    import gzip
    import hashlib
    from tests.conftest import load_case
    from witch_amd import gcmm
    case = load_case("example_e2e")
    g = case.g

    class _Sub:
        def __init__(self, path, n):
            self.hmm_model_path, self.num_taxa = path, n
    index_to_hmm = {i: _Sub(p, n) for i, p, n in zip(case.hmm_index, case.hmm_paths, case.nseq)}
    retained = {int(k): v for k, v in g["retained"].items()}
    nongaps = {int(k): v for k, v in g["nongaps"].items()}
    B = g["backbone_length"]
    bpath = str(tmp_path / "backbone.fasta")
    with gzip.open(os.path.join(case.dir, "backbone.fasta.gz"), "rt") as f, open(bpath, "w") as o:
        o.write(f.read())
    queries = list(zip(case.qnames, case.qseqs))
    kw = dict(subset_to_retained_columns=retained, subset_to_nongaps_per_column=nongaps, backbone_length=B)
    one = gcmm.QueryAlignmentEngine.run(index_to_hmm, queries, case.k, chunk=0, **kw)
    many = gcmm.QueryAlignmentEngine.run(index_to_hmm, queries, case.k, chunk=257, **kw)
    assert one.timings["chunks"] == 1 and many.timings["chunks"] == 2
    for name in ("decibits", "flags", "topk_idx", "n_kept", "n_used", "cols", "col_offsets", "merged", "merged_minmax", "qpair_off"):
        assert np.array_equal(getattr(one, name), getattr(many, name)), name
    assert np.array_equal(one.topk_w.view(np.uint64), many.topk_w.view(np.uint64))
    for row in (0, 256, 257, 499):
        for lab, _ in many.weights(row)[:int(many.n_used[row])]:
            assert many.aligned_columns(row, lab) == one.aligned_columns(row, lab)
    gcmm.install(many)
    o, m = gcmm.mergeAlignmentsDevice(bpath, {}, output_path=str(tmp_path / "chunked.fasta"))
    assert hashlib.sha256(open(o, "rb").read()).hexdigest() == g["final_sha256"]["full"]
    assert hashlib.sha256(open(m, "rb").read()).hexdigest() == g["final_sha256"]["masked"]
    lean = gcmm.QueryAlignmentEngine.run(index_to_hmm, queries, case.k, chunk=100, keep_scores=False, **kw)
    assert lean.decibits is None and lean.flags is None and np.array_equal(lean.merged, one.merged)
    with pytest.raises(RuntimeError):
        lean.ranked(0)


@pytest.mark.gpu
def test_ehmm_built_without_hmmbuild_scores_identically(tmp_path):
    """the eHMM of the end-to-end example built by wh_hmmbuild (no STATS / MAXL lines, from the
    reduced subset alignments as the reference builds them) loads and scores exactly like the files HMMER's
    hmmbuild wrote: same deci-bits, flags, top-k and aligned columns for all 500 fragments."""
    _need_gpu()
    import gzip
    from witch_amd import synth
    from witch_amd.ehmm import EHMM, pack_queries
    from witch_amd.gcmm.hmmbuild import build_ehmm
    from tests.conftest import load_case
    case = load_case("example_e2e")
    names, rows = [], []
    with gzip.open(os.path.join(case.dir, "backbone.fasta.gz"), "rt") as fh:
        for line in fh:
            line = line.strip()
            if line.startswith(">"):
                names.append(line[1:].split()[0]); rows.append("")
            elif line:
                rows[-1] += line
    subs = synth.bfs_subsets(len(rows), 15)
    built = build_ehmm(names, rows, [("A_0_%d" % i, list(range(lo, hi))) for i, (lo, hi) in enumerate(subs)], "dna", str(tmp_path))
    e1 = EHMM(case.hmm_paths, hmm_index=case.hmm_index, nseq=case.nseq)
    e2 = EHMM([b[0] for b in built], hmm_index=case.hmm_index, nseq=case.nseq)
    assert np.array_equal(e1.M, e2.M)
    seqs = [e1.digitize(s) for s in case.qseqs]
    res, offs = pack_queries(seqs)
    d1, f1 = e1.score(res, offs)
    d2, f2 = e2.score(res, offs)
    assert np.array_equal(d1, d2) and np.array_equal(f1, f2)
    i1, w1, _, nu1 = e1.topk(d1, f1, case.k)
    i2, w2, _, nu2 = e2.topk(d2, f2, case.k)
    assert np.array_equal(i1, i2) and np.array_equal(w1, w2) and np.array_equal(nu1, nu2)
    pq = [q for q in range(0, len(seqs), 10) for _ in range(int(nu1[q]))]
    ph = [e1.pos_of_index[int(i1[q, j])] for q in range(0, len(seqs), 10) for j in range(int(nu1[q]))]
    c1, o1 = e1.align(res, offs, pq, ph)
    c2, o2 = e2.align(res, offs, pq, ph)
    assert np.array_equal(o1, o2)
    # aligned columns are MODEL columns (0-based node index); the MAP numbers differ (reduced vs full alignment)
    assert np.array_equal(c1, c2)
    e1.close(); e2.close()


@pytest.mark.gpu
def test_device_merge_writes_the_host_mergers_bytes(tmp_path):
    """SURVEY 8f #2 on the device: wh_merge (codes of the consensus kernel -> the two final matrices) against the
    host closed form fed with the per-query strings, on the end-to-end example (500 fragments into a 500-row
    backbone; insertion runs at hundreds of gaps, leading / trailing insertions, a renamed taxon) - and against the
    reference pipeline's own two files (sha256 of the golden)."""
    _need_gpu()
    import gzip
    import hashlib
    from tests.conftest import load_case
    from witch_amd import gcmm
    case = load_case("example_e2e")
    g = case.g

    class _Sub:
        def __init__(self, path, n):
            self.hmm_model_path, self.num_taxa = path, n
    index_to_hmm = {i: _Sub(p, n) for i, p, n in zip(case.hmm_index, case.hmm_paths, case.nseq)}
    retained = {int(k): v for k, v in g["retained"].items()}
    nongaps = {int(k): v for k, v in g["nongaps"].items()}
    B = g["backbone_length"]
    bpath = str(tmp_path / "backbone.fasta")
    with gzip.open(os.path.join(case.dir, "backbone.fasta.gz"), "rt") as f, open(bpath, "w") as o:
        o.write(f.read())
    eng = gcmm.install(gcmm.QueryAlignmentEngine.run(
        index_to_hmm, list(zip(case.qnames, case.qseqs)), case.k,
        subset_to_retained_columns=retained, subset_to_nongaps_per_column=nongaps, backbone_length=B))
    weights = gcmm.writeWeights(index_to_hmm, gcmm.rankBitscores(index_to_hmm, {}))
    taxa = [qn for qn in case.qnames if qn in weights]
    queries = [gcmm.alignSubQueriesNew(bpath, B, index_to_hmm, None, 120, qn, qs, weights[qn], q)[0]
               for q, (qn, qs) in enumerate(zip(case.qnames, case.qseqs)) if qn in weights]
    rename = {taxa[3]: taxa[3] + "_renamed_original"}          # merger.py:84-93: renamed taxa move to the end
    for tag, ren in (("plain", {}), ("renamed", rename)):
        h_full, h_masked = gcmm.mergeAlignmentsCollapsed(bpath, queries, ren, None, output_path=str(tmp_path / ("host_%s.fasta" % tag)))
        d_full, d_masked = gcmm.mergeAlignmentsDevice(bpath, ren, output_path=str(tmp_path / ("dev_%s.fasta" % tag)), taxa=taxa)
        assert open(h_full, "rb").read() == open(d_full, "rb").read(), tag
        assert open(h_masked, "rb").read() == open(d_masked, "rb").read(), tag
        if tag == "plain":
            assert hashlib.sha256(open(d_full, "rb").read()).hexdigest() == g["final_sha256"]["full"]
            assert hashlib.sha256(open(d_masked, "rb").read()).hexdigest() == g["final_sha256"]["masked"]
    # default taxa = every query with a reported HMM, batch order
    d2, _ = gcmm.mergeAlignmentsDevice(bpath, {}, output_path=str(tmp_path / "dev_default.fasta"))
    assert open(d2, "rb").read() == open(str(tmp_path / "dev_plain.fasta"), "rb").read()


@pytest.mark.gpu
def test_device_merge_on_every_golden_case(golden_case, tmp_path):
    """wh_merge == the host closed-form merger on every golden case that has consensus data (short DNA, protein,
    degenerate residues, chimeric and very short queries -> leading / trailing / interior insertion runs), with a
    stand-in backbone (the merge never looks at the backbone's characters) that already contains one query's name
    (that query widens the gaps but gets no row, alignment_tools.py:1226-1230)."""
    _need_gpu()
    from witch_amd import gcmm
    case = golden_case
    g = case.g
    if not g.get("merged"):
        pytest.skip("case has no backbone alignment")

    class _Sub:
        def __init__(self, path, n):
            self.hmm_model_path, self.num_taxa = path, n
    index_to_hmm = {i: _Sub(p, n) for i, p, n in zip(case.hmm_index, case.hmm_paths, case.nseq)}
    retained = {int(k): v for k, v in g["retained"].items()}
    nongaps = {int(k): v for k, v in g["nongaps"].items()}
    B = g["backbone_length"]
    gcmm.install(gcmm.QueryAlignmentEngine.run(
        index_to_hmm, list(zip(case.qnames, case.qseqs)), case.k,
        subset_to_retained_columns=retained, subset_to_nongaps_per_column=nongaps, backbone_length=B))
    weights = gcmm.writeWeights(index_to_hmm, gcmm.rankBitscores(index_to_hmm, {}))
    taxa = [qn for qn in case.qnames if qn in weights]
    assert len(taxa) >= 2
    queries = [gcmm.alignSubQueriesNew("bb", B, index_to_hmm, None, 120, qn, qs, weights[qn], q)[0]
               for q, (qn, qs) in enumerate(zip(case.qnames, case.qseqs)) if qn in weights]
    sym = "ACDEFGHIKLMNPQRSTVWY" if case.alphabet == "amino" else "ACGT"
    rng = np.random.default_rng(5)
    bpath = str(tmp_path / "bb.fasta")
    with open(bpath, "w") as f:
        for r, name in enumerate(["bb0", "bb1", taxa[1], "bb3"]):
            row = "".join(sym[int(x)] if rng.random() > 0.2 else "-" for x in rng.integers(0, len(sym), size=B))
            f.write(">%s\n%s\n" % (name, row))
    h_full, h_masked = gcmm.mergeAlignmentsCollapsed(bpath, queries, {}, None, output_path=str(tmp_path / "host.fasta"))
    d_full, d_masked = gcmm.mergeAlignmentsDevice(bpath, {}, output_path=str(tmp_path / "dev.fasta"), taxa=taxa)
    assert open(h_full, "rb").read() == open(d_full, "rb").read(), case.name
    assert open(h_masked, "rb").read() == open(d_masked, "rb").read(), case.name


@pytest.mark.gpu
@pytest.mark.parametrize("ranks", [2, 4])
def test_multi_rank_level1_writes_the_reference_files(tmp_path, ranks):
    """SURVEY 8e through the PRODUCT path, rehearsed with two and four ranks on one GPU (gloo):
    sharded engine -> gathered top-k -> mergeAlignmentsDevice with the all-reduced gap widths -> rank 0 writes.
    The two files must be the reference pipeline's (sha256 of the end-to-end golden), like the one-rank run."""
    _need_gpu()
    import json
    import socket
    import subprocess
    import sys
    from tests.conftest import ROOT, load_case
    g = load_case("example_e2e").g
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", WITCH_LEVEL1_REHEARSAL="1")
    script = os.path.join(ROOT, "tools", "level1_ranks.py")
    r1 = subprocess.run([sys.executable, script, str(tmp_path / "one.fasta")], capture_output=True, text=True, timeout=600, env=env)
    assert r1.returncode == 0, r1.stderr[-2000:]
    r2 = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks),
                         "--master-addr", "127.0.0.1", "--master-port", str(port), script, str(tmp_path / "many.fasta")],
                        capture_output=True, text=True, timeout=600, env=env)
    assert r2.returncode == 0, r2.stderr[-2000:]
    j1 = json.loads([l for l in r1.stdout.splitlines() if l.startswith("{")][0])
    j2 = json.loads([l for l in r2.stdout.splitlines() if l.startswith("{")][0])
    assert j2["world"] == ranks and j2["rows_local"] == [0, 500 // ranks]
    for j in (j1, j2):
        assert j["full"] == g["final_sha256"]["full"] and j["masked"] == g["final_sha256"]["masked"]


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _json_line(text):
    import json
    return json.loads([l for l in text.splitlines() if l.startswith("{")][0])


@pytest.mark.gpu
def test_rccl_collectives_on_one_gpu(tmp_path):
    """The `nccl` (= RCCL) branch executed on hardware: bench.py and the level-1 chain started as fresh children under
    torch.distributed.run with ONE rank and WITCH_FORCE_COLLECTIVES=1 - init_process_group("nccl"), the top-k
    all-gather on DEVICE tensors, the merge's MAX all-reduce on a device tensor and the row gather all run through
    RCCL; the gathered top-k CRC equals the plain run's and the level-1 chain writes the reference pipeline's files."""
    _need_gpu()
    import subprocess
    import sys
    from tests.conftest import ROOT, load_case
    common = ["--steps", "1", "--warmup", "0", "--nq", "3001", "--nh", "12", "--no-cpu-baseline"]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    env.pop("WITCH_FORCE_COLLECTIVES", None)
    r1 = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + common,
                        capture_output=True, text=True, timeout=900, env=env)
    assert r1.returncode == 0, r1.stderr[-2000:]
    envf = dict(env, WITCH_FORCE_COLLECTIVES="1")
    launcher = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1"]
    r2 = subprocess.run(launcher + ["--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "1"] + common,
                        capture_output=True, text=True, timeout=900, env=envf)
    assert r2.returncode == 0, r2.stderr[-3000:]
    j1, j2 = _json_line(r1.stdout), _json_line(r2.stdout)
    assert j1["config"]["collective_backend"] is None and j2["config"]["collective_backend"] == "nccl"
    assert j1["config"]["topk_crc32"] == j2["config"]["topk_crc32"]
    g = load_case("example_e2e").g
    script = os.path.join(ROOT, "tools", "level1_ranks.py")
    r3 = subprocess.run(launcher + ["--master-port", str(_free_port()), script, str(tmp_path / "rccl.fasta")],
                        capture_output=True, text=True, timeout=600, env=envf)
    assert r3.returncode == 0, r3.stderr[-3000:]
    j3 = _json_line(r3.stdout)
    assert j3["backend"] == "nccl" and j3["world"] == 1
    assert j3["full"] == g["final_sha256"]["full"] and j3["masked"] == g["final_sha256"]["masked"]


@pytest.mark.gpu
def test_two_rank_rehearsal_of_the_protein_shape(tmp_path):
    """BASELINE.json configs[4]'s shape rehearsed with two ranks on the one GPU (gloo gather): 2 000 mixed-length protein
    queries x all 500 HMMs, sharded 1 000 / 1 000, must gather exactly the 1-rank top-k table."""
    _need_gpu()
    import subprocess
    import sys
    from tests.conftest import ROOT
    common = ["--workload", "aa_50k_x500", "--steps", "1", "--warmup", "0", "--nq", "2000", "--full", "--no-cpu-baseline"]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    env.pop("WITCH_FORCE_COLLECTIVES", None)
    import pathlib
    import signal
    import types

    def run(cmd, env_, tag):
        # A child that stops must fail THIS test with what it last said (a silent wait gets the whole GPU run killed): output
        # to files (a pipe stays open while any grandchild lives), own process group, every member killed at the limit.
        keep = os.path.join(os.environ.get("GRAFT_REPO_ROOT", ""), "gpurun_out")      # (kept when the GPU box has the scratch directory)
        where = pathlib.Path(keep) if os.path.isdir(keep) else tmp_path
        out, err = where / ("rehearsal_" + tag + ".out"), where / ("rehearsal_" + tag + ".err")
        with open(out, "w") as fo, open(err, "w") as fe:
            p = subprocess.Popen(cmd, stdout=fo, stderr=fe, env=dict(env_, WITCH_BENCH_WATCHDOG="150"), start_new_session=True)
            try:
                rc = p.wait(timeout=240)
            except subprocess.TimeoutExpired:
                os.killpg(p.pid, signal.SIGKILL)
                p.wait()
                import torch
                free_b, total_b = torch.cuda.mem_get_info()
                pytest.fail("no result after 240 s (device memory free %.1f of %.1f GB): %s\n%s" % (free_b / 1e9, total_b / 1e9, " ".join(cmd[-12:]), err.read_text()[-6000:]))
        return types.SimpleNamespace(returncode=rc, stdout=out.read_text(), stderr=err.read_text())
    # Two ranks on ONE card need two workspaces for 2 000-residue protein queries (~100 GB each: envelope slabs and the resolver's
    # float64 matrices of every resident wave).  A card that cannot hold them does not fail the allocation: the ranks hang inside
    # the driver and cannot be killed - so ask first.
    import torch
    torch.cuda.empty_cache()
    free_b, total_b = torch.cuda.mem_get_info()
    assert free_b >= 230e9, "this process (or another) holds %.0f GB of the card's %.0f GB: close the handles of earlier tests" % ((total_b - free_b) / 1e9, total_b / 1e9)
    r1 = run([sys.executable, "-X", "faulthandler", os.path.join(ROOT, "bench.py"), "--gpus", "1"] + common, env, "one_rank")
    assert r1.returncode == 0, r1.stderr[-2000:]
    r2 = run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
              "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
              os.path.join(ROOT, "bench.py"), "--gpus", "2"] + common, dict(env, WITCH_BENCH_REHEARSAL="1"), "two_ranks")
    assert r2.returncode == 0, r2.stderr[-2000:]
    j1, j2 = _json_line(r1.stdout), _json_line(r2.stdout)
    assert j2["n_gpus"] == 2 and j2["config"]["n_hmms"] == 500 and j2["config"]["n_queries"] == 2000
    assert j1["config"]["topk_crc32"] == j2["config"]["topk_crc32"]
    assert j1["distributions"]["n_used"] == j2["distributions"]["n_used"]


@pytest.mark.gpu
def test_consensus_with_twenty_models_on_a_20000_column_backbone():
    """The consensus kernel beyond its round-2 limits (k <= 16, backbones of <= ~19 000 columns: the DP row in LDS):
    k = 20 kept models per query and a backbone of 20 000 columns (the DP row then lives in the wave's HBM region).
    The 20 protein models of amino_multidomain, their match states mapped to random increasing columns of a
    20 000-column backbone, short query windows aligned to ALL 20 models with random weights; codes and touched
    range must equal the Python restatement of aligner.py:376-473."""
    _need_gpu()
    from oracle import consensus as ocons
    from tests.conftest import load_case
    from witch_amd.ehmm import EHMM, pack_queries
    case = load_case("amino_multidomain")
    e = EHMM(case.hmm_paths, hmm_index=case.hmm_index, nseq=case.nseq)
    assert e.H == 20
    rng = np.random.default_rng(11)
    B = 20000
    retained = [np.sort(rng.choice(B, size=int(m), replace=False)).astype(np.int32) for m in e.M]
    nongaps = [rng.integers(1, 60, size=int(m)).astype(np.int32) for m in e.M]
    # windows of the first queries: 40-70 residues from inside a family domain
    seqs = []
    for qi in range(5):
        full = e.digitize(case.qseqs[qi])
        lo = int(rng.integers(0, max(1, len(full) - 80)))
        seqs.append(full[lo:lo + int(rng.integers(40, 71))])
    res, offs = pack_queries(seqs)
    pq = [q for q in range(len(seqs)) for _ in range(e.H)]
    ph = [h for _ in range(len(seqs)) for h in range(e.H)]
    cols, co = e.align(res, offs, pq, ph)
    w = rng.random(len(pq))
    qpo = np.arange(len(seqs) + 1, dtype=np.int64) * e.H
    codes, mm = e.consensus(offs, qpo, ph, w, co, cols, retained, nongaps, B)
    n_span = 0
    for q in range(len(seqs)):
        L = len(seqs[q])
        aligned = [(h, cols[co[q * e.H + h]:co[q * e.H + h + 1]].tolist()) for h in range(e.H)]
        want, (mn, mx) = ocons.consensus_trace(L, aligned, {h: w[q * e.H + h] for h in range(e.H)},
                                               {h: retained[h] for h in range(e.H)}, {h: nongaps[h] for h in range(e.H)}, B)
        assert codes[offs[q]:offs[q + 1]].tolist() == want, q
        assert (int(mm[q, 0]), int(mm[q, 1])) == (mn, mx), q
        n_span = max(n_span, mx - mn + 1)
    assert n_span > 3000          # the DP really ran over thousands of columns
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cells_per_lane", [4, 12, 16, 24])
def test_several_waves_per_pair_kernel_on_the_golden_cases(cells_per_lane, orc):
    """wh_score_wide.hip (models of 3 073 - 12 288 nodes in production: several wavefronts per pair, the D scan and the
    row sums crossing the waves through LDS) forced onto the golden cases (WH_FORCE_WIDE, read at wh_ehmm_load): with
    4 cells per lane a 1 211-node model runs on 5 waves, with 24 on one - every workgroup size from 1 to 5 - and with 12 / 16
    through the variants that keep the transition tables in registers and the emission rows in LDS (production: 3 073 -
    6 144 / 6 145 - 8 192 nodes), against the oracle: Forward log-odds, flags and deci-bit scores (multidomain pairs through the same resolver queue), and the
    aligned columns of the several-waves-per-pair alignment kernel (pairs that leave float32 range are handed to the
    float64 kernel, as in production)."""
    _need_gpu()
    from tests.conftest import load_case
    from witch_amd.ehmm import EHMM, pack_queries
    old = os.environ.get("WH_FORCE_WIDE")
    os.environ["WH_FORCE_WIDE"] = str(cells_per_lane)
    try:
        for name in ("dna_synth", "dna_hmmbuild", "amino_hmmbuild", "example_sub30"):
            case = load_case(name)
            e = EHMM(case.hmm_paths, hmm_index=case.hmm_index, nseq=case.nseq)
            seqs = [e.digitize(s_) for s_ in case.qseqs]
            res, offs = pack_queries(seqs)
            deci, flags, fwd = e.score(res, offs, want_fwd=True)
            # ... and the several-waves-per-pair ALIGNMENT kernel: every query against the first two models
            pq = [q for q in range(len(seqs)) for _ in range(min(2, e.H))]
            ph = [h for _ in range(len(seqs)) for h in range(min(2, e.H))]
            cols, co = e.align(res, offs, pq, ph)
            e.close()
            ohm = [orc.OracleHMM(p) for p in case.hmm_paths]
            for p_ in range(len(pq)):
                want = ohm[ph[p_]].align(seqs[pq[p_]])
                assert np.array_equal(cols[co[p_]:co[p_ + 1]], want), (name, "alignment", pq[p_], ph[p_])
            od, of, ofwd, osc = orc.score_batch(ohm, res, offs)
            fin = np.isfinite(ofwd)
            assert np.max(np.abs(fwd[fin] - ofwd[fin])) <= 1e-4, (name, float(np.max(np.abs(fwd[fin] - ofwd[fin]))))
            assert np.array_equal(flags & 7, of & 7), name
            multi = (of & 2) != 0
            _check_decibits(np.where(multi, od, deci), od, osc, (of & 1) == 1, name)
            _check_decibits(np.where(multi, deci, od), od, osc, (of & 1) == 1, name + " (multidomain)", LONG_EPS)
    finally:
        if old is None:
            os.environ.pop("WH_FORCE_WIDE", None)
        else:
            os.environ["WH_FORCE_WIDE"] = old


@pytest.mark.gpu
@pytest.mark.parametrize("alphabet,root_len,qlen", [("dna", 1000, 150), ("dna", 1500, (60, 420)), ("dna", 500, (30, 300)), ("amino", 700, (40, 260))])
def test_alignment_on_a_node_window_equals_the_full_width_passes(alphabet, root_len, qlen, tmp_path):
    """Fragment queries are aligned on the 256 / 512 nodes around the dominant Forward path (wh_align.hip:
    align_window): every column must equal what the full-width sweeps (option WH_NO_WINDOW) produce, on family
    fragments, on fragments with random flanks and on pure background sequences; and the window path must
    actually have run (wh_last_align_paths)."""
    _need_gpu()
    from witch_amd import synth
    from witch_amd.ehmm import EHMM, pack_queries
    fam = synth.make_family(4242 + root_len, root_len, 16, alphabet, 0.04 if alphabet == "dna" else 0.03, 1e-4)
    eh = synth.make_ehmm(fam, 6, str(tmp_path), witch_layout=False)
    e = EHMM(eh.paths, hmm_index=eh.index, nseq=eh.nseq)
    _, s1 = synth.make_queries(fam, 11, 300, qlen, 0.05)
    _, s2 = synth.make_queries(fam, 12, 150, qlen, 0.15, flank_frac=0.4)
    rng = np.random.default_rng(5)
    K = 4 if alphabet == "dna" else 20
    s3 = [rng.integers(0, K, size=int(rng.integers(20, 200))).astype(np.int8) for _ in range(50)]
    seqs = [s.astype(np.uint8) for s in s1 + s2 + s3]
    res, offs = pack_queries(seqs)
    H = len(eh.paths)
    pq = np.repeat(np.arange(len(seqs), dtype=np.int64), H)
    ph = np.tile(np.arange(H, dtype=np.int32), len(seqs))
    cw, co = e.align(res, offs, pq, ph)
    paths = e.last_align_paths()
    e.set_option("WH_NO_WINDOW", "1")
    cf, co2 = e.align(res, offs, pq, ph)
    paths_full = e.last_align_paths()
    e.set_option("WH_NO_WINDOW", "")
    e.close()
    assert np.array_equal(co, co2)
    bad = np.flatnonzero(cw != cf)
    assert bad.size == 0, (bad[:10], cw[bad[:10]], cf[bad[:10]])
    n = len(pq)
    assert sum(paths.values()) == n and paths_full == {"window256": 0, "window512": 0, "window_rejected": 0, "full_width": n}
    if int(e.M.max()) >= 512:       # 8 or more nodes per lane: fragments go through a window
        assert paths["window256"] + paths["window512"] > n // 2, paths


@pytest.mark.gpu
def test_forward_rows_that_underflow_to_zero_are_written(orc, tmp_path):
    """A strong family window followed by a long random flank: after the hit the Forward sweep has rescaled by ~2^-300,
    the flank's rows underflow to zero in every cell, and `0 > -0` must not keep them from being written - the
    full-width Backward sweep reads rows without looking at the masks and used to see the previous pair's cells there
    (found by tests/tools/fuzz_align.py, seed 103; before the fix one of the three pairs below differed from the oracle in
    every call that followed another pair in the same slab)."""
    _need_gpu()
    import importlib.util
    from tests.conftest import ROOT
    from witch_amd.ehmm import EHMM, pack_queries
    spec = importlib.util.spec_from_file_location("fuzz_align", os.path.join(ROOT, "tests", "tools", "fuzz_align.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    alph, root, eh, seqs = fz.make_case(103, str(tmp_path))
    e = EHMM(eh.paths, hmm_index=eh.index, nseq=eh.nseq)
    res, offs = pack_queries(seqs)
    ohm = [orc.OracleHMM(p) for p in eh.paths]
    allp = [(q, h) for q in range(len(seqs)) for h in range(e.H)]
    for sel in (allp, [(1, 0), (1, 1), (1, 2)], [(1, 0), (1, 1), (1, 2)], allp):
        cols, co = e.align(res, offs, [q for q, _ in sel], [h for _, h in sel])
        for p, (q, h) in enumerate(sel):
            assert np.array_equal(cols[co[p]:co[p + 1]], ohm[h].align(seqs[q])), (q, h, len(seqs[q]))
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tool,args", [
    ("fuzz_align.py", ["100", "6"]),                       # 300-1 600-node families (seed 103: the round-3 spill bug)
    ("fuzz_align.py", ["3000", "2", "1600", "3072"]),      # pass-synchronous kernels
    ("fuzz_align.py", ["6000", "1", "3100", "6000"]),      # several-waves-per-pair kernels: 12-cell lanes, tables in registers
    ("fuzz_align.py", ["6501", "1", "6200", "8000"]),      # ... 24-cell lanes, tables from L2 (beyond 6 144 nodes)
    ("fuzz_resolver.py", ["1", "8"]),                      # multidomain resolver: two- and three-copy queries, DNA and protein
    ("fuzz_built_models.py", ["1", "10"]),                 # models written by wh_hmmbuild from random alignments
    ("fuzz_level1.py", ["200", "4", "4"]),                 # consensus rows and merged files through the level-1 functions
    ("fuzz_topk.py", ["1", "12"]),                         # weights / top-k / cut with engineered ties
])
def test_randomised_tools_find_no_difference(tool, args):
    """A short run of each randomised check under tools/ (the campaigns of DESIGN section 9.2b use the same programs with
    more seeds): scores under the exact boundary rule, flags, aligned columns in three pair orders, consensus rows,
    merged files and top-k rows all equal to the oracle's."""
    _need_gpu()
    import subprocess
    import sys
    from tests.conftest import ROOT
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", tool)] + args, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (tool, r.stdout[-1500:], r.stderr[-1500:])
