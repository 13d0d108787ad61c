"""Queries beyond the resolver's LDS block: the long-query pass against the CPU oracle.

The resolver's per-wave LDS block holds the query (a byte per residue) and the emitting state of every residue (2 bytes, 4
with a model of more than 32 767 nodes).  A call whose longest query does not fit used to run WITHOUT the resolver: every
multidomain region of every pair of the call stayed one envelope.  Now the main resolver launches are sized for a length
cap that keeps their occupancy, a pair of a longer query is listed, and the long-query pass resolves it with the two
per-residue arrays in the wave's HBM block (include/witch_hip.h: wh_last_long_query_pairs).  The inputs: 60 000 and
100 000 residues of uniform background with three mutated partial copies of a model's consensus at L/3 (two regions, one
of them resolved into two domains), on the golden hmmbuild models (129 / 99 nodes: the 4-cell class, which the scoring
kernels accept at these lengths).  The oracle is the reference; the tolerance is the project's boundary rule for the
multidomain class (tests/test_gpu_parity.py: _check_decibits with LONG_EPS)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.test_gpu_parity import LONG_EPS, _check_decibits, _need_gpu, orc  # noqa: F401  (orc: the oracle fixture)
from witch_amd._lib import WH_MAX_ENVELOPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (60000, 100000)
SEEDS = (0, 1, 2, 3)
ALPHABETS = ("dna", "amino")
LDS_BUDGET = 160 * 1024 - 512            # witch_amd/csrc/wh_host.h: kLdsBudget


def _paths(alph):
    return [os.path.join(ROOT, "tests", "golden", "%s_hmmbuild" % alph, "hmms", "A_0_%d.hmm" % i) for i in (0, 1)]


def _consensus(h):
    return np.argmax(h.odds[:h.K, 1:], axis=0).astype(np.uint8)


def _mutated(rng, part, K):
    c = part.copy()
    hit = rng.random(len(c)) < 0.25
    c[hit] = rng.integers(0, K, size=int(hit.sum())).astype(np.uint8)
    return c


def _three_copies(rng, h):
    cons, M = _consensus(h), h.M
    return [_mutated(rng, p, h.K) for p in (cons[:int(0.8 * M)], cons[int(0.3 * M):], cons[:int(0.6 * M)])]


def _long_query(h, L, seed):
    """Uniform background of L residues; at L/3 three mutated partial copies of the consensus of <h>, back to back."""
    rng = np.random.default_rng(seed)
    seq = rng.integers(0, h.K, size=L).astype(np.uint8)
    pos = L // 3
    for c in _three_copies(rng, h):
        seq[pos:pos + len(c)] = c
        pos += len(c)
    return seq


def _many_regions_query(h, L=60000):
    """20 separated consensus copies (a region each), the three-copy block (two regions, one multidomain), background."""
    rng = np.random.default_rng(977)
    seq = rng.integers(0, h.K, size=L).astype(np.uint8)
    cons = _consensus(h)
    pos = 2000
    for _ in range(20):
        c = _mutated(rng, cons, h.K)
        seq[pos:pos + len(c)] = c
        pos += len(c) + 700
    pos += 5000
    for c in _three_copies(rng, h):
        seq[pos:pos + len(c)] = c
        pos += len(c)
    return seq


def _short_two_copy_queries(h, n=200):
    """Two copies of a mutated consensus window back to back inside random flanks: 150-600 residues, a multidomain region."""
    rng = np.random.default_rng(31)
    cons, out = _consensus(h), []
    for _ in range(n):
        w = int(rng.integers(75, h.M + 1))
        s0 = int(rng.integers(0, h.M - w + 1))
        c = cons[s0:s0 + w].copy()
        hit = rng.random(w) < 0.05
        c[hit] = rng.integers(0, h.K, size=int(hit.sum())).astype(np.uint8)
        total = int(rng.integers(max(150, 2 * w), 601))
        left = int(rng.integers(0, total - 2 * w + 1))
        out.append(np.concatenate([rng.integers(0, h.K, size=left).astype(np.uint8), c, c,
                                   rng.integers(0, h.K, size=total - 2 * w - left).astype(np.uint8)]))
    return out


class _Inputs:
    """The models of one alphabet, the test queries and the oracle's results of each (computed once per module)."""

    def __init__(self, orc_mod, alph):
        self.alph = alph
        self.paths = _paths(alph)
        self.ohm = [orc_mod.OracleHMM(p) for p in self.paths]
        self.long_keys = [(L, s) for L in LENGTHS for s in SEEDS]
        self._seqs, self._scored = {}, {}

    def seq(self, key):
        if key not in self._seqs:
            if key == "many":
                self._seqs[key] = _many_regions_query(self.ohm[0])
            elif key[0] == "short":
                for t, s in enumerate(_short_two_copy_queries(self.ohm[0])):
                    self._seqs[("short", t)] = s
            else:
                self._seqs[key] = _long_query(self.ohm[0], *key)
        return self._seqs[key]

    def short_keys(self):
        self.seq(("short", 0))
        return [k for k in self._seqs if k != "many" and k[0] == "short"]

    def oracle(self, key):
        if key not in self._scored:
            self._scored[key] = [h.score(self.seq(key)) for h in self.ohm]
        return self._scored[key]

    def ehmm(self):
        from witch_amd.ehmm import EHMM
        return EHMM(self.paths, hmm_index=[0, 1], nseq=[h.nseq for h in self.ohm])


@pytest.fixture(scope="module")
def inputs(orc):  # noqa: F811
    return {a: _Inputs(orc, a) for a in ALPHABETS}


def _check_against_oracle(ohm, results, deci, flags, det, ctx):
    """Every pair: no WH_FLAG_TRUNC, the oracle's reported / multidomain bits, region and envelope counts, deci-bits under the
    boundary rule.  <results>: per query the oracle's results on every model."""
    H, nq = len(ohm), len(results)
    od = np.zeros((nq, H), dtype=np.int32)
    of = np.zeros((nq, H), dtype=np.uint8)
    osc = np.zeros((nq, H), dtype=np.float32)
    for q, rs in enumerate(results):
        for h, r in enumerate(rs):
            od[q, h], of[q, h], osc[q, h] = r.decibits, r.flags & 0xFF, r.seq_score
            d = det[q * H + h]
            if q < 24 or int(deci[q, h]) != r.decibits or d.nenv != min(r.nenv, WH_MAX_ENVELOPES) or d.nregions != r.nregions:
                print(ctx, q, h, "device", int(deci[q, h]), int(flags[q, h]), d.nregions, d.nenv, "oracle", r.decibits, r.flags, r.nregions, r.nenv)
    assert (flags & 8).sum() == 0, ("WH_FLAG_TRUNC", ctx, np.argwhere(flags & 8)[:8])
    assert np.array_equal(flags & 3, of & 3), (ctx, np.argwhere((flags & 3) != (of & 3))[:8])
    for q, rs in enumerate(results):
        for h, r in enumerate(rs):
            d = det[q * H + h]
            assert d.nregions == r.nregions, (ctx, q, h, d.nregions, r.nregions)
            assert d.nenv == min(r.nenv, WH_MAX_ENVELOPES), (ctx, q, h, d.nenv, r.nenv)
    _check_decibits(deci, od, osc, (of & 1) == 1, ctx, LONG_EPS)


def _resolver_pairs(results):
    """Pairs the long-query pass takes: a multidomain region (the resolver's queue) or more regions than a scoring kernel lists
    (the long-list pass hands every such pair to the resolver)."""
    return sum(1 for rs in results for r in rs if (r.flags & 2) or r.nregions > WH_MAX_ENVELOPES)


def _lds_formulas():
    """resolve_lds_bytes(Lcap, Mmax) and generic_lds_bytes(Lcap) of the built library (C++ functions of namespace wh)."""
    from witch_amd._lib import lib
    L = lib()
    res, gen = getattr(L, "_ZN2wh17resolve_lds_bytesEii"), getattr(L, "_ZN2wh17generic_lds_bytesEi")
    res.restype, res.argtypes = C.c_size_t, [C.c_int, C.c_int]
    gen.restype, gen.argtypes = C.c_size_t, [C.c_int]
    return res, gen


# ------------------------------------------------------------------------------------------------ CPU
def test_the_lengths_are_beyond_the_resolver_cap_and_below_the_scoring_caps():
    """The two inequalities that make the GPU tests mean something, from the library's own formulas: the resolver's LDS block
    of one wave does not fit at 60 000 or 100 000 residues (it does at 50 000), the any-size front end's does."""
    res, gen = _lds_formulas()
    for M in (99, 129, 200):
        assert res(50000, M) <= LDS_BUDGET
        for L in LENGTHS:
            assert res(L, M) > LDS_BUDGET, (L, M, res(L, M))
            assert gen(L) <= LDS_BUDGET, (L, gen(L))
    assert res(31000, 40000) <= LDS_BUDGET < res(32000, 40000)       # 32-bit states: the cap DESIGN.md section 8 names


def test_oracle_counts_of_the_long_inputs(inputs):
    """Guards the inputs, not the feature: on the model whose consensus they carry the oracle finds REPORTED|MULTI, two
    regions and three envelopes on every long query; on the other model of the eHMM a multidomain region too.  The
    many-regions query has more regions than WH_MAX_ENVELOPES and a multidomain one."""
    for alph in ALPHABETS:
        inp = inputs[alph]
        for key in inp.long_keys:
            rs = inp.oracle(key)
            assert (rs[0].flags & 3, rs[0].nregions, rs[0].nenv) == (3, 2, 3), (alph, key, rs[0].flags, rs[0].nregions, rs[0].nenv)
            assert all((r.flags & 3) == 3 and r.nenv == r.nregions + 1 for r in rs), (alph, key, [(r.flags, r.nregions, r.nenv) for r in rs])
    many = inputs["dna"].oracle("many")
    assert all(r.nregions > WH_MAX_ENVELOPES and (r.flags & 2) and r.nenv > r.nregions for r in many), [(r.flags, r.nregions, r.nenv) for r in many]
    short = [inputs["dna"].oracle(k) for k in inputs["dna"].short_keys()[:40]]
    assert sum(1 for rs in short if rs[0].flags & 2) >= 20            # the short queries of the mixed call are multidomain mostly


def test_the_getter_is_declared_exported_and_bound():
    from witch_amd import _lib
    from witch_amd.ehmm import EHMM
    assert "wh_last_long_query_pairs" in _lib.SYMBOLS and hasattr(EHMM, "last_long_queries")
    header = open(os.path.join(ROOT, "include", "witch_hip.h")).read()
    assert "int wh_last_long_query_pairs(wh_ehmm *e, int64_t out[2]);" in header
    assert hasattr(_lib.lib(), "wh_last_long_query_pairs")


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("alph", ALPHABETS)
def test_long_queries_alone_equal_the_oracle(inputs, alph):
    """60 000 and 100 000 residues, seeds 0-3, on the two models: regions, envelopes and score are the oracle's, nothing is
    flagged, and the getter counts exactly the pairs with a multidomain region."""
    _need_gpu()
    from witch_amd.ehmm import pack_queries
    inp = inputs[alph]
    seqs = [inp.seq(k) for k in inp.long_keys]
    results = [inp.oracle(k) for k in inp.long_keys]
    e = inp.ehmm()
    res, offs = pack_queries(seqs)
    deci, flags, det = e.score(res, offs, want_detail=True)
    lq = e.last_long_queries()
    e.close()
    print(alph, "last_long_queries", lq)
    _check_against_oracle(inp.ohm, results, deci, flags, det, ("long queries", alph))
    assert lq == (_resolver_pairs(results), max(LENGTHS)), lq


@pytest.mark.gpu
@pytest.mark.parametrize("alph", ALPHABETS)
def test_short_pairs_beside_long_queries_keep_their_results(inputs, alph):
    """200 two-copy fragments of 150-600 residues and the long queries in one call: every pair equals the oracle, the short
    pairs come out as in a call of their own (they used to lose their second envelope), and the pass takes the long
    queries' pairs only."""
    _need_gpu()
    from witch_amd.ehmm import pack_queries
    inp = inputs[alph]
    skeys = inp.short_keys()
    lkeys = inp.long_keys[::2]
    short, longq = [inp.seq(k) for k in skeys], [inp.seq(k) for k in lkeys]
    results = [inp.oracle(k) for k in skeys + lkeys]
    e = inp.ehmm()
    r0, o0 = pack_queries(short)
    d0, f0, det0 = e.score(r0, o0, want_detail=True)
    assert e.last_long_queries() == (0, 0)
    x0 = np.ctypeslib.as_array(det0).copy()
    r1, o1 = pack_queries(short + longq)
    d1, f1, det1 = e.score(r1, o1, want_detail=True)
    lq = e.last_long_queries()
    e.close()
    print(alph, "last_long_queries", lq)
    _check_against_oracle(inp.ohm, results, d1, f1, det1, ("mixed call", alph))
    assert lq == (_resolver_pairs(results[len(skeys):]), max(len(s) for s in longq)), lq
    ns = len(short)
    assert np.array_equal(d1[:ns], d0) and np.array_equal(f1[:ns], f0)
    x1 = np.ctypeslib.as_array(det1)[:ns * len(inp.ohm)]
    for name in x0.dtype.names:
        a, b = x0[name], x1[name]
        if a.dtype.kind == "f":
            print(alph, name, "max |difference| of the short pairs' records", float(np.nanmax(np.abs(a.astype(np.float64) - b.astype(np.float64)))) if a.size else 0.0)
    assert x0.tobytes() == x1.tobytes(), [n for n in x0.dtype.names if x0[n].tobytes() != x1[n].tobytes()]
    assert any(d.nenv > d.nregions for d in det1[:ns * len(inp.ohm)])          # the case this test is about


@pytest.mark.gpu
def test_many_regions_in_a_long_query(inputs):
    """More than WH_MAX_ENVELOPES regions, one of them multidomain, in 60 000 residues: the long-list pass's own resolver round
    hands the pair to the long-query pass."""
    _need_gpu()
    from witch_amd.ehmm import pack_queries
    inp = inputs["dna"]
    results = [inp.oracle("many")]
    e = inp.ehmm()
    res, offs = pack_queries([inp.seq("many")])
    deci, flags, det = e.score(res, offs, want_detail=True)
    lq, n_ll = e.last_long_queries(), e.last_long_list_pairs()
    e.close()
    print("many regions", lq, n_ll)
    _check_against_oracle(inp.ohm, results, deci, flags, det, ("many regions in a long query",))
    assert n_ll >= 1 and lq[0] >= 1 and lq[1] == 60000, (n_ll, lq)


@pytest.mark.gpu
def test_a_big_region_in_a_long_query(orc, tmp_path):  # noqa: F811
    """A 40-copy tandem block (one region of more than 32 domains per trace) inside 60 000 residues of background: the
    long-query pass counts the region's lists like any launch and runs the pair again with longer ones."""
    _need_gpu()
    from tests.test_resolver_big_regions import _Family
    from witch_amd.ehmm import pack_queries
    fam = _Family(orc, str(tmp_path), "dna", 180, 60)
    rng = np.random.default_rng(5)
    seq = rng.integers(0, 4, size=60000).astype(np.uint8)
    block = fam.tandem(40)
    seq[20000:20000 + len(block)] = block
    results = [[h.score(seq) for h in fam.ohm]]
    assert all(r.nenv - (r.nregions - 1) > 32 for r in results[0]), [(r.nregions, r.nenv) for r in results[0]]
    e = fam.ehmm()
    res, offs = pack_queries([seq])
    deci, flags, det = e.score(res, offs, want_detail=True)
    lq, over = e.last_long_queries(), e.last_region_overflow()
    e.close()
    print("big region in a long query", lq, over)
    _check_against_oracle(fam.ohm, results, deci, flags, det, ("big region in a long query",))
    assert lq == (len(fam.ohm), 60000), lq
    assert over["pairs"] >= 1 and over["max_domains"] > 32, over


@pytest.mark.gpu
def test_nothing_moves_for_calls_that_fit(orc, tmp_path):  # noqa: F811
    """amino_multidomain, a 1 024 x 200 headline slice and the 6-28-copy tandem inputs: no pair goes through the pass, and the
    results do not depend on WH_NO_LONG_QUERY."""
    _need_gpu()
    import bench
    from tests.conftest import load_case
    from tests.test_resolver_big_regions import ROWS, _Family
    from witch_amd.ehmm import EHMM, pack_queries
    batches = []
    for key in ROWS:
        fam = _Family(orc, str(tmp_path / "tandem"), *key)
        batches.append((fam.ehmm(), [fam.tandem(c) for c in (6, 12, 20, 28)]))
    case = load_case("amino_multidomain")
    ea = EHMM(case.hmm_paths, hmm_index=case.hmm_index, nseq=case.nseq)
    batches.append((ea, [ea.digitize(s) for s in case.qseqs]))
    _, se, _, hseqs, _ = bench.make_workload("dna_100k_x200", str(tmp_path / "headline"), 1024, 200)
    batches.append((EHMM(se.paths, hmm_index=se.index, nseq=se.nseq), [s.astype(np.uint8) for s in hseqs]))
    for e, seqs in batches:
        res, offs = pack_queries(seqs)
        deci, flags, det = e.score(res, offs, want_detail=True)
        assert e.last_long_queries() == (0, 0), e.last_long_queries()
        e.set_option("WH_NO_LONG_QUERY", "1")
        deci0, flags0, det0 = e.score(res, offs, want_detail=True)
        e.set_option("WH_NO_LONG_QUERY", "")
        assert e.last_long_queries() == (0, 0)
        assert np.array_equal(deci, deci0) and np.array_equal(flags, flags0)
        assert np.ctypeslib.as_array(det).tobytes() == np.ctypeslib.as_array(det0).tobytes()
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("alph", ALPHABETS)
def test_without_the_pass_a_long_query_switches_the_resolver_off(inputs, alph):
    """WH_NO_LONG_QUERY keeps what a call did before the pass existed: no resolver for the whole call, so the multidomain region
    of every long pair stays one envelope - one short of the oracle - and nothing says so."""
    _need_gpu()
    from witch_amd.ehmm import pack_queries
    inp = inputs[alph]
    e = inp.ehmm()
    e.set_option("WH_NO_LONG_QUERY", "1")
    res, offs = pack_queries([inp.seq(k) for k in inp.long_keys])
    deci, flags, det = e.score(res, offs, want_detail=True)
    lq = e.last_long_queries()
    e.close()
    assert lq == (0, 0), lq
    H = len(inp.ohm)
    for q, key in enumerate(inp.long_keys):
        for h, r in enumerate(inp.oracle(key)):
            d = det[q * H + h]
            print(alph, key, h, "device", int(flags[q, h]), d.nregions, d.nenv, "oracle", r.flags, r.nregions, r.nenv)
            assert (r.flags & 2) and d.nregions == r.nregions and d.nenv == r.nenv - 1, (alph, key, h, d.nregions, d.nenv, r.nregions, r.nenv)
            assert not (flags[q, h] & 8)
