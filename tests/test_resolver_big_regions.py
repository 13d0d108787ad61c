"""Regions beyond the resolver's fixed lists: the big-region pass against the CPU oracle.

The resolver keeps 32 domains of a sampled trace, 8 192 sampled segments and 64 significant clusters of ONE multidomain
region in fixed lists (LDS and a small HBM block per wave).  hmmsearch has no such limit: a tandem repeat of 36 to 96
copies of a family fragment is one region with that many domains per trace.  Such a region is counted to the end, its
pair is listed, and the big-region pass scores it again inside the same call with every list in HBM
(include/witch_hip.h: wh_last_region_overflow).  The inputs are those of test_one_region_with_up_to_28_domains with more
copies; the oracle (realloc'ed lists, 256 envelopes per pair) is the reference; the tolerance is the project's boundary
rule for the multidomain class (tests/test_gpu_parity.py: _check_decibits with LONG_EPS)."""
import os

import numpy as np
import pytest

from tests.test_gpu_parity import LONG_EPS, _check_decibits, _need_gpu, orc  # noqa: F401  (orc: the oracle fixture)
from witch_amd._lib import WH_MAX_ENVELOPES

# (alphabet, root length, fragment length): copies -> (regions, envelopes) the oracle finds, on both models of the eHMM
ROWS = {
    ("dna", 180, 60): {36: (1, 36), 48: (1, 48), 72: (1, 72), 96: (1, 96)},
    ("amino", 700, 45): {40: (1, 37), 72: (1, 67)},
}


class _Family:
    def __init__(self, orc_mod, workdir, alph, root_len, flen):
        from witch_amd import synth
        self.alph = alph
        self.fam = synth.make_family(5200 + root_len, root_len, 16, alph, 0.03, 1e-4)
        self.eh = synth.make_ehmm(self.fam, 2, os.path.join(workdir, alph), witch_layout=False)
        _, self.frags = synth.make_queries(self.fam, 5, 14, flen)
        self.ohm = [orc_mod.OracleHMM(p) for p in self.eh.paths]
        self._scored = {}

    def tandem(self, copies):
        return np.concatenate([self.frags[c % len(self.frags)].astype(np.uint8) for c in range(copies)])

    def oracle(self, key, seq):
        """The oracle's results of <seq> on every model, computed once per module."""
        if key not in self._scored:
            self._scored[key] = [h.score(seq) for h in self.ohm]
        return self._scored[key]

    def ehmm(self):
        from witch_amd.ehmm import EHMM
        return EHMM(self.eh.paths, hmm_index=self.eh.index, nseq=self.eh.nseq)


@pytest.fixture(scope="module")
def families(orc, tmp_path_factory):  # noqa: F811
    work = str(tmp_path_factory.mktemp("big_regions"))
    return {key: _Family(orc, work, *key) for key in ROWS}


def _check_against_oracle(fam, keys, seqs, deci, flags, det, ctx):
    """The five checks of every pair: no WH_FLAG_TRUNC, the oracle's reported / multidomain bits, deci-bits under the
    boundary rule, every region counted, the first WH_MAX_ENVELOPES envelopes listed."""
    H = len(fam.ohm)
    od = np.zeros((len(seqs), H), dtype=np.int32)
    of = np.zeros((len(seqs), H), dtype=np.uint8)
    osc = np.zeros((len(seqs), H), dtype=np.float32)
    for q, (key, s) in enumerate(zip(keys, seqs)):
        for h, r in enumerate(fam.oracle(key, s)):
            od[q, h], of[q, h], osc[q, h] = r.decibits, r.flags & 0xFF, r.seq_score
            d = det[q * H + h]
            print(ctx, key, h, "device", int(deci[q, h]), int(flags[q, h]), d.nregions, d.nenv, "oracle", r.decibits, r.flags, r.nregions, r.nenv)
    assert (flags & 8).sum() == 0, ("WH_FLAG_TRUNC", ctx, flags)
    assert np.array_equal(flags & 3, of & 3), (ctx, flags, of)
    _check_decibits(deci, od, osc, (of & 1) == 1, ctx, LONG_EPS)
    for q, (key, s) in enumerate(zip(keys, seqs)):
        for h, r in enumerate(fam.oracle(key, s)):
            d = det[q * H + h]
            assert d.nregions == r.nregions, (ctx, key, h, d.nregions, r.nregions)
            assert d.nenv == min(r.nenv, WH_MAX_ENVELOPES), (ctx, key, h, d.nenv, r.nenv)


def _mixed_regions_query(fam):
    """More than WH_MAX_ENVELOPES regions AND one region beyond the resolver's lists: 20 separated fragment copies, then a
    40-copy tandem block (the long-list pass feeds the big-region pass)."""
    rng = np.random.default_rng(4078)
    parts = []
    for c in range(20):
        parts.append(fam.frags[c % len(fam.frags)].astype(np.uint8))
        parts.append(rng.integers(0, 4, size=int(rng.integers(60, 90))).astype(np.uint8))
    parts.append(fam.tandem(40))
    return np.concatenate(parts)


# ------------------------------------------------------------------------------------------------ CPU
def test_oracle_counts_of_the_tandem_inputs(families):
    """Guards the inputs, not the feature: the oracle finds ONE region and the envelope counts of the issue's table, on both
    models, and every row has more domains than the resolver's LDS list (32), the long DNA rows more than 64."""
    for key, rows in ROWS.items():
        fam = families[key]
        for copies, (nreg, nenv) in rows.items():
            for r in fam.oracle(copies, fam.tandem(copies)):
                assert (r.nregions, r.nenv) == (nreg, nenv), (key, copies, r.nregions, r.nenv)
                assert r.nenv > 32 and (r.flags & 2)
    dna = families[("dna", 180, 60)]
    assert any(r.nregions == 1 and r.nenv > 64 for c in ROWS[dna_key()] for r in dna.oracle(c, dna.tandem(c)))
    mixed = dna.oracle("mixed", _mixed_regions_query(dna))
    assert all(r.nregions > WH_MAX_ENVELOPES and r.nenv - (r.nregions - 1) > 32 for r in mixed), [(r.nregions, r.nenv) for r in mixed]


def dna_key():
    return ("dna", 180, 60)


def test_the_getter_is_declared_and_bound():
    from witch_amd import _lib
    from witch_amd.ehmm import EHMM
    assert "wh_last_region_overflow" in _lib.SYMBOLS and hasattr(EHMM, "last_region_overflow")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "witch_hip.h")).read()
    assert "int wh_last_region_overflow(wh_ehmm *e, int64_t *out4);" in header


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_regions_beyond_the_resolvers_lists_equal_the_oracle(families):
    """36 to 96 tandem copies (DNA) and 40 / 72 (protein): one region, more than 32 domains per trace, and from 72 copies on
    more than 8 192 segments and more than 64 clusters.  Every pair equals the oracle."""
    _need_gpu()
    from witch_amd.ehmm import pack_queries
    for key, rows in ROWS.items():
        fam = families[key]
        copies = list(rows)
        seqs = [fam.tandem(c) for c in copies]
        orc_rows = [r for c, s in zip(copies, seqs) for r in fam.oracle(c, s)]
        assert any(r.nenv > 32 for r in orc_rows)                                 # the case this test is about
        if key[0] == "dna":
            assert any(r.nregions == 1 and r.nenv > 64 for r in orc_rows)
        e = fam.ehmm()
        res, offs = pack_queries(seqs)
        deci, flags, det = e.score(res, offs, want_detail=True)
        over = e.last_region_overflow()
        print(key, over)
        _check_against_oracle(fam, copies, seqs, deci, flags, det, ("big regions", key[0]))
        assert over["pairs"] >= 1 and over["max_domains"] > 32, over
        if key[0] == "dna":
            assert over["max_segments"] > 8192 and over["max_clusters"] > 64, over
        assert e.last_long_list_pairs() == 0                                      # one region each: not the long-list pass's pairs
        # without the pass the same pairs come back flagged (what the pass is for)
        e.set_option("WH_NO_BIG_REGION", "1")
        _, flags0, _ = e.score(res, offs, want_detail=True)
        e.set_option("WH_NO_BIG_REGION", "")
        assert (flags0 & 8).any() and e.last_region_overflow()["pairs"] == 0
        e.close()


@pytest.mark.gpu
def test_no_cost_and_no_change_where_nothing_overflows(families, tmp_path):
    """6 to 28 copies, amino_multidomain and a 1 024 x 200 headline slice: the pass finds nothing and, switched off, changes
    nothing.  A mixed batch: 300 ordinary queries score bitwise the same with and without the 96-copy query beside them."""
    _need_gpu()
    import bench
    from tests.conftest import load_case
    from witch_amd.ehmm import EHMM, pack_queries
    zero = {"pairs": 0, "max_domains": 0, "max_segments": 0, "max_clusters": 0}
    batches = []
    for key in ROWS:
        fam = families[key]
        batches.append((fam.ehmm(), [fam.tandem(c) for c in (6, 12, 20, 28)]))
    case = load_case("amino_multidomain")
    ea = EHMM(case.hmm_paths, hmm_index=case.hmm_index, nseq=case.nseq)
    batches.append((ea, [ea.digitize(s) for s in case.qseqs]))
    _, se, _, hseqs, _ = bench.make_workload("dna_100k_x200", str(tmp_path / "headline"), 1024, 200)
    hseqs = [s.astype(np.uint8) for s in hseqs]
    batches.append((EHMM(se.paths, hmm_index=se.index, nseq=se.nseq), hseqs))
    for e, seqs in batches:
        res, offs = pack_queries(seqs)
        deci, flags = e.score(res, offs)
        assert e.last_region_overflow() == zero, e.last_region_overflow()
        e.set_option("WH_NO_BIG_REGION", "1")
        deci0, flags0 = e.score(res, offs)
        e.set_option("WH_NO_BIG_REGION", "")
        assert np.array_equal(deci, deci0) and np.array_equal(flags, flags0)
        e.close()
    # the mixed batch: the tandem family's two models and twenty headline models
    dna = families[dna_key()]
    em = EHMM(list(dna.eh.paths) + list(se.paths[:20]), hmm_index=list(range(22)), nseq=list(dna.eh.nseq) + list(se.nseq[:20]))
    r0, o0 = pack_queries(hseqs[:300])
    d0, f0 = em.score(r0, o0)
    assert em.last_region_overflow() == zero
    r1, o1 = pack_queries(hseqs[:300] + [dna.tandem(96)])
    d1, f1 = em.score(r1, o1)
    assert em.last_region_overflow()["pairs"] >= 1
    assert (f1 & 8).sum() == 0
    assert np.array_equal(d1[:300], d0) and np.array_equal(f1[:300], f0)
    em.close()


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["force_wide_4", "score_kernel_11", "long_list"])
def test_other_routes_into_the_resolver_queue(families, route):
    """The 48-copy DNA query through the several-waves-per-pair kernels and a staged schedule, and a query with more than
    WH_MAX_ENVELOPES regions whose last region is a 40-copy tandem block (long-list pass -> big-region pass)."""
    _need_gpu()
    from witch_amd.ehmm import pack_queries
    fam = families[dna_key()]
    key, seq = (48, fam.tandem(48)) if route != "long_list" else ("mixed", _mixed_regions_query(fam))
    old = os.environ.get("WH_FORCE_WIDE")
    if route == "force_wide_4":
        os.environ["WH_FORCE_WIDE"] = "4"          # (read at load)
    try:
        e = fam.ehmm()
    finally:
        if route == "force_wide_4":
            if old is None:
                os.environ.pop("WH_FORCE_WIDE", None)
            else:
                os.environ["WH_FORCE_WIDE"] = old
    if route == "score_kernel_11":
        e.set_option("WH_SCORE_KERNEL", "11")
    res, offs = pack_queries([seq])
    deci, flags, det = e.score(res, offs, want_detail=True)
    over = e.last_region_overflow()
    n_long = e.last_long_list_pairs()
    e.close()
    _check_against_oracle(fam, [key], [seq], deci, flags, det, ("big regions", route))
    assert over["pairs"] >= 1 and over["max_domains"] > 32, over
    assert n_long == (len(fam.ohm) if route == "long_list" else 0), n_long
