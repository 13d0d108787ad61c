"""Queries longer than a scoring or alignment class can plan in LDS: the long-query scoring and alignment passes.

The scoring and alignment launches keep the query in a wave's LDS block.  A call whose longest query a size class cannot plan
used to be refused (WH_ERANGE, "query length ... does not fit in LDS").  Now the launches are sized for the main length cap
Lmain (witch_amd/csrc/wh_plan.h: the largest length every class accepts), they leave the pairs of longer queries alone, and
those pairs are scored by the float64 front end in its pair-list mode plus the resolver, and aligned by the float64 any-size
alignment kernel (include/witch_hip.h: wh_last_long_score_pairs, wh_last_long_align_pairs).  WH_SCORE_LMAIN=<n> forces the
cap, so the routing is tested with the golden cases' queries of up to ~110 residues; one test uses a query that is
genuinely over the cap.  The oracle is the checker; helpers and tolerances are those of tests/test_gpu_parity.py.

Main length cap by cells per lane Q, scoring / alignment (tools/plan_check.cpp): DNA 142 368 / 142 816 (Q=4), 121 888,
101 408, 80 928 (Q=16), 30 124 (Q=20, pass-synchronous from here), 28 076 ... 15 788 (Q=48).  Protein 125 984 (Q=4), 89 120,
52 256, 32 172 (Q=16), 30 124 (Q=20), 28 076 ... 15 788 (Q=48).  A 16-cell protein class keeps 92 KB of tables beside ONE
wave's residues (15 392 of them): with that alone its cap was HALF the 20-cell class's, so the planner now sends a 16-cell
class whose query leaves no wave beside the tables to the pass-synchronous kernels, as it sends the 20-cell protein
classes - queries that were refused before, nothing that ran."""
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import CASES, load_case
from tests.test_gpu_parity import BOUNDARY_EPS, LONG_EPS, _near_boundary_eps, _need_gpu, orc  # noqa: F401  (orc: the oracle fixture)
from witch_amd._lib import WH_MAX_ENVELOPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "witch_amd", "csrc")
LDS_BUDGET = 160 * 1024 - 512            # witch_amd/csrc/wh_plan.h: kLdsBudget
ALPH = {"dna": 0, "rna": 1, "amino": 2}
ROUTING_CASES = ("dna_synth", "amino_hmmbuild")


def _model_nodes(paths):
    out = []
    for p in paths:
        for line in open(p):
            if line.startswith("LENG"):
                out.append(int(line.split()[1]))
                break
    return out


def _cap_of(alphabet, nodes):
    from witch_amd._lib import lib
    m = np.ascontiguousarray(nodes, dtype=np.int32)
    return lib().wh_query_len_cap(ALPH[alphabet], m.ctypes.data, len(m))


# ------------------------------------------------------------------------------------------------ CPU
def test_new_symbols_are_declared_exported_and_bound():
    """The table of tests/test_abi_host.py, extended: header, export list, ctypes table, Python methods."""
    from witch_amd import _lib
    from witch_amd.ehmm import EHMM
    from witch_amd.gcmm.engine import QueryAlignmentEngine
    header = open(os.path.join(ROOT, "include", "witch_hip.h")).read()
    for decl, name in (("int wh_last_long_score_pairs(wh_ehmm *e, int64_t out[2]);", "wh_last_long_score_pairs"),
                       ("int wh_last_long_align_pairs(wh_ehmm *e, int64_t out[2]);", "wh_last_long_align_pairs"),
                       ("int      wh_query_len_cap(int alphabet, const int32_t *model_nodes, int n);", "wh_query_len_cap")):
        assert decl in header, decl
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name), name
    assert hasattr(EHMM, "last_long_score") and hasattr(EHMM, "last_long_align") and hasattr(EHMM, "max_query_len")
    assert QueryAlignmentEngine().long_score_pairs == 0
    for knob in ("WH_SCORE_LMAIN", "WH_NO_LONG_SCORE", "WH_LONGQ_FORCE"):
        assert knob in header and knob in open(os.path.join(CSRC, "wh_knobs.h")).read(), knob      # (the knobs' one table)


@pytest.mark.parametrize("name", CASES)
def test_query_len_cap_is_sane_for_every_golden_case(name):
    """Positive, no wrapped size_t, and at most the analytic bound: a wave's residue buffer holds a byte per residue, so the cap
    of a class is below what the SMALLEST tables any kernel family keeps for it leave of the LDS budget - beside both
    transition orientations and the emission rows one wave for up to 24 cells per lane, beside one orientation four waves
    (the pass-synchronous kernel) from 20 cells per lane on."""
    case = load_case(name)
    nodes = _model_nodes(case.hmm_paths)
    assert len(nodes) == len(case.hmm_paths)
    K = 20 if case.alphabet == "amino" else 4
    bound = LDS_BUDGET
    for m in nodes:
        q = 4 * (-(-m // 256))           # cells per lane: 64 lanes, in steps of four; beyond 48: no one-wave class
        if q > 48:
            continue                     # (the several-wave and float64 kernels: their caps are far above the one-wave classes')
        one_wave = LDS_BUDGET - 16 - (K + 16) * q * 64 * 4 if q <= 24 else 0
        four_waves = (LDS_BUDGET - 16 - 8 * q * 64 * 4) // 4 if q >= 20 else 0
        bound = min(bound, max(one_wave, four_waves))
    cap = _cap_of(case.alphabet, nodes)
    print(name, "nodes", nodes[:8], "cap", cap, "bound", bound)
    assert 0 < cap <= bound < 1 << 20, (name, cap, bound)
    for sub in ([min(nodes)], [max(nodes)]):
        assert 0 < _cap_of(case.alphabet, sub) < 1 << 20
    assert _cap_of(case.alphabet, [max(nodes)]) == cap          # the largest class decides here (see the module docstring)


@pytest.fixture(scope="module")
def plan_table(tmp_path_factory):
    """tools/plan_check.cpp, compiled with the address and undefined-behaviour sanitizers and run as a program of its own (no GPU,
    nothing loaded into Python): its own checks pass, and its table of caps per alphabet and class."""
    from witch_amd import _lib
    _lib.lib()
    exe = str(tmp_path_factory.mktemp("plan") / "plan_check")
    cxx = next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++", "/usr/bin/g++") if os.path.exists(c)), "c++")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
           os.path.join(ROOT, "tools", "plan_check.cpp"), _lib.LIB_PATH, "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH),
           "-Wl,--allow-shlib-undefined", "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "plan_check: ok" in r.stdout, r.stdout[-3000:]
    table = {}
    for line in r.stdout.splitlines():
        f = dict(x.split("=") for x in line.split()[1:]) if line.startswith("cap ") else {}
        if "Q" in f:
            table[(int(f["K"]), int(f["Q"]))] = (int(f["score"]), int(f["align"]))
    assert len(table) == 24
    return table


def test_planner_runs_clean_under_the_sanitizers(plan_table):
    for (K, Q), (s, a) in plan_table.items():
        assert 0 < s < LDS_BUDGET and 0 < a < LDS_BUDGET, (K, Q, s, a)


@pytest.mark.parametrize("alph", ["dna", "amino"])
def test_main_length_cap_is_monotone_in_the_model_class(plan_table, alph):
    """The cap does not grow with the cells per lane of the class, for either alphabet."""
    K = 20 if alph == "amino" else 4
    caps = [plan_table[(K, Q)] for Q in range(4, 49, 4)]
    print(alph, caps)
    for (s0, a0), (s1, a1) in zip(caps, caps[1:]):
        assert s1 <= s0 and a1 <= a0, (alph, caps)


# ------------------------------------------------------------------------------------------------ GPU
class _Ref:
    """A set of models and queries with the oracle's result of every pair and alignment, computed once."""

    def __init__(self, orc_mod, paths, index, nseq, seqs, align_models=2):
        self.paths, self.index, self.nseq, self.seqs = list(paths), list(index), list(nseq), seqs
        self.ohm = [orc_mod.OracleHMM(p) for p in paths]
        self.H = len(paths)
        self.res = [[h.score(s) for h in self.ohm] for s in seqs]
        self.pq = [q for q in range(len(seqs)) for _ in range(min(align_models, self.H))]
        self.ph = [h for _ in range(len(seqs)) for h in range(min(align_models, self.H))]
        self.cols = [self.ohm[h].align(seqs[q]) for q, h in zip(self.pq, self.ph)]

    def ehmm(self):
        from witch_amd.ehmm import EHMM
        return EHMM(self.paths, hmm_index=self.index, nseq=self.nseq)

    def run(self, e, sel=None):
        """score (with Forward and detail) and align the queries <sel> (all): a dict of everything that comes back"""
        from witch_amd.ehmm import pack_queries
        sel = list(range(len(self.seqs))) if sel is None else list(sel)
        res, offs = pack_queries([self.seqs[q] for q in sel])
        deci, flags, fwd, det = e.score(res, offs, want_fwd=True, want_detail=True)
        out = {"sel": sel, "deci": deci, "flags": flags, "fwd": fwd, "det": np.ctypeslib.as_array(det).copy(), "long_score": e.last_long_score()}
        pos = {q: t for t, q in enumerate(sel)}
        keep = [t for t, q in enumerate(self.pq) if q in pos]
        out["pairs"] = keep
        out["cols"], out["co"] = e.align(res, offs, [pos[self.pq[t]] for t in keep], [self.ph[t] for t in keep])
        out["long_align"] = e.last_long_align()
        return out

    def check(self, out, ctx):
        """tests/test_gpu_parity.py test_score_against_oracle_and_golden's comparisons, pair by pair: Forward log-odds, flags,
        regions, envelopes, deci-bits under the boundary rule; and the aligned columns."""
        for t, q in enumerate(out["sel"]):
            for h in range(self.H):
                r, d = self.res[q][h], out["det"][t * self.H + h]
                where = (ctx, q, h)
                if np.isfinite(r.fwd_bits):
                    tol = max(1e-4, 2.0 * float(np.spacing(np.float32(abs(r.fwd_bits)))))
                    assert abs(float(out["fwd"][t, h]) - r.fwd_bits) <= tol, (where, float(out["fwd"][t, h]), r.fwd_bits)
                    assert abs(float(d["fwd_bits"]) - r.fwd_bits) <= tol, (where, float(d["fwd_bits"]), r.fwd_bits)
                assert int(out["flags"][t, h]) & 7 == r.flags & 7, (where, int(out["flags"][t, h]), r.flags)
                assert not int(out["flags"][t, h]) & 8, where
                assert d["nregions"] == r.nregions and d["nenv"] == min(r.nenv, WH_MAX_ENVELOPES), (where, d["nregions"], d["nenv"], r.nregions, r.nenv)
                for v in range(d["nenv"]):
                    assert (d["env_i"][v], d["env_j"][v]) == (r.env_i[v], r.env_j[v]), (where, v)
                    assert abs(d["envsc"][v] - r.envsc[v]) <= 2e-4 * max(1.0, abs(r.envsc[v]) / 50), (where, d["envsc"][v], r.envsc[v])
                    len_t = max(1.0, (r.env_j[v] - r.env_i[v] + 1) / 250.0)
                    assert abs(d["domcorr"][v] - r.domcorr[v]) <= (2e-2 if r.env_multi[v] else 1e-3 * len_t), (where, d["domcorr"][v], r.domcorr[v])
                self.check_decibits(q, h, out["deci"][t, h], where)
        for u, t in enumerate(out["pairs"]):
            got = out["cols"][out["co"][u]:out["co"][u + 1]]
            assert np.array_equal(got, self.cols[t]), (ctx, "alignment", self.pq[t], self.ph[t])

    def check_decibits(self, q, h, got, where):
        """the boundary rule of tests/test_gpu_parity.py: the oracle's deci-bits, or one unit off with its float score at a rounding boundary"""
        r = self.res[q][h]
        if r.flags & 1 and int(got) != r.decibits:
            assert abs(int(got) - r.decibits) == 1, (where, int(got), r.decibits)
            assert _near_boundary_eps(r.seq_score, LONG_EPS if r.flags & 2 else BOUNDARY_EPS), (where, r.seq_score)

    def check_scores(self, q, deci, flags, fwd, ctx):
        """one query's row of a call without the per-pair detail: Forward log-odds, flags and deci-bits against the oracle, as check does"""
        for h in range(self.H):
            r, where = self.res[q][h], (ctx, q, h)
            if np.isfinite(r.fwd_bits):
                tol = max(1e-4, 2.0 * float(np.spacing(np.float32(abs(r.fwd_bits)))))
                assert abs(float(fwd[h]) - r.fwd_bits) <= tol, (where, float(fwd[h]), r.fwd_bits)
            assert int(flags[h]) & 7 == r.flags & 7 and not int(flags[h]) & 8, (where, int(flags[h]), r.flags)
            self.check_decibits(q, h, deci[h], where)

    def expect_counts(self, out, lmain, ctx):
        """the getters against the count made here"""
        lens = [len(self.seqs[q]) for q in out["sel"]]
        long_q = [n for n in lens if n > lmain]
        want = (len(long_q) * self.H, max(long_q)) if long_q else (0, 0)
        assert out["long_score"] == want, (ctx, out["long_score"], want)
        n_al = sum(1 for t in out["pairs"] if len(self.seqs[self.pq[t]]) > lmain)
        assert out["long_align"] == ((n_al, max(long_q)) if n_al else (0, 0)), (ctx, out["long_align"], n_al)


def _same_short(ref, a, b, lmain, ctx):
    """the pairs of the queries of up to <lmain> residues: bitwise what the other run gave"""
    rows = [t for t, q in enumerate(a["sel"]) if len(ref.seqs[q]) <= lmain]
    assert a["sel"] == b["sel"] and rows
    for name in ("deci", "flags", "fwd"):
        assert a[name][rows].tobytes() == b[name][rows].tobytes(), (ctx, name)
    drows = [t * ref.H + h for t in rows for h in range(ref.H)]
    assert a["det"][drows].tobytes() == b["det"][drows].tobytes(), (ctx, "detail")
    for u, t in enumerate(a["pairs"]):
        if len(ref.seqs[ref.pq[t]]) <= lmain:
            assert np.array_equal(a["cols"][a["co"][u]:a["co"][u + 1]], b["cols"][b["co"][u]:b["co"][u + 1]]), (ctx, "cols", t)


def _third_long(seqs):
    """a length with about a third of the queries beyond it: of the lengths that leave at least a quarter of them long (many
    golden queries share one length), the one that leaves the fewest"""
    lens = sorted(len(s) for s in seqs)
    ok = [n for n in sorted(set(lens)) if sum(1 for x in lens if x > n) * 4 >= len(lens)]
    return ok[-1]


_refs = {}


def _golden_ref(orc_mod, name):
    if name not in _refs:
        from witch_amd import _lib
        case = load_case(name)
        _lib.lib()
        seqs = []
        for s in case.qseqs:
            text = np.empty(len(s), dtype=np.uint8)
            assert _lib.lib().wh_digitize(ALPH[case.alphabet], s.encode(), len(s), text.ctypes.data) == 0
            seqs.append(text)
        _refs[name] = _Ref(orc_mod, case.hmm_paths, case.hmm_index, case.nseq, seqs)
    return _refs[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ROUTING_CASES)
def test_routing_at_small_shapes(orc, name):  # noqa: F811
    """About a third of the golden queries made "long" by WH_SCORE_LMAIN: every pair and every alignment equals the oracle, the
    short queries' outputs are bitwise those of a run without the knob, the getters count what the host counts - and the same
    with the residues-in-HBM kernels forced (WH_LONGQ_FORCE), whose results are identical to the LDS-residue run."""
    _need_gpu()
    ref = _golden_ref(orc, name)
    lmain = _third_long(ref.seqs)
    e = ref.ehmm()
    base = ref.run(e)
    assert base["long_score"] == (0, 0) and base["long_align"] == (0, 0)
    ref.check(base, (name, "no knob"))
    e.set_option("WH_SCORE_LMAIN", str(lmain))
    out = ref.run(e)
    print(name, "Lmain", lmain, "long_score", out["long_score"], "long_align", out["long_align"])
    ref.check(out, (name, "Lmain", lmain))
    ref.expect_counts(out, lmain, name)
    assert out["long_score"][0] >= ref.H * (len(ref.seqs) // 4)
    _same_short(ref, out, base, lmain, name)
    e.set_option("WH_LONGQ_FORCE", "1")
    hbm = ref.run(e)
    e.close()
    ref.check(hbm, (name, "residues in HBM"))
    for key in ("deci", "flags", "fwd", "det", "cols"):
        assert hbm[key].tobytes() == out[key].tobytes(), (name, "residues in HBM", key)
    assert hbm["long_score"] == out["long_score"] and hbm["long_align"] == out["long_align"]


@pytest.mark.gpu
def test_routing_edge_cases(orc):  # noqa: F811
    """A query of exactly Lmain stays on the main launch and one of Lmain + 1 goes to the pass; a call whose every query is
    long; a call with none long, which makes no launch more than without the knob; an empty query next to a long one; and
    WH_NO_LONG_SCORE, under which the knob does nothing."""
    _need_gpu()
    ref = _golden_ref(orc, "dna_synth")
    lens = sorted(set(len(s) for s in ref.seqs))
    lmain = next(n for n in lens if n + 1 in lens)            # both lengths occur among the golden queries
    e = ref.ehmm()
    e.set_timing(True)
    base = ref.run(e)
    n_launches = len(e.last_score_launches())
    e.set_option("WH_SCORE_LMAIN", str(lmain))
    out = ref.run(e)
    ref.check(out, ("edge", lmain))
    ref.expect_counts(out, lmain, "edge")
    assert any(len(s) == lmain for s in ref.seqs) and any(len(s) == lmain + 1 for s in ref.seqs)
    _same_short(ref, out, base, lmain, "edge")
    # every query long
    longest = [q for q in range(len(ref.seqs)) if len(ref.seqs[q]) > lmain]
    out = ref.run(e, longest)
    ref.check(out, ("every query long",))
    assert out["long_score"][0] == len(longest) * ref.H
    # none long: the cap is the call's own longest query, nothing is launched or read back for the pass
    e.set_option("WH_SCORE_LMAIN", str(max(lens)))
    out = ref.run(e)
    assert out["long_score"] == (0, 0) and out["long_align"] == (0, 0)
    assert len(e.last_score_launches()) == n_launches
    for key in ("deci", "flags", "fwd", "det", "cols"):
        assert out[key].tobytes() == base[key].tobytes(), key
    # an empty query next to a long one
    e.set_option("WH_SCORE_LMAIN", str(lmain))
    from witch_amd.ehmm import pack_queries
    q_long = longest[0]
    res, offs = pack_queries([np.zeros(0, dtype=np.uint8), ref.seqs[q_long]])
    deci, flags, fwd = e.score(res, offs, want_fwd=True)
    assert e.last_long_score() == (ref.H, len(ref.seqs[q_long]))
    assert not deci[0].any() and not flags[0].any() and np.all(np.isneginf(fwd[0]))
    ref.check_scores(q_long, deci[1], flags[1], fwd[1], "beside an empty query")
    cols, co = e.align(res, offs, [0, 1], [0, 0])
    assert co[1] == 0 and np.array_equal(cols, ref.ohm[0].align(ref.seqs[q_long]))
    # under WH_NO_LONG_SCORE there is no pass and the forced cap is ignored (the refusal itself: the over-the-cap test below)
    e.set_option("WH_NO_LONG_SCORE", "1")
    out = ref.run(e)
    e.close()
    assert out["long_score"] == (0, 0) and out["long_align"] == (0, 0)
    assert out["deci"].tobytes() == base["deci"].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["pass-synchronous", "wide"])
def test_each_kernel_family_skips_long_queries(orc, family, tmp_path):  # noqa: F811
    """The same knob run on a handle that takes the pass-synchronous kernels (a protein class of 20 cells per lane) and on one
    that takes the several-waves-per-pair kernels (WH_FORCE_WIDE=4): both leave a query beyond the cap to the pass."""
    _need_gpu()
    old = os.environ.get("WH_FORCE_WIDE")
    try:
        if family == "wide":
            os.environ["WH_FORCE_WIDE"] = "4"
            ref = _golden_ref(orc, "dna_synth")
        else:
            from witch_amd import synth
            fam = synth.make_family(77, 1250, 16, "amino", 0.03, 1e-4)
            eh = synth.make_ehmm(fam, 2, str(tmp_path), witch_layout=False)
            _, seqs = synth.make_queries(fam, 5, 8, (60, 400))
            ref = _Ref(orc, eh.paths, eh.index, eh.nseq, [s.astype(np.uint8) for s in seqs], align_models=1)
        e = ref.ehmm()
        if family != "wide":
            assert 1216 < int(e.M.max()) <= 1280          # 20 cells per lane
        lmain = _third_long(ref.seqs)
        base = ref.run(e)
        e.set_option("WH_SCORE_LMAIN", str(lmain))
        out = ref.run(e)
        e.close()
    finally:
        if old is None:
            os.environ.pop("WH_FORCE_WIDE", None)
        else:
            os.environ["WH_FORCE_WIDE"] = old
    print(family, "Lmain", lmain, out["long_score"], out["long_align"])
    ref.check(out, (family, lmain))
    ref.expect_counts(out, lmain, family)
    assert out["long_score"][0] > 0
    _same_short(ref, out, base, lmain, family)


@pytest.mark.gpu
def test_a_query_over_the_cap_is_scored_and_aligned(orc):  # noqa: F811
    """The call that used to fail with WH_ERANGE.  The golden case with the smallest cap is example_ehmm; on its shortest model
    (1 286 nodes, 24 cells per lane) wh_ehmm_max_query_len is 28 076.  A query of 1.1 x that - the golden queries back to back,
    then random residues, seed 1 - scored and aligned alone and beside eight short queries: score, flags, regions, envelopes
    and aligned columns are the oracle's.  (One model: the oracle needs seconds per model at this size.)"""
    _need_gpu()
    case = load_case("example_ehmm")
    nodes = _model_nodes(case.hmm_paths)
    h0 = int(np.argmin(nodes))
    from witch_amd.ehmm import EHMM
    e = EHMM([case.hmm_paths[h0]], hmm_index=[case.hmm_index[h0]], nseq=[case.nseq[h0]])
    cap = e.max_query_len()
    assert cap == _cap_of("dna", [nodes[h0]]) and 20000 < cap < 40000, cap
    L = int(1.1 * cap)
    short = [e.digitize(s) for s in case.qseqs[:8]]
    rng = np.random.default_rng(1)
    cat = np.concatenate([e.digitize(s) for s in case.qseqs])[:L // 2]
    longq = np.concatenate([cat, rng.integers(0, 4, size=L - len(cat)).astype(np.uint8)])
    ref = _Ref(orc, [case.hmm_paths[h0]], [case.hmm_index[h0]], [case.nseq[h0]], short + [longq], align_models=1)
    e.set_timing(True)
    alone = ref.run(e, [8])
    ms = e.last_kernel_ms(4)[0]
    both = ref.run(e)
    # WH_NO_LONG_SCORE restores the refusal: the same call is WH_ERANGE again, for scoring and for alignment
    from witch_amd._lib import WitchHipError, WH_ERANGE
    from witch_amd.ehmm import pack_queries
    e.set_option("WH_NO_LONG_SCORE", "1")
    res, offs = pack_queries([longq])
    for call in (lambda: e.score(res, offs), lambda: e.align(res, offs, [0], [0])):
        with pytest.raises(WitchHipError) as refused:
            call()
        assert "(%d)" % WH_ERANGE in str(refused.value) and "does not fit in LDS" in str(refused.value), str(refused.value)
    e.close()
    print("cap", cap, "L", L, "oracle", ref.res[8][0].decibits, ref.res[8][0].flags, ref.res[8][0].nregions, ref.res[8][0].nenv, "device", int(alone["deci"][0, 0]), "long_score", alone["long_score"])
    ref.check(alone, ("over the cap, alone", L))
    ref.check(both, ("over the cap, beside short queries", L))
    assert alone["long_score"] == (1, L) and both["long_score"] == (1, L)
    assert alone["long_align"] == (1, L) and both["long_align"] == (1, L)
    assert ref.res[8][0].flags & 1
    print("resolver-stage timer of the call with the long query alone (long-query scoring pass included): %.1f ms" % ms)


@pytest.mark.gpu
def test_a_16_cell_protein_class_takes_the_pass_synchronous_kernels_beyond_one_wave(orc, tmp_path):  # noqa: F811
    """A protein model of 16 cells per lane keeps 92 KB of tables in LDS; beyond 15 392 residues not one wave's block fits beside
    them.  Such a query now runs on the pass-synchronous scoring and alignment kernels (as 20-cell protein models do), so the
    class accepts what the next larger one accepts: 16 500 residues - the family's fragments back to back, then random
    residues - are scored and aligned by the main launches (no pair for the long-query passes) and equal the oracle."""
    _need_gpu()
    from witch_amd import synth
    fam = synth.make_family(78, 950, 16, "amino", 0.03, 1e-4)
    eh = synth.make_ehmm(fam, 1, str(tmp_path), witch_layout=False)
    _, seqs = synth.make_queries(fam, 5, 6, (200, 600))
    seqs = [s.astype(np.uint8) for s in seqs]
    rng = np.random.default_rng(2)
    cat = np.concatenate(seqs)
    longq = np.concatenate([cat, rng.integers(0, 20, size=16500 - len(cat)).astype(np.uint8)])
    ref = _Ref(orc, eh.paths, eh.index, eh.nseq, seqs[:3] + [longq], align_models=1)
    e = ref.ehmm()
    assert 768 < int(e.M.max()) <= 1024 and 30124 <= e.max_query_len() <= 32172, (e.M, e.max_query_len())
    out = ref.run(e)
    e.close()
    ref.check(out, ("16 cells per lane, 16 500 residues",))
    assert out["long_score"] == (0, 0) and out["long_align"] == (0, 0)


E2E_LONG_QUERIES = 24          # of the 500 fragments of example_e2e: the longest ones, 360 pairs for the long-query scoring pass


@pytest.mark.gpu
def test_engine_run_with_long_queries_writes_the_same_merged_files(tmp_path, monkeypatch):
    """QueryAlignmentEngine.run on the end-to-end example with WH_SCORE_LMAIN in the environment, set so that the 24 longest of
    the 500 fragments go to the long-query scoring and alignment passes: the two merged files have the sha256 of the run
    without the knob, which are the reference pipeline's.  Against HMMER's own search table the run with the knob stays within
    what test_end_to_end_example_against_the_reference_pipeline allows (3 reported-mask differences, 2 scores one deci-bit
    off), and outside the long queries' rows its scores and flags are bitwise those of the run without it.
    Confirmed on the CPU beforehand with the oracle: Lmain is 351 (fragments of 79 to 430 residues, median 257), and on the 360
    pairs of the 24 longer fragments the float64 oracle has HMMER's reported set and HMMER's printed score for every pair (0
    mask differences, 0 scores off) - the pass, which computes what the oracle computes, cannot use up the allowance."""
    _need_gpu()
    import gzip
    import hashlib
    from witch_amd import gcmm
    case = load_case("example_e2e")
    g = case.g

    class _Sub:
        def __init__(self, path, n):
            self.hmm_model_path, self.num_taxa = path, n
    index_to_hmm = {i: _Sub(p, n) for i, p, n in zip(case.hmm_index, case.hmm_paths, case.nseq)}
    kw = dict(subset_to_retained_columns={int(k): v for k, v in g["retained"].items()},
              subset_to_nongaps_per_column={int(k): v for k, v in g["nongaps"].items()}, backbone_length=g["backbone_length"])
    bpath = str(tmp_path / "backbone.fasta")
    with gzip.open(os.path.join(case.dir, "backbone.fasta.gz"), "rt") as f, open(bpath, "w") as o:
        o.write(f.read())
    queries = list(zip(case.qnames, case.qseqs))
    lens = sorted(len(s) for s in case.qseqs)
    lmain = lens[-E2E_LONG_QUERIES - 1]
    n_long = sum(1 for n in lens if n > lmain)
    assert 0 < n_long <= E2E_LONG_QUERIES

    def files_of(eng, name):
        gcmm.install(eng)
        o, m = gcmm.mergeAlignmentsDevice(bpath, {}, output_path=str(tmp_path / name))
        return hashlib.sha256(open(o, "rb").read()).hexdigest(), hashlib.sha256(open(m, "rb").read()).hexdigest()

    base = gcmm.QueryAlignmentEngine.run(index_to_hmm, queries, case.k, **kw)
    assert base.long_score_pairs == 0
    base_sha = files_of(base, "base.fasta")
    monkeypatch.setenv("WH_SCORE_LMAIN", str(lmain))
    eng = gcmm.QueryAlignmentEngine.run(index_to_hmm, queries, case.k, **kw)
    monkeypatch.delenv("WH_SCORE_LMAIN")
    print("Lmain", lmain, "long queries", n_long, "long_score_pairs", eng.long_score_pairs)
    assert eng.long_score_pairs == n_long * len(case.hmm_paths)
    short = np.array([len(s) <= lmain for s in case.qseqs])
    assert np.array_equal(eng.decibits[short], base.decibits[short]) and np.array_equal(eng.flags[short], base.flags[short])
    n_mask = n_score = 0
    for col, hf in enumerate(case.hmm_files):
        S = g["search"][hf]
        for row, qn in enumerate(case.qnames):
            rep = bool(eng.flags[row, col] & 1)
            if rep != (qn in S):
                n_mask += 1
            elif rep and int(round(S[qn]["score"] * 10)) != int(eng.decibits[row, col]):
                n_score += 1
                assert abs(int(round(S[qn]["score"] * 10)) - int(eng.decibits[row, col])) == 1, (hf, qn)
    differ = int((eng.decibits != base.decibits).sum()), int((eng.flags != base.flags).sum())
    print("against HMMER: %d reported-mask differences, %d scores one deci-bit off; against the run without the knob: %d scores, %d flags differ" % (n_mask, n_score, *differ))
    assert n_mask <= 3 and n_score <= 2, (n_mask, n_score)
    assert (eng.flags & 8).sum() == 0 and not eng.truncated_pairs and not eng.unaligned_pairs
    sha = files_of(eng, "long.fasta")
    assert sha == base_sha, (sha, base_sha)
    assert sha == (g["final_sha256"]["full"], g["final_sha256"]["masked"])


@pytest.mark.gpu
def test_level0_shims_pass_a_long_query_through(tmp_path, monkeypatch):
    """hmmsearch and hmmalign (the C clients and the resident GPU server) with WH_SCORE_LMAIN in the server's environment, so
    that half the queries of dna_hmmbuild are beyond the cap: the calls succeed, the handle reports pairs of the long-query
    passes, and the outputs are HMMER's golden ones as far as test_level0_shims_reproduce_hmmer_outputs asks."""
    _need_gpu()
    import threading
    from tests.refparse import evalHMMSearchOutput
    from witch_amd.shim import formats
    from witch_amd.shim.server import Server, GpuBackend
    bindir = os.path.join(ROOT, "witch_amd", "shim", "bin")
    subprocess.run(["make", "-C", os.path.join(ROOT, "witch_amd", "shim")], check=True, stdout=subprocess.DEVNULL)
    case = load_case("dna_hmmbuild")
    lens = sorted(len(s) for s in case.qseqs)
    lmain = lens[len(lens) // 2]
    assert lens[-1] > lmain
    monkeypatch.setenv("WH_SCORE_LMAIN", str(lmain))
    sock = str(tmp_path / "gpu.sock")
    backend = GpuBackend(0)
    srv = Server(backend, sock)
    ready = threading.Event()
    threading.Thread(target=srv.serve_forever, args=(ready,), daemon=True).start()
    assert ready.wait(10)
    env = dict(os.environ, WITCH_HIP_SOCKET=sock)
    fa = os.path.join(case.dir, "queries.fasta")
    hf, hp = case.hmm_files[0], case.hmm_paths[0]
    out = str(tmp_path / ("hmmsearch.results." + os.path.basename(hf)))
    r = subprocess.run([os.path.join(bindir, "hmmsearch"), "--cpu", "1", "--noali", "-E", "99999999", "-o", out, "--max", hp, fa],
                       env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    handle = backend.cache[os.path.realpath(hp)][1]
    n_long = sum(1 for n in lens if n > lmain)
    assert handle.last_long_score() == (n_long, lens[-1]), (handle.last_long_score(), n_long)
    got, want = evalHMMSearchOutput(out), case.g["search"][hf]
    multi = {q for q, v in want.items() if len(v.get("dom", [0])) != 1}
    assert len(set(got) ^ set(want)) <= max(1, len(want) // 20), (hf, set(got) ^ set(want))
    seqs = dict(zip(case.qnames, case.qseqs))
    n_long_scores = 0
    for q, (ev, sc) in got.items():
        if q in multi or q not in want:
            continue
        assert abs(sc - want[q]["score"]) <= 0.1001, (hf, q, sc, want[q]["score"])
        n_long_scores += len(seqs[q]) > lmain
    assert n_long_scores > 0
    n_aln = 0
    for qn, a in case.g["align"].items():
        if len(seqs[qn]) <= lmain or n_aln >= 3:
            continue
        one = tmp_path / (qn + ".fa")
        one.write_text(">%s\n%s\n" % (qn, seqs[qn]))
        idx, cols = next(iter(a["cols"].items()))
        hp2 = case.hmm_paths[case.hmm_index.index(int(idx))]
        aout = str(tmp_path / ("hmmalign.%s.%s.out" % (qn, idx)))
        r = subprocess.run([os.path.join(bindir, "hmmalign"), "-o", aout, hp2, str(one)], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert backend.cache[os.path.realpath(hp2)][1].last_long_align() == (1, len(seqs[qn]))
        row = "".join(l.split()[1] for l in open(aout) if l.strip() and not l.startswith("#") and l.strip() != "//")
        assert formats.decode_stockholm_row(row) == list(cols), (qn, aout)
        n_aln += 1
    assert n_aln > 0
