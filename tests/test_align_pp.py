"""Per-residue posterior probabilities of wh_align_pp (hmmalign's PP line) on the GPU, one test per alignment code path.

For every path: the columns are bit-identical to the same call with pp = NULL and to wh_align (and to hmmalign's stored
columns); pp is compared with the float64 reference of tests/pp_reference.py; its characters (formats.pp_char) with
hmmalign's stored ones (tests/golden/align_pp).

Tolerances (from the project, not from the code under test):
  float32 paths   |pp - ref| <= 2e-4 + 3e-6 L   (three factors F, B, 1/Z at the accepted Forward tolerance of 1e-4 bit =
                  7e-5 relative; kAlnWinTol * L = what the window certificate may drop)
  float64 kernel  1e-9
Characters: outside the guard band (reference within the path's tolerance of a character boundary) equal to hmmalign's;
inside it at most one step apart; at most 1 % of a case's residues lie in the band.
"""
import os

import numpy as np
import pytest

from tests import pp_reference as ppr
from tests.conftest import load_case

pytestmark = pytest.mark.gpu

CHARS = "0123456789*"
BOUNDS = 0.05 + np.arange(10) / 10.0


def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def tol32(L):
    return 2e-4 + 3e-6 * L


def _case(name):
    from witch_amd.ehmm import EHMM, pack_queries
    case = load_case(name)
    e = EHMM(case.hmm_paths, hmm_index=case.hmm_index, nseq=case.nseq)
    seqs = [e.digitize(s) for s in case.qseqs]
    res, offs = pack_queries(seqs)
    ref = ppr.case_reference(name)
    pq = np.array([r[0] for r in ref], dtype=np.int64)
    ph = np.array([r[1] for r in ref], dtype=np.int32)
    return e, seqs, res, offs, pq, ph, ref


def _align3(e, res, offs, pq, ph):
    """The three calls of every test: wh_align, wh_align_pp with pp = NULL, wh_align_pp with pp; the columns of all
    three must be the same bytes.  Returns (cols, col_offsets, pp)."""
    from witch_amd._lib import check, lib
    c0, co = e.align(res, offs, pq, ph)
    c1 = np.full_like(c0, -7)
    res = np.ascontiguousarray(res, dtype=np.uint8)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    pq = np.ascontiguousarray(pq, dtype=np.int64)
    ph = np.ascontiguousarray(ph, dtype=np.int32)
    check(lib().wh_align_pp(e._h, res.ctypes.data, offs.ctypes.data, len(offs) - 1, pq.ctypes.data, ph.ctypes.data, len(pq),
                            co.ctypes.data, c1.ctypes.data, None), "wh_align_pp")
    c2, co2, pp = e.align(res, offs, pq, ph, want_pp=True)
    assert pp.dtype == np.float32 and len(pp) == len(c2) and np.array_equal(co, co2)
    assert c0.tobytes() == c1.tobytes() == c2.tobytes(), "columns change with the PP output"
    return c0, co, pp


def _steps(a, b):
    return abs(CHARS.index(a) - CHARS.index(b))


def _check(tag, ref, cols, co, pp, tol_of, cap=0.01):
    """pp against the reference within tol_of(pair number, L), characters against hmmalign's; returns the largest |delta|."""
    from witch_amd.shim.formats import pp_char
    worst, n, n_band = 0.0, 0, 0
    for p, (q, h, want_cols, digits, want) in enumerate(ref):
        got_c, got = cols[co[p]:co[p + 1]], pp[co[p]:co[p + 1]].astype(np.float64)
        L = len(want)
        assert np.array_equal(got_c, want_cols), (tag, "columns", q, h)
        tol = tol_of(p, L)
        d = np.abs(got - want)
        worst = max(worst, float(d.max()) if L else 0.0)
        assert np.all(np.isfinite(got)) and np.all(d <= tol), (tag, q, h, "max |pp - ref| %.3g > %.3g" % (d.max(), tol))
        band = np.min(np.abs(want[:, None] - BOUNDS[None, :]), axis=1) <= tol
        n += L
        n_band += int(band.sum())
        for i in range(L):
            c = pp_char(got[i])
            if c != digits[i]:
                assert band[i] and _steps(c, digits[i]) == 1, (tag, q, h, i, c, digits[i], want[i])
    print("%s: %d residues, largest |pp - ref| %.3g, %d in the guard band" % (tag, n, worst, n_band))
    assert n_band <= cap * n, (tag, "residues in the guard band", n_band, n)
    return worst


@pytest.mark.parametrize("name", ["dna_hmmbuild", "amino_hmmbuild"])
def test_default_launch(name):
    """Path 1: the default launch on the golden cases.  (Their models have fewer than 8 nodes per lane, where the kernel
    has no window: test_node_window.)"""
    _need_gpu()
    e, seqs, res, offs, pq, ph, ref = _case(name)
    cols, co, pp = _align3(e, res, offs, pq, ph)
    e.close()
    _check(name + " default", ref, cols, co, pp, lambda p, L: tol32(L))


@pytest.mark.parametrize("name", ["dna_hmmbuild", "amino_hmmbuild"])
def test_full_width(name):
    """Path 2: the same with WH_NO_WINDOW=1."""
    _need_gpu()
    e, seqs, res, offs, pq, ph, ref = _case(name)
    e.set_option("WH_NO_WINDOW", "1")
    cols, co, pp = _align3(e, res, offs, pq, ph)
    e.close()
    _check(name + " full width", ref, cols, co, pp, lambda p, L: tol32(L))


def test_device_resident_entry_point():
    """EHMM.align_t(want_pp=True) (wh_align_pp_dev on torch tensors) gives the bytes of the host entry point."""
    _need_gpu()
    import torch
    e, seqs, res, offs, pq, ph, ref = _case("dna_hmmbuild")
    cols, co, pp = e.align(res, offs, pq, ph, want_pp=True)
    dev = torch.device("cuda:0")
    ct, pt = e.align_t(torch.from_numpy(res).to(dev), torch.from_numpy(offs).to(dev), int(np.diff(offs).max()),
                       torch.from_numpy(pq).to(dev), torch.from_numpy(ph).to(dev), torch.from_numpy(co).to(dev), int(co[-1]),
                       want_pp=True)
    e.close()
    assert ct.cpu().numpy().tobytes() == cols.tobytes() and pt.cpu().numpy().tobytes() == pp.tobytes()


@pytest.mark.parametrize("alphabet", ["dna", "amino"])
def test_node_window(alphabet, tmp_path):
    """Path 1 where it differs from path 2: two 700-node models and 36 fragment queries (pp_reference.window_case; hmmalign's
    text in the fixture window_<alphabet>), aligned on a node window - which must have run - and at full width.  0.17 %
    (DNA) and 0.05 % (protein) of these residues lie in the guard band (reference alone, measured on the CPU)."""
    _need_gpu()
    from witch_amd.ehmm import EHMM, pack_queries
    paths, names, seqs = ppr.window_case(alphabet, str(tmp_path))
    ref = ppr.fixture_reference("window_" + alphabet, paths, seqs)
    e = EHMM(paths)
    res, offs = pack_queries(seqs)
    pq = np.array([r[0] for r in ref], dtype=np.int64)
    ph = np.array([r[1] for r in ref], dtype=np.int32)
    wcols, co, wpp = _align3(e, res, offs, pq, ph)
    paths_run = e.last_align_paths()
    e.set_option("WH_NO_WINDOW", "1")
    fcols, fco, fpp = _align3(e, res, offs, pq, ph)
    e.close()
    assert paths_run["window256"] + paths_run["window512"] > 0, paths_run
    _check(alphabet + " node window", ref, wcols, co, wpp, lambda p, L: tol32(L))
    _check(alphabet + " node window, full width", ref, fcols, fco, fpp, lambda p, L: tol32(L))
    # a window's posteriors are lower bounds of the full-width ones, up to float32 noise
    for p in range(len(ref)):
        assert np.all(wpp[co[p]:co[p + 1]] <= fpp[co[p]:co[p + 1]] + tol32(co[p + 1] - co[p]))


def test_several_waves_per_pair():
    """Path 3: the several-waves-per-pair kernel forced onto dna_hmmbuild (WH_FORCE_WIDE=4, read at load)."""
    _need_gpu()
    old = os.environ.get("WH_FORCE_WIDE")
    os.environ["WH_FORCE_WIDE"] = "4"
    try:
        e, seqs, res, offs, pq, ph, ref = _case("dna_hmmbuild")
        cols, co, pp = _align3(e, res, offs, pq, ph)
        e.close()
    finally:
        if old is None:
            os.environ.pop("WH_FORCE_WIDE", None)
        else:
            os.environ["WH_FORCE_WIDE"] = old
    _check("dna_hmmbuild, several waves per pair", ref, cols, co, pp, lambda p, L: tol32(L))


@pytest.fixture(scope="module")
def any_size_runs():
    """The three runs of path 4, made once for its two tests."""
    _need_gpu()
    e, seqs, res, offs, pq, ph, ref = _case("dna_hmmbuild")
    lens = np.array([len(s) for s in seqs])
    lmain = int(np.median(lens))
    e.set_option("WH_SCORE_LMAIN", str(lmain))
    cols, co, pp = _align3(e, res, offs, pq, ph)
    n_long = e.last_long_align()[0]
    cols64, co64, pp64 = e.align(res, offs, pq, ph, want_pp="float64")
    assert pp64.dtype == np.float64 and cols64.tobytes() == cols.tobytes() and np.array_equal(co64, co)
    assert pp64.astype(np.float32).tobytes() == pp.tobytes(), "the float output is not the float64 output rounded once"
    e.set_option("WH_LONGQ_FORCE", "1")
    cols2, co2, pp2 = _align3(e, res, offs, pq, ph)
    n_long2 = e.last_long_align()[0]
    e.close()
    long_pair = lens[pq] > lmain
    assert n_long == n_long2 == int(long_pair.sum()) > 0
    return ref, cols, co, pp, cols2, pp2, long_pair, pp64


def test_any_size_float64_kernel_columns_characters_and_both_residue_placements(any_size_runs):
    """Path 4: queries longer than the median go to the any-size float64 kernel (WH_SCORE_LMAIN), then the same with the
    residues in the wave's HBM slab (WH_LONGQ_FORCE): columns, characters, and PP bitwise equal between the two runs.
    The float output is held to what one rounding of a float64 posterior to float32 allows: 1e-9 plus half a float32
    spacing at the value (3e-8 below 1), and must be the float64 output (wh_align_pp64) rounded once; the bound of 1e-9
    itself is the next test's, on the float64 output."""
    ref, cols, co, pp, cols2, pp2, long_pair, pp64 = any_size_runs
    assert cols.tobytes() == cols2.tobytes() and pp.tobytes() == pp2.tobytes()
    half_ulp = lambda v: np.spacing(np.maximum(v, 1e-30).astype(np.float32)).astype(np.float64) / 2   # noqa: E731
    worst = 0.0
    for p, (q, h, _, _, want) in enumerate(ref):
        if long_pair[p]:
            d = np.abs(pp[co[p]:co[p + 1]].astype(np.float64) - want)
            worst = max(worst, float(d.max()))
            assert np.all(d <= 1e-9 + half_ulp(want)), (q, h, float(d.max()))
    print("float64 kernel: largest |pp - ref| %.3g" % worst)
    _check("dna_hmmbuild, any-size kernel", ref, cols, co, pp, lambda p, L: 1e-9 + 2.0 ** -25 if long_pair[p] else tol32(L))


def test_any_size_float64_kernel_values_within_1e_9(any_size_runs):
    """Path 4, the bound as set: |pp - ref| <= 1e-9 on the pairs of the float64 kernel.  The bound is asserted on the
    float64 output only (wh_align_pp64); the float output of wh_align_pp is held to 1e-9 plus one rounding to float32 in the
    test in front of this one, which is looser than 1e-9 (wh_align_pp64: a float holds a value below 1 only to 2^-25 = 2.98e-8, which is what the float output of the same
    call is off by - the test in front of this one).  The float32 kernels' pairs of the same call come back as their
    float32 values widened and keep the float32 bound."""
    ref, cols, co, pp, cols2, pp2, long_pair, pp64 = any_size_runs
    worst = 0.0
    for p, (q, h, _, _, want) in enumerate(ref):
        got = pp64[co[p]:co[p + 1]]
        if long_pair[p]:
            worst = max(worst, float(np.abs(got - want).max()))
        else:
            assert np.array_equal(got, pp[co[p]:co[p + 1]].astype(np.float64)) and np.abs(got - want).max() <= tol32(len(want))
    print("float64 kernel, float64 output: largest |pp - ref| %.3g" % worst)
    assert worst <= 1e-9, worst


def _long_model_runs(tmp_path, kind_wanted):
    """The 1 900-node model of the fixture and its queries of one class, each aligned in a call of its own:
    [(q, query, hmmalign's columns, hmmalign's characters, reference, cols, pp, pp64, n_logspace)]."""
    from oracle import oracle as orc
    from witch_amd.ehmm import EHMM, pack_queries
    fx = ppr.load_fixture("long_model")
    fam, hp = ppr.long_model(fx["spec"], str(tmp_path))
    names, seqs, kinds = ppr.long_queries(fx["spec"], fam)
    model = ppr.Model(orc.OracleHMM(hp))
    e = EHMM([hp])
    assert int(e.M[0]) > 1536                      # the pass-synchronous kernels' range
    out = []
    for q, (s, kind, rec) in enumerate(zip(seqs, kinds, fx["pairs"])):
        if kind != kind_wanted:
            continue
        _, row, ppl, _, rf = ppr.parse_stockholm(rec["sto"])
        want_cols, digits = ppr.row_cols_digits(row, ppl, rf)
        assert len(digits) == len(s) == rec["L"]
        want = ppr.path_posteriors(model, s, want_cols)
        res, offs = pack_queries([s])
        cols, co, pp = _align3(e, res, offs, np.zeros(1, np.int64), np.zeros(1, np.int32))
        n_log = e.last_align_status()[0]
        c64, _, pp64 = e.align(res, offs, np.zeros(1, np.int64), np.zeros(1, np.int32), want_pp="float64")
        assert c64.tobytes() == cols.tobytes() and pp64.astype(np.float32).tobytes() == pp.tobytes()
        out.append((q, s, want_cols, digits, want, cols, pp, pp64, n_log))
    e.close()
    return fx, out


def test_pass_synchronous_kernels(tmp_path):
    """Path 5, probability space: two fragment queries of 150 - 400 nt on one 1 900-node DNA model (pass-synchronous
    kernels, one table orientation resident) stay in float32 range and meet the float32 tolerance."""
    _need_gpu()
    fx, runs = _long_model_runs(tmp_path, "fragment")
    assert len(runs) == 2
    for q, s, want_cols, digits, want, cols, pp, pp64, n_log in runs:
        assert 150 <= len(s) <= 400 and n_log == 0
        _check("long model, fragment %d" % q, [(q, 0, want_cols, digits, want)], cols, np.array([0, len(s)]), pp, lambda p, L: tol32(L))


def test_pairs_that_leave_float32_range(tmp_path):
    """Path 5, log space: two multi-copy queries (2 215 and 2 799 nt, the shortest of the recipe's four) on the 1 900-node
    model; each leaves float32 range (n_logspace > 0).  Without PP such a pair is redone by the float32 log-space pass; a
    call with PP hands it to the float64 any-size kernel instead (the log-space pass's float32 posteriors were measured up
    to 0.033 from the reference and up to 1.016), whose own log-space code is float64.  Checked: hmmalign's columns from
    both; the characters against hmmalign's under the fixture's cap (twice the share on which hmmalign's own character
    differs from the reference's, or 1 % when that share is below 0.5 % - it is 0), never more than one step; and the
    values against the reference: float64 logarithms of up to 1.39 L nats (ln 4 per DNA residue) summed over L rows
    carry at most L * 2^-53 * 1.39 L each, three of them (F, B, Z) make 4.6e-16 L^2 = 3.6e-9 at 2 799 nt, on the float64
    output; the float output adds one rounding to float32."""
    _need_gpu()
    from witch_amd.shim.formats import pp_char
    fx, runs = _long_model_runs(tmp_path, "multicopy")
    assert len(runs) == 2
    share = fx["hmmalign_vs_reference_share"]["multicopy"]
    cap = 2.0 * share if share >= 0.005 else 0.01
    for q, s, want_cols, digits, want, cols, pp, pp64, n_log in runs:
        L = len(s)
        assert n_log > 0, (q, "stayed in float32 range")
        assert np.array_equal(cols, want_cols)
        tol = 3 * L * 2.0 ** -53 * 1.39 * L
        d64, d32 = np.abs(pp64 - want), np.abs(pp.astype(np.float64) - want)
        steps = np.array([_steps(pp_char(pp[i]), digits[i]) for i in range(L)])
        print("long model, query %d (%d residues) left float32 range: largest |pp64 - ref| %.3g (bound %.3g), float output %.3g, "
              "%d characters differ (cap %.1f)" % (q, L, float(d64.max()), tol, float(d32.max()), int((steps > 0).sum()), cap * L))
        assert np.all(np.isfinite(pp64)) and pp64.min() >= 0.0 and pp64.max() <= 1.0 + 1e-6
        assert d64.max() <= tol and d32.max() <= tol + 2.0 ** -25
        assert steps.max() <= 1 and (steps > 0).sum() <= cap * L


def test_edges(tmp_path):
    """A 1-residue query, an unrelated sequence, degenerate codes and a zero-length query in one batch; pp pre-filled with
    NaN between guard words and with gaps between the pairs' ranges: every entry of a range is finite and in
    [0, 1 + 1e-6] and within the float32 tolerance of the reference, everything else is untouched."""
    _need_gpu()
    from oracle import oracle as orc
    from witch_amd import synth
    from witch_amd._lib import check, lib
    from witch_amd.ehmm import EHMM, pack_queries
    fam = synth.make_family(1000 + 21, 300, 8, "dna", 0.05, 2e-3)
    eh = synth.make_ehmm(fam, 2, str(tmp_path), witch_layout=False)
    rng = np.random.default_rng(21)
    _, frag = synth.make_queries(fam, 2100, 3, 120)
    deg = frag[1].astype(np.uint8).copy()
    deg[rng.integers(0, len(deg), size=12)] = rng.integers(4, 15, size=12).astype(np.uint8)     # degenerate codes (not gap / * / ~)
    seqs = [frag[0][:1].astype(np.uint8), rng.choice(4, size=90, p=synth.background("dna")).astype(np.uint8), deg,
            np.zeros(0, np.uint8), frag[2].astype(np.uint8)]
    e = EHMM(eh.paths, hmm_index=eh.index, nseq=eh.nseq)
    res, offs = pack_queries(seqs)
    res = np.ascontiguousarray(res, dtype=np.uint8)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    pq = np.repeat(np.arange(len(seqs), dtype=np.int64), e.H)
    ph = np.tile(np.arange(e.H, dtype=np.int32), len(seqs))
    lens = np.array([len(seqs[q]) for q in pq])
    GAP, GUARD = 5, 8
    co = np.zeros(len(pq) + 1, dtype=np.int64)
    co[1:] = np.cumsum(lens + GAP)
    buf = np.full(GUARD + int(co[-1]) + GUARD, np.nan, dtype=np.float32)
    cols = np.full(int(co[-1]), -9, dtype=np.int32)
    pp = buf[GUARD:GUARD + int(co[-1])]
    check(lib().wh_align_pp(e._h, res.ctypes.data, offs.ctypes.data, len(offs) - 1, pq.ctypes.data, ph.ctypes.data, len(pq),
                            co.ctypes.data, cols.ctypes.data, pp.ctypes.data), "wh_align_pp")
    cols0 = np.full(int(co[-1]), -9, dtype=np.int32)
    check(lib().wh_align(e._h, res.ctypes.data, offs.ctypes.data, len(offs) - 1, pq.ctypes.data, ph.ctypes.data, len(pq),
                         co.ctypes.data, cols0.ctypes.data), "wh_align")
    e.close()
    assert np.all(np.isnan(buf[:GUARD])) and np.all(np.isnan(buf[-GUARD:]))
    ohm = [orc.OracleHMM(p) for p in eh.paths]
    models = [ppr.Model(o) for o in ohm]
    for p in range(len(pq)):
        a, L = int(co[p]), int(lens[p])
        assert np.all(np.isnan(pp[a + L:int(co[p + 1])])), (p, "gap behind the range written")
        got, got_c = pp[a:a + L].astype(np.float64), cols[a:a + L]
        assert np.array_equal(got_c, cols0[a:a + L])
        assert np.all(np.isfinite(got)) and np.all(got >= 0.0) and np.all(got <= 1.0 + 1e-6), (p, got)
        want_c = ohm[ph[p]].align(seqs[pq[p]])
        assert np.array_equal(got_c, want_c)
        want = ppr.path_posteriors(models[ph[p]], seqs[pq[p]], want_c)
        if L:
            assert np.abs(got - want).max() <= tol32(L), (p, float(np.abs(got - want).max()))
