"""The 16-bit per-pair path record (wh_set_path_buffer16): written by the default fused kernel and by every other
scoring kernel, equal to what the staged launches record, consistent with the counters and flags the library already
reports, and - the point of it - a stratum of band-failed pairs checked against the float64 oracle.

Inputs: the committed golden cases example_e2e (500 real 16S fragments x 15 models of 1 278 - 2 574 nodes; the models of up
to 1 536 nodes are the 20- and 24-cell classes of the fused kernel, the longer ones go through the pass-synchronous
kernel) and dna_hmmbuild (50 x 8 small models)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gpu_parity import BOUNDARY_EPS, _check_one_decibit, _need_gpu, orc  # noqa: F401  (orc: fixture)

pytestmark = pytest.mark.gpu

P2_WIN, P2_FULL, P4_W256, P4_W512, P4_WFAIL, P4_FULL, DENSE, MULTI, BAND_KEPT, BAND_FAIL = (1 << b for b in range(10))
P2_ANY = P2_WIN | P2_FULL
P4_ANY = P4_W256 | P4_W512 | P4_WFAIL | P4_FULL
WINDOW_BITS = P2_WIN | P4_W256 | P4_W512 | P4_WFAIL
BAND_BITS = BAND_KEPT | BAND_FAIL
PREFILL = 0x7FFF
F_REPORTED, F_MULTI, F_EXACT = 1, 2, 16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_shared = {}


def _record(e, res, offs, shape, **kw):
    """One scoring call with a prefilled 16-bit record: (deci-bits, flags, [fwd,] record, counters)."""
    import torch
    rec = torch.full(shape, PREFILL, dtype=torch.int16, device="cuda")
    e.set_path_buffer16(rec)
    try:
        out = e.score(res, offs, **kw)
        cnt = e.last_score_paths()
    finally:
        e.set_path_buffer16(None)
    return tuple(out) + (rec.cpu().numpy().astype(np.int32) & 0xFFFF, cnt)


def _e2e():
    """example_e2e scored by the default kernel without the record and with it, and by the fully staged launches
    (WH_SCORE_KERNEL=11) with a second 16-bit buffer and the 8-bit one; shared by the tests below."""
    if "e2e" not in _shared:
        import torch
        from tests.conftest import load_case
        from witch_amd.ehmm import EHMM, pack_queries
        case = load_case("example_e2e")
        e = EHMM(case.hmm_paths, hmm_index=case.hmm_index, nseq=case.nseq)
        res, offs = pack_queries([e.digitize(s_) for s_ in case.qseqs])
        shape = (len(offs) - 1, e.H)
        plain = e.score(res, offs, want_fwd=True)
        d, f, w, rec, cnt = _record(e, res, offs, shape, want_fwd=True)
        p8 = torch.full(shape, 0xEE, dtype=torch.uint8, device="cuda")       # (0xEE is no record: P2_WIN and P2_FULL exclude each other)
        e.set_path_buffer(p8)
        e.set_option("WH_SCORE_KERNEL", "11")
        try:
            staged = _record(e, res, offs, shape, want_fwd=True)
            reruns = e.last_queue_reruns()
        finally:
            e.set_option("WH_SCORE_KERNEL", "")
            e.set_path_buffer(None)
        _shared["e2e"] = dict(case=case, e=e, res=res, offs=offs, shape=shape, plain=plain, d=d, f=f, w=w, rec=rec, cnt=cnt,
                              staged=staged, reruns=reruns, p8=p8.cpu().numpy().astype(np.int32),
                              reg=np.asarray(e.M) <= 24 * 64)          # models of the one-wavefront-per-pair (register) kernels
    return _shared["e2e"]


def test_default_kernel_fills_the_record():
    """Test 1 (fails without the feature).  The default kernel writes every element of the prefilled array, a reported pair
    has a P2 bit and a P4 / dense / resolver bit, and the call computes bitwise what it computes with no record set."""
    _need_gpu()
    s = _e2e()
    rec, f, reg = s["rec"], s["f"], s["reg"]
    assert rec.shape == s["shape"] and not np.any(rec == PREFILL) and np.all(rec < 1024)
    rep = (f & F_REPORTED) != 0
    assert rep.sum() > 0 and reg.any()
    assert np.all((rec[rep] & P2_ANY) != 0)
    assert np.all((rec[rep] & (P4_ANY | DENSE | MULTI)) != 0)
    assert not np.any(((rec & P2_WIN) != 0) & ((rec & P2_FULL) != 0))         # a pair's regions come from ONE of the two sweeps
    d0, f0, w0 = s["plain"]
    assert np.array_equal(s["d"], d0) and np.array_equal(f, f0) and np.array_equal(s["w"].view(np.uint32), w0.view(np.uint32))
    assert np.any(rec[:, reg] & BAND_BITS) and np.any(rec[:, reg] & WINDOW_BITS)


def test_fused_record_equals_the_staged_record():
    """Test 2.  The staged launches (WH_SCORE_KERNEL=11) record the same 16 bits for every pair, no batch fell back, results
    are identical, and the low byte of the staged launches' record is what the 8-bit wh_set_path_buffer gets in that call.
    (A class whose batch does not fit the staged launches' LDS plans - the 24-cell models with fragments beyond 300 nt - is
    left to the fused kernel in that call too: its pairs are in the 16-bit record and not in the 8-bit one.  On an MI355X
    the staged launches served the 500 pairs of the 20-cell model; 0 of 7 500 records differ.)"""
    _need_gpu()
    s = _e2e()
    d, f, w, rec11, cnt11 = s["staged"]
    assert s["reruns"] == 0
    assert np.array_equal(d, s["d"]) and np.array_equal(f, s["f"])
    assert not np.any(rec11 == PREFILL)
    staged = s["p8"] != 0xEE
    print("pairs the staged launches served: %d of %d register-class pairs" % (int(staged.sum()), int(s["reg"].sum()) * s["shape"][0]))
    assert staged.any() and not staged[:, ~s["reg"]].any()
    assert np.array_equal(s["p8"][staged], rec11[staged] & 0xFF)
    diff = np.argwhere(rec11 != s["rec"])
    print("pairs whose fused and staged records differ: %d of %d" % (len(diff), rec11.size))
    for q, h in diff[:12]:
        print("  pair (%d, %d): fused %#05x staged %#05x" % (q, h, s["rec"][q, h], rec11[q, h]))
    assert len(diff) == 0


def test_record_agrees_with_flags_and_counters():
    """Dense <=> WH_FLAG_EXACT; resolver bit <=> WH_FLAG_MULTI on reported pairs of the register-kernel classes; each of the
    five path counters whose event has a bit of its own (256-node window, 512-node window, window rejected, full width,
    P2 window kept) counts envelopes or sweeps, so its bit is on no more pairs than the counter says, and on some pair iff
    the counter is non-zero.  The sixth counter (P2 window in doubt) has no bit of its own: such a pair carries
    WH_PATH_P2_FULL like a pair that never tried a window, so there the bit bounds the counter from ABOVE.  Without the
    band (WH_SPILL_BAND=0) no band bit, without windows (WH_NO_WINDOW=1) no window bit."""
    _need_gpu()
    s = _e2e()
    e, rec, f, cnt, reg = s["e"], s["rec"], s["f"], s["cnt"], s["reg"]
    assert np.array_equal((rec & DENSE) != 0, (f & F_EXACT) != 0)
    rep = ((f & F_REPORTED) != 0)[:, reg]
    assert np.array_equal(((rec[:, reg] & MULTI) != 0)[rep], ((f[:, reg] & F_MULTI) != 0)[rep])
    r = rec[:, reg]                                                         # (the counters count the register kernels only)
    for name, bit in (("window256", P4_W256), ("window512", P4_W512), ("window_rejected", P4_WFAIL), ("full_width", P4_FULL), ("p2_window", P2_WIN)):
        n = int(((r & bit) != 0).sum())
        print("%-16s counter %7d  pairs with the bit %7d" % (name, cnt[name], n))
        assert n <= cnt[name], (name, n, cnt[name])
        assert (n > 0) == (cnt[name] > 0), (name, n, cnt[name])
    n_full2 = int(((r & P2_FULL) != 0).sum())
    print("%-16s counter %7d  pairs with P2_FULL %7d" % ("p2_window_in_doubt", cnt["p2_window_in_doubt"], n_full2))
    assert cnt["p2_window_in_doubt"] <= n_full2
    # a band that failed is followed by a full-width sweep of the banded rows, and the two band bits of one ENVELOPE exclude
    # each other (a pair may carry both: two envelopes)
    assert np.all((r[(r & BAND_FAIL) != 0] & P4_FULL) != 0)
    assert not np.any(rec[:, ~reg] & (WINDOW_BITS | BAND_BITS))             # the pass-synchronous kernel has neither
    for opt, val, forbidden in (("WH_SPILL_BAND", "0", BAND_BITS), ("WH_NO_WINDOW", "1", WINDOW_BITS)):
        e.set_option(opt, val)
        try:
            d, f2, rec2, cnt2 = _record(e, s["res"], s["offs"], s["shape"])
        finally:
            e.set_option(opt, "")
        assert not np.any(rec2 == PREFILL) and not np.any(rec2 & forbidden), opt
        assert np.array_equal(f2 & 3, f & 3), opt


def _oracle_check(orc, s, d, f, w, pq, ph, tag):
    ohm = [None] * s["e"].H
    for h in set(ph):
        ohm[h] = orc.OracleHMM(s["case"].hmm_paths[h])
    od, of, ofwd, osc = orc.score_pairs(ohm, s["res"], s["offs"], pq, ph)
    pq, ph = np.array(pq), np.array(ph)
    gd, gf, gw = d[pq, ph], f[pq, ph], w[pq, ph]
    bad = np.nonzero((gf & 3) != (of & 3))[0]
    assert len(bad) == 0, [(tag, int(pq[i]), int(ph[i]), int(gf[i]), int(of[i])) for i in bad[:5]]
    fin = np.isfinite(ofwd)
    assert np.all(np.abs(gw[fin] - ofwd[fin]) <= 1e-4), float(np.max(np.abs(gw[fin] - ofwd[fin])))
    n_off = 0
    for i in np.nonzero(gd != od)[0]:
        n_off += _check_one_decibit(gd[i], od[i], osc[i], (tag, int(pq[i]), int(ph[i])), 0.02 if of[i] & 2 else BOUNDARY_EPS)
    return n_off


def _strata(rec, seed, most=300):
    fail = np.argwhere((rec & BAND_FAIL) != 0)
    kept = np.argwhere(((rec & BAND_KEPT) != 0) & ((rec & BAND_FAIL) == 0))
    rng = np.random.default_rng(seed)
    if len(fail) > most:
        fail = fail[rng.choice(len(fail), size=most, replace=False)]
    if len(kept) > len(fail):
        kept = kept[rng.choice(len(kept), size=max(len(fail), 1), replace=False)]
    return fail, kept


def test_band_failed_stratum_against_the_oracle(orc):
    """Test 4.  With the default band on example_e2e, record of the default kernel: every pair with WH_PATH_BAND_FAIL (up to 300, seeded choice) and as
    many with WH_PATH_BAND_KEPT only go through the float64 oracle under test_gpu_parity's rule - reported / multidomain
    flags identical, Forward log-odds within 1e-4 bit, deci-bits under the rounding-boundary rule of SURVEY 8.0.  The
    stratum must not be empty.  Counted on an MI355X: 191 of the 7 500 pairs carry the band-failed bit, 36 the band-kept bit
    alone (only the 20-cell model is banded at this length cap); all 227 checked, none off by a deci-bit."""
    _need_gpu()
    s = _e2e()
    fail, kept = _strata(s["rec"], 5)
    n_fail = len(fail)
    print("band-failed pairs in the record: %d of %d (band kept only: %d); sampled %d + %d" %
          (int(((s["rec"] & BAND_FAIL) != 0).sum()), s["rec"].size, int((((s["rec"] & BAND_KEPT) != 0) & ((s["rec"] & BAND_FAIL) == 0)).sum()), n_fail, len(kept)))
    assert n_fail > 0
    both = np.concatenate([fail, kept])
    n_off = _oracle_check(orc, s, s["d"], s["f"], s["w"], [int(x) for x in both[:, 0]], [int(x) for x in both[:, 1]], "default band")
    print("one deci-bit off at a rounding boundary: %d of %d" % (n_off, len(both)))


def test_narrow_band_fills_the_stratum_and_changes_no_result(orc):
    """The stratum populated deterministically: WH_SPILL_BAND=1001 (margins of one node below and above P1's blocks) makes the
    band too narrow for most envelopes.  Flags and Forward log-odds equal the default band's bitwise, deci-bits are at most
    one unit apart (a pair that lost its band is stored unbanded: the result of a run without the band, and the band-vs-
    unbanded difference is the last bits of a float32 null2 sum), and a sample of its band-failed pairs passes the oracle."""
    _need_gpu()
    s = _e2e()
    e = s["e"]
    e.set_option("WH_SPILL_BAND", "1001")
    try:
        d, f, w, rec, cnt = _record(e, s["res"], s["offs"], s["shape"], want_fwd=True)
    finally:
        e.set_option("WH_SPILL_BAND", "")
    assert not np.any(rec == PREFILL)
    n_fail = int(((rec & BAND_FAIL) != 0).sum())
    print("narrow band: band-failed pairs %d, default band %d" % (n_fail, int(((s["rec"] & BAND_FAIL) != 0).sum())))
    assert n_fail > int(((s["rec"] & BAND_FAIL) != 0).sum())
    assert np.array_equal(f & 3, s["f"] & 3) and np.array_equal(w.view(np.uint32), s["w"].view(np.uint32))
    assert np.max(np.abs(d.astype(np.int64) - s["d"])) <= 1
    fail, kept = _strata(rec, 6, most=150)
    both = np.concatenate([fail, kept])
    _oracle_check(orc, s, d, f, w, [int(x) for x in both[:, 0]], [int(x) for x in both[:, 1]], "narrow band")


_CHILD = r"""
import json, sys
import numpy as np, torch
sys.path.insert(0, %r)
from tests.conftest import load_case
from witch_amd.ehmm import EHMM, pack_queries
case = load_case("dna_hmmbuild")
e = EHMM(case.hmm_paths, hmm_index=case.hmm_index, nseq=case.nseq)
res, offs = pack_queries([e.digitize(s_) for s_ in case.qseqs])
rec = torch.full((len(offs) - 1, e.H), 0x7FFF, dtype=torch.int16, device="cuda")
e.set_path_buffer16(rec)
d, f = e.score(res, offs)
e.set_path_buffer16(None)
e.close()
print("RECORD " + json.dumps({"rec": (rec.cpu().numpy().astype(np.int32) & 0xFFFF).tolist(), "flags": f.astype(np.int32).tolist()}))
"""


def _family_rule(rec, f):
    assert not np.any(rec == PREFILL)
    rep = (f & F_REPORTED) != 0
    assert rep.sum() > 0
    assert np.all((rec[rep] & (P2_FULL | P4_FULL)) == (P2_FULL | P4_FULL))
    assert not np.any(rec & (WINDOW_BITS | BAND_BITS))
    assert np.array_equal((rec & DENSE) != 0, (f & F_EXACT) != 0)


def test_wide_kernel_leaves_nothing_stale():
    """Every model through the several-waves-per-pair kernel (WH_FORCE_WIDE=12 is read when the library loads a
    model set: a fresh child process)."""
    _need_gpu()
    env = dict(os.environ, WH_FORCE_WIDE="12")
    out = subprocess.run([sys.executable, "-c", _CHILD % ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RECORD ")][-1][7:])
    _family_rule(np.array(got["rec"]), np.array(got["flags"]))


def test_long_query_scoring_pass_leaves_nothing_stale():
    """WH_SCORE_LMAIN below the longest query - the pairs of the longer queries are scored by the long-query
    scoring pass (the any-size float64 front end on a pair list) and carry ITS record; the others keep the main launches'."""
    _need_gpu()
    from tests.conftest import load_case
    from witch_amd.ehmm import EHMM, pack_queries
    case = load_case("dna_hmmbuild")
    e = EHMM(case.hmm_paths, hmm_index=case.hmm_index, nseq=case.nseq)
    res, offs = pack_queries([e.digitize(s_) for s_ in case.qseqs])
    lens = np.diff(offs)
    lmain = int(np.sort(lens)[len(lens) // 2])
    assert lmain < lens.max()
    e.set_option("WH_SCORE_LMAIN", str(lmain))
    try:
        d, f, rec, cnt = _record(e, res, offs, (len(lens), e.H))
        n_long = e.last_long_score()[0]
    finally:
        e.set_option("WH_SCORE_LMAIN", "")
    d0, f0 = e.score(res, offs)
    e.close()
    long_q = lens > lmain
    assert n_long == int(long_q.sum()) * len(case.hmm_paths) and n_long > 0
    assert np.array_equal(f & 3, f0 & 3)
    _family_rule(rec[long_q], f[long_q])
    assert not np.any(rec == PREFILL)
    rep = (f & F_REPORTED) != 0
    assert np.all((rec[rep] & P2_ANY) != 0) and np.all((rec[rep] & (P4_ANY | DENSE | MULTI)) != 0)
