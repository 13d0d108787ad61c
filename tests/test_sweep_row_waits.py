"""The row loops of the default scoring kernel that no longer wait for their own row stores and row requests (WH_ROW_WAITS,
wh_score7.hip) against the A/B slot, which keeps the parent's loops (WH_SCORE_KERNEL=8, K7B_FLAGS: WH_ROW_WAITS=0).

The change moves waits, never an operand or the order of a sum: every output must be the same BITS.  What it touches is the
branch between the two sources of a row's emission pieces - the LDS copy for a canonical residue, L2 for a degenerate code -
in the Forward sweeps and both window sweeps, and the place where the envelope window sweep requests the next Forward row.
So every length comes once canonical and once with degenerate codes (4..14 for DNA, as tests/test_gpu_parity.py draws them): at
row 1, at the last row, at two adjacent rows, at every eighth row (the rows whose mask the multihit Forward sweep samples),
and one query is degenerate throughout; a two-copy query carries one inside each copy (several envelopes).  Lengths 1, 2, 3
(without the resolver: envelopes of two and three rows), 8, 9, 64, 65, 149, 150, and 400 for the 512-node window.  One small
family per register class (8 to 24 cells per lane, the classes of tests/test_sweep_row_pairs.py), two models, 22 queries."""
import numpy as np
import pytest

from tests.test_gpu_parity import BOUNDARY_EPS, _check_one_decibit, _need_gpu
from tests.test_sweep_row_pairs import CLASSES, _assert_same_bits, _family, _run

LENGTHS = (1, 2, 3, 8, 9, 64, 65, 149, 150, 400)
ORACLE_CLASS = SG_CLASS = 16
DEGEN_LO, DEGEN_HI = 4, 15                # DNA: K = 4, Kp = 18; the last three codes are gap-like


def _degenerate_rows(L, n):
    """0-based positions of the degenerate codes of the n-th length."""
    eighth = list(range(7, L, 8))
    return [[0], [L - 1], [L // 2 - 1, L // 2] if L > 2 else [0, 1], eighth or [L - 1], [0, L - 1] + eighth][n % 5]


def _queries(fam, cells):
    """(queries, indices of those that hold degenerate codes)."""
    from witch_amd import synth
    rng = np.random.default_rng(1100 + cells)
    seqs, degen = [], []
    for n, L in enumerate(LENGTHS):
        s = synth.make_queries(fam, 140 + n, 1, L)[1][0].astype(np.uint8)
        seqs.append(s)
        d = s.copy()
        rows = [r for r in _degenerate_rows(L, n) if 0 <= r < L]
        d[rows] = rng.integers(DEGEN_LO, DEGEN_HI, size=len(rows)).astype(np.uint8)
        degen.append(len(seqs))
        seqs.append(d)
    degen.append(len(seqs))
    seqs.append(rng.integers(DEGEN_LO, DEGEN_HI, size=40).astype(np.uint8))                  # degenerate throughout
    frag = synth.make_queries(fam, 160, 1, 71, sub_rate=0.0)[1][0].astype(np.uint8)
    two = np.concatenate([frag, rng.integers(0, 4, size=12).astype(np.uint8), frag])
    two[[30, 31, 71 + 12 + 40]] = rng.integers(DEGEN_LO, DEGEN_HI, size=3).astype(np.uint8)
    degen.append(len(seqs))
    seqs.append(two)
    assert len(seqs) == 22
    return seqs, degen


def test_inputs_on_the_oracle(tmp_path):
    """(CPU) On the reference arithmetic these inputs give envelopes of odd and of even length and pairs with several
    envelopes in every class, and degenerate codes fall inside envelopes."""
    from oracle import oracle as orc
    for cells in sorted(CLASSES):
        fam, eh = _family(cells, str(tmp_path / str(cells)))
        ohm = [orc.OracleHMM(p) for p in eh.paths]
        seqs, degen = _queries(fam, cells)
        lens, several, inside = [], 0, 0
        for n, s in enumerate(seqs):
            for h in ohm:
                r = h.score(s)
                lens += [r.env_j[e] - r.env_i[e] + 1 for e in range(r.nenv)]
                several += r.nenv > 1
                inside += sum(bool((s[r.env_i[e] - 1:r.env_j[e]] >= DEGEN_LO).any()) for e in range(r.nenv)) if n in degen else 0
        lens = np.array(lens)
        print("\n[%d cells] %d envelopes, %d odd, %d even, shortest %d, pairs with several %d, envelopes with a degenerate code %d"
              % (cells, len(lens), (lens % 2 == 1).sum(), (lens % 2 == 0).sum(), lens.min(), several, inside))
        assert (lens % 2 == 1).any() and (lens % 2 == 0).any() and several > 0 and inside > 0, cells


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{cells: (default, slot)}, {("nores", cells): ...} without the resolver, {"sg": ...} with the special states in HBM, and
    {"oracle": (hmm paths, degenerate queries, default)} for the oracle's class; each run = (deci, flags, fwd, detail, paths)."""
    _need_gpu()
    from witch_amd.ehmm import EHMM
    out = {}
    for cells in sorted(CLASSES):
        fam, eh = _family(cells, str(tmp_path_factory.mktemp("w%d" % cells)))
        e = EHMM(eh.paths, hmm_index=eh.index, nseq=eh.nseq)
        assert all(4 * -(-int(m) // 256) == cells for m in e.M), (cells, list(e.M))
        seqs, degen = _queries(fam, cells)
        res = [[s_ for s_ in seqs if len(s_) < 300], [s_ for s_ in seqs if len(s_) >= 300]]
        out[cells] = (_run(e, res, "7"), _run(e, res, "8"))
        e.set_option("WH_NO_RESOLVE", "1")
        try:
            out[("nores", cells)] = (_run(e, res, "7"), _run(e, res, "8"))
        finally:
            e.set_option("WH_NO_RESOLVE", "")
        if cells == SG_CLASS:
            e.set_option("WH_FORCE_SPECG", "1")
            try:
                out["sg"] = (_run(e, res, "7"), _run(e, res, "8"))
            finally:
                e.set_option("WH_FORCE_SPECG", "")
        if cells == ORACLE_CLASS:
            dq = [seqs[n] for n in degen]
            out["oracle"] = (list(eh.paths), dq, _run(e, [dq], "7"))
        e.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("cells", sorted(CLASSES))
def test_same_bits_as_the_ab_slot(runs, cells):
    new, old = runs[cells]
    print("\n[%d cells] paths %s" % (cells, new[4]))
    _assert_same_bits(new, old, cells)


@pytest.mark.gpu
@pytest.mark.parametrize("cells", sorted(CLASSES))
def test_same_bits_without_the_resolver(runs, cells):
    """A query of two or three residues is one envelope of two or three rows here: the sweeps' first and last rows only."""
    new, old = runs[("nores", cells)]
    print("\n[%d cells, no resolver] paths %s" % (cells, new[4]))
    _assert_same_bits(new, old, ("nores", cells))
    d = new[3]
    lens = (d["env_j"] - d["env_i"] + 1)[np.arange(d["domcorr"].shape[1])[None, :] < d["nenv"][:, None]]
    assert (lens == 2).any() and (lens == 3).any(), sorted(set(lens.tolist()))[:6]


@pytest.mark.gpu
def test_same_bits_with_special_states_in_hbm(runs):
    new, old = runs["sg"]
    print("\n[WH_FORCE_SPECG] paths %s" % (new[4],))
    _assert_same_bits(new, old, "sg")


@pytest.mark.gpu
def test_both_window_widths_ran(runs):
    for side in (0, 1):
        tot = {}
        for cells in CLASSES:
            for key, val in runs[cells][side][4].items():
                tot[key] = tot.get(key, 0) + val
        print("\n%s: %s" % ("slot" if side else "default", tot))
        assert tot["window256"] > 0 and tot["window512"] > 0, tot


@pytest.mark.gpu
def test_degenerate_queries_against_the_oracle(runs):
    """Flags equal, Forward log-odds within 1e-4 bit, deci-bits under the rounding-boundary rule (0.02 bit for multidomain
    pairs): the tolerances of tests/test_gpu_parity.py."""
    from oracle import oracle as orc
    from witch_amd.ehmm import pack_queries
    paths, dq, (deci, flags, fwd, _, _) = runs["oracle"]
    ohm = [orc.OracleHMM(p) for p in paths]
    od, of, ofwd, osc = orc.score_batch(ohm, *pack_queries(dq))
    deci, flags, fwd = deci.reshape(od.shape), flags.reshape(of.shape), fwd.reshape(ofwd.shape)
    fin = np.isfinite(ofwd)
    assert np.array_equal(np.isfinite(fwd), fin)
    print("\nmax |Forward - oracle| = %.3g bit over %d pairs, %d reported" % (np.max(np.abs(fwd[fin] - ofwd[fin])), fin.sum(), (of & 1).sum()))
    assert np.max(np.abs(fwd[fin] - ofwd[fin])) <= 1e-4
    assert np.array_equal(flags & 3, of & 3)
    assert (of & 1).any()
    for q, h in np.argwhere((of & 1) == 1):
        _check_one_decibit(deci[q, h], od[q, h], osc[q, h], ("degenerate", int(q), int(h)), eps=0.02 if of[q, h] & 2 else BOUNDARY_EPS)
