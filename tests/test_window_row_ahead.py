"""The node-window sweeps of the default scoring kernel with a row's residue code and emission piece requested ahead
(WH_ROW_AHEAD, wh_score7.hip) against the A/B slot, which keeps the parent's rows (WH_SCORE_KERNEL=8, K7B_FLAGS: WH_ROW_AHEAD=0).

The change moves loads and waits, never an operand or the order of a sum: every output must be the same BITS - deci-bits,
flags, Forward scores, regions, envelopes, envelope scores and domain corrections.  A row now enters with its residue code in
a scalar register (read two rows earlier, at a clamped index) and with the LDS emission piece of that code in registers
(requested by the row before, for a canonical stand-in where the code is degenerate: that row takes the L2 branch and ignores
the piece).  So the lengths are the prologue of a two-deep and a one-deep pipeline - 1, 2, 3, 4, 5: with fewer rows than stages
every clamped dummy read runs - then 63, 64, 65, 150, and 400 for the 512-node window; and each length comes canonical and with
degenerate codes (4..14 for DNA) at rows 1 and 2 (the first two consumers), at the last two rows (the first two requests), at
two adjacent rows in the middle (a fallback row right after a prefetched one, and the reverse), and at every row.  One two-copy
query: envelopes that begin after row 1.  Everything again with WH_NO_RESOLVE (a query of 2 to 5 residues is then one envelope
of as many rows).  One small family per register class (8 to 24 cells per lane, the families of tests/test_sweep_row_pairs.py),
two models, 51 queries.  The per-pair path record must show the windowed multihit sweep and the 256-node envelope window on
pairs of every class and the 512-node window on the 16-cell class: otherwise nothing was compared."""
import numpy as np
import pytest

from tests.test_gpu_parity import _need_gpu
from tests.test_sweep_row_pairs import CLASSES, _assert_same_bits, _family, _run

LENGTHS = (1, 2, 3, 4, 5, 63, 64, 65, 150, 400)
DEGEN_LO, DEGEN_HI = 4, 15                # DNA: K = 4, Kp = 18; the last three codes are gap-like
P2_WIN, P4_W256, P4_W512 = 1, 4, 8        # WH_PATH_* (include/witch_hip.h)
W512_CLASS = 16


def _degenerate_rows(L):
    """0-based positions of the degenerate codes of the four variants of a length."""
    mid = max(L // 2, 1)
    return [[0, 1], [L - 2, L - 1], [mid - 1, mid], list(range(L))]


def _queries(fam, cells):
    """(queries, indices of those that hold degenerate codes, index of the two-copy query)."""
    from witch_amd import synth
    rng = np.random.default_rng(1200 + cells)
    seqs, degen = [], []
    for n, L in enumerate(LENGTHS):
        s = synth.make_queries(fam, 240 + n, 1, L)[1][0].astype(np.uint8)
        seqs.append(s)
        for rows in _degenerate_rows(L):
            rows = sorted(set(r for r in rows if 0 <= r < L))
            d = s.copy()
            d[rows] = rng.integers(DEGEN_LO, DEGEN_HI, size=len(rows)).astype(np.uint8)
            degen.append(len(seqs))
            seqs.append(d)
    frag = synth.make_queries(fam, 260, 1, 71, sub_rate=0.0)[1][0].astype(np.uint8)
    two = np.concatenate([frag, rng.integers(0, 4, size=12).astype(np.uint8), frag])
    two[[30, 31, 71 + 12 + 40]] = rng.integers(DEGEN_LO, DEGEN_HI, size=3).astype(np.uint8)
    seqs.append(two)
    assert len(seqs) == 51
    return seqs, degen, len(seqs) - 1


def test_inputs_on_the_oracle(tmp_path):
    """(CPU) On the reference arithmetic these inputs give, in every class: envelopes that begin after row 1, degenerate codes
    inside envelopes and, without the resolver, envelopes of 2, 3, 4 and 5 rows."""
    from oracle import oracle as orc
    for cells in sorted(CLASSES):
        fam, eh = _family(cells, str(tmp_path / str(cells)))
        ohm = [orc.OracleHMM(p) for p in eh.paths]
        seqs, degen, two = _queries(fam, cells)
        late, inside = 0, 0
        for n, s in enumerate(seqs):
            if len(s) > 160 or (n not in degen and n != two and len(s) > 5):
                continue                                   # (the oracle is slow: the long canonical queries add nothing here)
            for h in ohm:
                r = h.score(s)
                late += sum(r.env_i[e] > 1 for e in range(r.nenv))
                inside += sum(bool((s[r.env_i[e] - 1:r.env_j[e]] >= DEGEN_LO).any()) for e in range(r.nenv)) if n in degen else 0
        short = set()
        orc.set_resolve_multidomain(False)       # (the whole multidomain region is one envelope: WH_NO_RESOLVE on the GPU)
        try:
            for s in seqs:
                if 2 <= len(s) <= 5:
                    for h in ohm:
                        r = h.score(s)
                        short |= {int(r.env_j[e] - r.env_i[e] + 1) for e in range(r.nenv)}
        finally:
            orc.set_resolve_multidomain(True)
        print("\n[%d cells] envelopes that begin after row 1: %d, with a degenerate code: %d, row counts without the resolver: %s" % (cells, late, inside, sorted(short)))
        assert late > 0 and inside > 0 and short >= {2, 3, 4, 5}, (cells, late, inside, sorted(short))


def _paths(e, batches):
    """The 16-bit path record of the default object on the same batches, all pairs joined."""
    import torch
    from witch_amd.ehmm import pack_queries
    recs = []
    for seqs in batches:
        rec = torch.zeros((len(seqs), len(e.M)), dtype=torch.int16, device="cuda")
        e.set_path_buffer16(rec)
        try:
            e.score(*pack_queries(seqs))
        finally:
            e.set_path_buffer16(None)
        recs.append(rec.cpu().numpy().astype(np.int32).ravel() & 0xFFFF)
    return np.concatenate(recs)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{cells: (default, slot, path record)}, {("nores", cells): (default, slot)} without the resolver; each run = (deci, flags,
    fwd, detail, path counters)."""
    _need_gpu()
    from witch_amd.ehmm import EHMM
    out = {}
    for cells in sorted(CLASSES):
        fam, eh = _family(cells, str(tmp_path_factory.mktemp("a%d" % cells)))
        e = EHMM(eh.paths, hmm_index=eh.index, nseq=eh.nseq)
        assert all(4 * -(-int(m) // 256) == cells for m in e.M), (cells, list(e.M))
        seqs = _queries(fam, cells)[0]
        res = [[s_ for s_ in seqs if len(s_) < 300], [s_ for s_ in seqs if len(s_) >= 300]]
        assert len(res[0]) == 46 and len(res[1]) == 5
        out[cells] = (_run(e, res, "7"), _run(e, res, "8"), _paths(e, res))
        e.set_option("WH_NO_RESOLVE", "1")
        try:
            out[("nores", cells)] = (_run(e, res, "7"), _run(e, res, "8"))
        finally:
            e.set_option("WH_NO_RESOLVE", "")
        e.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("cells", sorted(CLASSES))
def test_same_bits_as_the_ab_slot(runs, cells):
    new, old, _ = runs[cells]
    print("\n[%d cells] paths %s" % (cells, new[4]))
    _assert_same_bits(new, old, cells)
    d = new[3]
    first = d["env_i"][np.arange(d["domcorr"].shape[1])[None, :] < d["nenv"][:, None]]
    assert (first > 1).any(), cells                                              # envelopes that begin after row 1


@pytest.mark.gpu
@pytest.mark.parametrize("cells", sorted(CLASSES))
def test_same_bits_without_the_resolver(runs, cells):
    """A query of 2 to 5 residues is one envelope of as many rows here: sweeps shorter than the pipelines are deep."""
    new, old = runs[("nores", cells)]
    print("\n[%d cells, no resolver] paths %s" % (cells, new[4]))
    _assert_same_bits(new, old, ("nores", cells))
    d = new[3]
    lens = (d["env_j"] - d["env_i"] + 1)[np.arange(d["domcorr"].shape[1])[None, :] < d["nenv"][:, None]]
    assert set(lens.tolist()) >= {2, 3, 4, 5}, sorted(set(lens.tolist()))[:8]


@pytest.mark.gpu
@pytest.mark.parametrize("cells", sorted(CLASSES))
def test_the_window_sweeps_ran(runs, cells):
    """The per-pair record of the default object: without these paths the comparison above compared nothing."""
    rec = runs[cells][2]
    n = {name: int(((rec & bit) != 0).sum()) for name, bit in (("P2_WIN", P2_WIN), ("P4_W256", P4_W256), ("P4_W512", P4_W512))}
    print("\n[%d cells] pairs by path: %s of %d" % (cells, n, rec.size))
    assert n["P2_WIN"] > 0 and n["P4_W256"] > 0, (cells, n)
    if cells == W512_CLASS:
        assert n["P4_W512"] > 0, (cells, n)
