"""Sixteen waves per workgroup (four per SIMD, wh_score7w.o) against the twelve-wave launch of the same handle.

For models of 8, 12 and 16 cells per lane the planner (wh_plan.h: plan_score_lds) can take sixteen waves where sixteen six-array
blocks fit beside the tables, with the multihit Backward window in place (ScoreArgs::p2win == 2): by default in the 16-cell
class, whose headline run it won, and under WH_MAX_WAVES=16 in the other two (FORCE_16 below).  WH_MAX_WAVES=12 plans and
launches what the library launched before: wh::k7::score_kernel7 at twelve waves, three more rows per wave (p2win == 1).  No
operand and no order of a sum differs between the two objects, so every output must be the same BITS: deci-bits, flags, Forward
scores, regions, envelopes, envelope scores and domain corrections, and the envelope bits of the per-pair path record (which
depend on the pair alone).  The P2 bits of the record may differ: whether a wave tries the window on a pair depends on the slack
it measured on ITS last two pairs of the model (FrontState, wh_score7.hip), and sixteen waves deal the pairs differently - both
ways give the full-width sweep's regions.  What the test asserts about them is that the same pairs reached the sweep at all; it
prints the counts.

Shapes, per class (the families of tests/test_sweep_row_pairs.py: 450, 700 and 950 nodes at the root): lengths 1 to 5, 63 to
65 and 150, canonical and with degenerate codes at the first row, the last row, two adjacent rows and every eighth row; fragments,
unrelated queries, two-copy queries (several envelopes, multidomain regions, windows whose scan ends in doubt and restores the
Forward sweep's rows from the copy); a batch smaller than one work item and one of 16 x 32 + 1 queries (the item edge); the
largest length at which sixteen waves fit the class, from the planner's formula restated here, and that length + 1, which must
run twelve.  The batch at the largest length of the 16-cell class holds fragments with eight to fifteen short deletions (one
envelope over 220 to 245 nodes): more than 256 nodes under a window's margins, the 512-node windows - the one sweep of the new object whose row loop spills.  Everything with
and without the resolver.  A subset is checked against the float64 oracle by the rule of smoke().  The test compares results."""
import numpy as np
import pytest

from tests.test_gpu_parity import _need_gpu
from tests.test_sweep_row_pairs import PER_ENVELOPE, SCALARS, _bits, _family

CELLS = (8, 12, 16)
FORCE_16 = (8, 12)                        # classes that do not take sixteen waves by default: asked for with WH_MAX_WAVES=16
K_DNA = 4
DEGEN_LO, DEGEN_HI = 4, 15                # DNA: K = 4, Kp = 18; the last three codes are gap-like
P2_WIN, P2_FULL, P4_W256, P4_W512 = 1, 2, 4, 8      # WH_PATH_* (include/witch_hip.h)
ENVELOPE_COUNTERS = ("window256", "window512", "window_rejected", "full_width")
# wh_plan.h: kLdsBudget, kLdsHeader, kScoreSpecArrays, kRegsInts (5 x WH_MAX_ENVELOPES), FW_NARR, kWave
LDS_BUDGET, LDS_HEADER, SPEC_ARRAYS, REGS_INTS, FW_NARR, WAVE = 160 * 1024 - 512, 16, 6, 80, 8, 64


def _lds_bytes(cells, L, waves, arrays):
    """lds_bytes(kLdsHeader, score_table_bytes(K, Q), waves, plan_block1's wave block) of wh_plan.h."""
    row_stride = (L + 1 + 3) // 4 * 4
    residue_words = (L + 3) // 4 + 4
    wave_words = arrays * row_stride + 32 + REGS_INTS + residue_words
    return LDS_HEADER + (K_DNA + 2 * FW_NARR) * cells * WAVE * 4 + waves * wave_words * 4


def _max_len_16(cells):
    L = 1
    while _lds_bytes(cells, L + 1, 16, SPEC_ARRAYS) <= LDS_BUDGET:
        L += 1
    return L


def test_planner_formula_restated():
    """(CPU) The headline's shape: sixteen six-array blocks fit a 16-cell DNA model at 150 residues, sixteen nine-array blocks do
    not, twelve do; the largest length of each class."""
    assert _lds_bytes(16, 150, 16, 6) == 16 + 81920 + 16 * 4264 <= LDS_BUDGET
    assert _lds_bytes(16, 150, 16, 9) > LDS_BUDGET >= _lds_bytes(16, 150, 12, 9)
    caps = {cells: _max_len_16(cells) for cells in CELLS}
    print("\nlargest length with sixteen waves: %s" % caps)
    assert caps[16] == 183 and caps[8] > caps[12] > caps[16]


def _with_degenerate(rng, s, rows):
    d = s.copy()
    rows = sorted(set(r for r in rows if 0 <= r < len(s)))
    d[rows] = rng.integers(DEGEN_LO, DEGEN_HI, size=len(rows)).astype(np.uint8)
    return d


def _with_deletions(leaf, start, L, n_del, size):
    """L residues of <leaf> from <start> on with <n_del> runs of <size> residues left out at equal distances: one alignment
    over L + n_del x size nodes."""
    piece = L // (n_del + 1)
    parts, at = [], start
    for n in range(n_del + 1):
        w = piece if n < n_del else L - piece * n_del
        parts.append(leaf[at:at + w])
        at += w + size
    return np.concatenate(parts).astype(np.uint8)


def _batches(fam, cells):
    """{name: queries}: main (up to 150 residues), small (5 queries), edge (513 short ones), fit (the largest sixteen-wave length),
    over (one residue more)."""
    from witch_amd import synth
    rng = np.random.default_rng(1600 + cells)
    main = []
    for n, L in enumerate((1, 2, 3, 4, 5, 63, 64, 65, 150)):
        s = synth.make_queries(fam, 300 + n, 1, L)[1][0].astype(np.uint8)
        main.append(s)
        if L in (5, 64, 150):
            mid = L // 2
            for rows in ([0], [L - 1], [mid - 1, mid], list(range(0, L, 8))):
                main.append(_with_degenerate(rng, s, rows))
    main += [s_.astype(np.uint8) for s_ in synth.make_queries(fam, 330, 24, 150)[1]]                 # fragments
    main += [s_.astype(np.uint8) for s_ in synth.make_queries(fam, 331, 12, (40, 149))[1]]
    main += [rng.integers(0, 4, size=int(L)).astype(np.uint8) for L in rng.integers(20, 151, size=10)]   # unrelated
    for n, L in enumerate((69, 70, 71, 72, 40, 41, 60, 55)):                                          # two copies
        frag = synth.make_queries(fam, 340 + n, 1, L, sub_rate=0.0)[1][0].astype(np.uint8)
        two = np.concatenate([frag, rng.integers(0, 4, size=3 + n).astype(np.uint8), frag])
        main.append(two[:150])
    assert 64 <= len(main) <= 128 and max(len(s_) for s_ in main) == 150, len(main)
    edge = [s_.astype(np.uint8) for s_ in synth.make_queries(fam, 350, 16 * 32 + 1, (30, 60))[1]]
    cap = _max_len_16(cells)
    leaf = fam.leaf_seq(0)
    wide = [_with_deletions(leaf, min(start, len(leaf) - cap - n_del * size - 1), cap, n_del, size)
            for start in (40, 300) for n_del, size in ((8, 5), (10, 5), (15, 4))]
    some = main[5:9] + main[21:33] + main[-4:]
    fit = some + wide + [synth.make_queries(fam, 360, 1, cap)[1][0].astype(np.uint8)]
    over = some + [synth.make_queries(fam, 361, 1, cap + 1)[1][0].astype(np.uint8)]
    assert max(len(s_) for s_ in fit) == cap and max(len(s_) for s_ in over) == cap + 1
    return {"main": main, "small": main[20:25], "edge": edge, "fit": fit, "over": over}


def _score(e, seqs):
    """One call: (deci, flags, fwd, detail, 16-bit path record, path counters, launch shapes)."""
    import torch
    from witch_amd.ehmm import pack_queries
    rec = torch.zeros((len(seqs), len(e.M)), dtype=torch.int16, device="cuda")
    e.set_path_buffer16(rec)
    try:
        deci, flags, fwd, det = e.score(*pack_queries(seqs), want_fwd=True, want_detail=True)
    finally:
        e.set_path_buffer16(None)
    return (deci, flags, fwd, np.ctypeslib.as_array(det).copy(), rec.cpu().numpy().astype(np.int32) & 0xFFFF, e.last_score_paths(), e.last_score_shapes())


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{(cells, resolver, batch): (sixteen-wave plan, WH_MAX_WAVES=12)}, {("oracle", cells): (queries, model files)}."""
    _need_gpu()
    from witch_amd.ehmm import EHMM
    out = {}
    for cells in CELLS:
        fam, eh = _family(cells, str(tmp_path_factory.mktemp("w%d" % cells)))
        e = EHMM(eh.paths, hmm_index=eh.index, nseq=eh.nseq)
        assert all(4 * -(-int(m) // 256) == cells for m in e.M), (cells, list(e.M))
        batches = _batches(fam, cells)
        out[("oracle", cells)] = (batches["main"], list(eh.paths))
        for resolver in (True, False):
            e.set_option("WH_NO_RESOLVE", "" if resolver else "1")
            for name, seqs in batches.items():
                e.set_option("WH_MAX_WAVES", "16" if cells in FORCE_16 else "")
                new = _score(e, seqs)
                e.set_option("WH_MAX_WAVES", "12")
                try:
                    ref = _score(e, seqs)
                finally:
                    e.set_option("WH_MAX_WAVES", "")
                out[(cells, resolver, name)] = (new, ref)
        e.close()
    return out


def _assert_same_results(new, ref, ctx):
    assert np.array_equal(new[0], ref[0]), ctx                                   # deci-bits
    assert np.array_equal(new[1], ref[1]), ctx                                   # flags
    assert np.array_equal(_bits(new[2]), _bits(ref[2])), ctx                     # Forward bits
    dn, do = new[3], ref[3]
    for name in SCALARS:
        assert np.array_equal(_bits(dn[name]), _bits(do[name])), (ctx, name)
    used = np.arange(dn["domcorr"].shape[1])[None, :] < dn["nenv"][:, None]
    for name in PER_ENVELOPE:
        assert np.array_equal(_bits(dn[name])[used], _bits(do[name])[used]), (ctx, name)
    # the path record: the envelope, band, dense and resolver bits are the pair's own; of the P2 bits, that the sweep ran
    p2 = P2_WIN | P2_FULL
    assert np.array_equal(new[4] & ~p2, ref[4] & ~p2), ctx
    assert np.array_equal((new[4] & p2) != 0, (ref[4] & p2) != 0), ctx
    for key in ENVELOPE_COUNTERS:
        assert new[5][key] == ref[5][key], (ctx, key, new[5], ref[5])


@pytest.mark.gpu
@pytest.mark.parametrize("resolver", (True, False))
@pytest.mark.parametrize("cells", CELLS)
def test_same_bits_as_twelve_waves(runs, cells, resolver):
    for name in ("main", "small", "edge", "fit", "over"):
        new, ref = runs[(cells, resolver, name)]
        print("\n[%d cells, resolver %d, %s] %d queries: shapes %s / %s; P2 window kept / in doubt: %d / %d against %d / %d; envelope paths %s"
              % (cells, resolver, name, new[0].shape[0], new[6], ref[6], new[5]["p2_window"], new[5]["p2_window_in_doubt"],
                 ref[5]["p2_window"], ref[5]["p2_window_in_doubt"], {k_: new[5][k_] for k_ in ENVELOPE_COUNTERS}))
        _assert_same_results(new, ref, (cells, resolver, name))
        if name != "small":
            assert (new[1] & 1).any(), (cells, resolver, name)                   # pairs were reported at all


@pytest.mark.gpu
@pytest.mark.parametrize("cells", CELLS)
def test_launch_shapes(runs, cells):
    """Sixteen waves in place up to the largest length that fits them, twelve (the plan as it was) one residue beyond, and the
    reference always twelve with its three more rows where they fit."""
    for name in ("main", "small", "edge", "fit"):
        new, ref = runs[(cells, True, name)]
        assert new[6] == [(cells, 16, 2)], (name, new[6])
        assert len(ref[6]) == 1 and ref[6][0][:2] == (cells, 12) and ref[6][0][2] in (0, 1), (name, ref[6])
    assert runs[(cells, True, "main")][1][6] == [(cells, 12, 1)]
    new, ref = runs[(cells, True, "over")]
    assert new[6] == ref[6] and new[6][0][0] == cells and new[6][0][1] <= 12 and new[6][0][2] != 2, (new[6], ref[6])


@pytest.mark.gpu
def test_the_paths_compared(runs):
    """Without these the comparison compared nothing: the in-place window kept and in doubt (rows restored from the copy), both
    envelope windows, the 512-node window - the spilling sweep - on the 16-cell class, several envelopes, multidomain regions."""
    tot = {}
    for cells in CELLS:
        for name in ("main", "fit"):
            new = runs[(cells, True, name)][0]
            for key, val in new[5].items():
                tot[key] = tot.get(key, 0) + val
            assert new[5]["p2_window"] > 0 and new[5]["window256"] > 0, (cells, name, new[5])
        main = runs[(cells, True, "main")][0]
        assert (main[3]["nenv"] > 1).any() and (main[1] & 2).any(), cells
    print("\nsixteen-wave runs, all classes: %s" % tot)
    assert tot["p2_window_in_doubt"] > 0, tot
    rec = runs[(16, True, "fit")][0][4]
    n512 = int(((rec & P4_W512) != 0).sum())
    print("16 cells, largest length: %d pairs with an envelope on the 512-node window" % n512)
    assert n512 > 0


@pytest.mark.gpu
@pytest.mark.parametrize("cells", CELLS)
def test_subset_against_the_oracle(runs, cells):
    """Flags and deci-bits of every fourth query of the main batch on the float64 oracle, by the rule of smoke(): one unit apart
    only when the oracle's score is within 0.002 bit (0.02 for the multidomain class) of a rounding boundary."""
    from oracle import oracle as orc
    from witch_amd.ehmm import pack_queries
    seqs, paths = runs[("oracle", cells)]
    pick = list(range(0, len(seqs), 4))
    new = runs[(cells, True, "main")][0]
    ohm = [orc.OracleHMM(p) for p in paths]
    od, of, _, osc = orc.score_batch(ohm, *pack_queries([seqs[n] for n in pick]))
    deci, flags = new[0][pick], new[1][pick]
    assert np.array_equal(flags & 3, of & 3), cells
    for q, h in np.argwhere((deci != od) & ((of & 1) == 1)):
        eps = 0.02 if of[q, h] & 2 else 0.002
        assert abs(int(deci[q, h]) - int(od[q, h])) == 1 and abs((abs(float(osc[q, h])) * 10.0) % 1.0 - 0.5) < eps * 10.0, (cells, q, h, deci[q, h], od[q, h], osc[q, h])
    assert (of & 1).any()
