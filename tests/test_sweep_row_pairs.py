"""Two rows per loop trip and scalar sweep arguments of the default scoring kernel against the A/B slot, and the per-split
slack of the certified region scan against the full-width multihit sweep.

The default object of wh_score7.hip walks the envelope window sweep two rows per trip (two register sets for the prefetched
Forward cells, swapped between the rows; an odd row count ends in a trip without its second row) and moves the wave-uniform
arguments of its sweeps to scalar registers; the A/B slot (WH_SCORE_KERNEL=8, K7B_FLAGS: WH_ROW_PAIRS=0) keeps the one-row
loops and the vector-register arguments.  Neither changes an operand or the order of a sum, so every output must be the same
BITS.  The multidomain test of the certified scan bounds each split point with the rows its own two sums run over: a window
is certified more often, and a certified scan's regions are still those of the full-width sweep (WH_NO_P2WIN), decision by
decision.

One small synthetic family per register class (8, 12, 16, 20, 24 cells per lane), 40 queries each: 1-5 residues (a trip
whose second row is absent, sweeps shorter than one trip), 7-9 (the eighth-row mask sample of the multihit Forward sweep),
63-65 (the 64-row chunks of the region scan), 149 / 150 (the headline's shape, odd and even), 300-450 (more than 256 nodes:
the 512-node window on the 16- and 24-cell models), two-copy queries (several envelopes of odd and even length in one pair;
multidomain regions).  A query of two or three residues is one multidomain region, which the resolver takes: a run with
WH_NO_RESOLVE=1 scores it as ONE envelope of two or three rows through the sweeps.  The long-query instantiation runs on one
class with seven queries.  test_inputs_on_the_oracle checks on the CPU that the envelopes of these inputs have both parities
and, without the resolver, that some have at most three rows."""
import numpy as np
import pytest

from tests.test_gpu_parity import _need_gpu

SHORT = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 149, 150)
LONG = (300, 351, 400, 450)
COPY = (69, 70, 71, 72, 40, 41)          # fragment length of the two-copy queries
# cells per lane -> root length of the family (a model of M nodes has 4 * ceil(M / 256) cells per lane)
CLASSES = {8: 450, 12: 700, 16: 950, 20: 1250, 24: 1450}
SG_CLASS = 16
SCALARS = ("fwd_bits", "seq_score", "pre_score", "seqbias_nats", "nregions", "nenv")
PER_ENVELOPE = ("env_i", "env_j", "envsc", "domcorr")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _family(cells, outdir):
    from witch_amd import synth
    fam = synth.make_family(9100 + cells, CLASSES[cells], 8, "dna", 0.03, 1e-4)
    return fam, synth.make_ehmm(fam, 2, outdir, witch_layout=False)


def _queries(fam, cells):
    """40 queries (module docstring)."""
    from witch_amd import synth
    rng = np.random.default_rng(900 + cells)
    seqs = [synth.make_queries(fam, 40 + n, 1, L)[1][0].astype(np.uint8) for n, L in enumerate(SHORT + LONG)]
    for n, L in enumerate(COPY):
        frag = synth.make_queries(fam, 70 + n, 1, L, sub_rate=0.0)[1][0].astype(np.uint8)
        seqs.append(np.concatenate([frag, rng.integers(0, 4, size=10 + n).astype(np.uint8), frag]))
    seqs += [s_.astype(np.uint8) for s_ in synth.make_queries(fam, 80, 9, 150)[1]]
    seqs += [s_.astype(np.uint8) for s_ in synth.make_queries(fam, 81, 8, 149)[1]]
    assert len(seqs) == 40
    return seqs


def _long_queries(fam):
    """Seven queries for the long-query kernels (special states in HBM): odd, even and tiny row counts, a 512-node window,
    two copies, and one query too long for a wave's LDS block."""
    from witch_amd import synth
    rng = np.random.default_rng(77)
    seqs = [synth.make_queries(fam, 90 + n, 1, L)[1][0].astype(np.uint8) for n, L in enumerate((3, 149, 150, 400))]
    frag = synth.make_queries(fam, 95, 1, 71, sub_rate=0.0)[1][0].astype(np.uint8)
    seqs.append(np.concatenate([frag, rng.integers(0, 4, size=12).astype(np.uint8), frag]))
    core = synth.make_queries(fam, 96, 1, 151)[1][0].astype(np.uint8)
    for L in (2500, 1801):
        s = rng.integers(0, 4, size=L).astype(np.uint8)
        s[700:700 + len(core)] = core
        seqs.append(s)
    return seqs


def test_inputs_on_the_oracle(tmp_path):
    """(CPU) The envelopes the reference arithmetic finds on these inputs: odd and even row counts in every class, one of at
    most three rows somewhere, and pairs with several envelopes - the shapes the two-row loop can go wrong at."""
    from oracle import oracle as orc
    small = 0
    for cells in sorted(CLASSES):
        fam, eh = _family(cells, str(tmp_path / str(cells)))
        ohm = [orc.OracleHMM(p) for p in eh.paths]
        lens, several = [], 0
        for s in _queries(fam, cells):
            for h in ohm:
                r = h.score(s)
                lens += [r.env_j[e] - r.env_i[e] + 1 for e in range(r.nenv)]
                several += r.nenv > 1
        lens = np.array(lens)
        print("\n[%d cells] %d envelopes, %d odd, %d even, shortest %d, pairs with several %d" % (cells, len(lens), (lens % 2 == 1).sum(), (lens % 2 == 0).sum(), lens.min(), several))
        assert (lens % 2 == 1).sum() >= 5 and (lens % 2 == 0).sum() >= 5 and several > 0, cells
        orc.set_resolve_multidomain(False)       # (the whole multidomain region is one envelope: WH_NO_RESOLVE on the GPU)
        try:
            for s in _queries(fam, cells)[:5]:
                r = ohm[0].score(s)
                small += sum(r.env_j[e] - r.env_i[e] + 1 <= 3 for e in range(r.nenv))
        finally:
            orc.set_resolve_multidomain(True)
    assert small >= 2 * len(CLASSES), small


def _run(e, batches, slot):
    """The batches one after the other (the 300-450-residue queries are one of their own: with them in the batch a wave's LDS
    block has no room for the three rows of the windowed multihit sweep on the 8- to 16-cell models); results joined, counters added."""
    from witch_amd.ehmm import pack_queries
    e.set_option("WH_SCORE_KERNEL", slot)
    parts, paths = [], {}
    try:
        for seqs in batches:
            deci, flags, fwd, det = e.score(*pack_queries(seqs), want_fwd=True, want_detail=True)
            parts.append((deci, flags, fwd, np.ctypeslib.as_array(det).copy()))
            for key, val in e.last_score_paths().items():
                paths[key] = paths.get(key, 0) + val
    finally:
        e.set_option("WH_SCORE_KERNEL", "")
    return tuple(np.concatenate([p_[n] for p_ in parts]) for n in range(4)) + (paths,)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Every class scored once by the default object, by the A/B slot and by the default object without the windowed multihit
    sweep: {cells: (default, slot, full width)}, {("nores", cells): (default, slot)} without the resolver and {"sg": (default,
    slot)} for the long-query kernels; each = (deci, flags, fwd, detail, path counters)."""
    _need_gpu()
    from witch_amd.ehmm import EHMM
    out = {}
    for cells in sorted(CLASSES):
        fam, eh = _family(cells, str(tmp_path_factory.mktemp("m%d" % cells)))
        e = EHMM(eh.paths, hmm_index=eh.index, nseq=eh.nseq)
        assert all(4 * -(-int(m) // 256) == cells for m in e.M), (cells, list(e.M))
        seqs = _queries(fam, cells)
        res = [[s_ for s_ in seqs if len(s_) < 300], [s_ for s_ in seqs if len(s_) >= 300]]
        assert len(res[0]) == 36 and len(res[1]) == 4
        new, old = _run(e, res, "7"), _run(e, res, "8")
        e.set_option("WH_NO_P2WIN", "1")
        try:
            full = _run(e, res, "7")
        finally:
            e.set_option("WH_NO_P2WIN", "")
        out[cells] = (new, old, full)
        e.set_option("WH_NO_RESOLVE", "1")
        try:
            out[("nores", cells)] = (_run(e, res, "7"), _run(e, res, "8"))
        finally:
            e.set_option("WH_NO_RESOLVE", "")
        if cells == SG_CLASS:
            res = [_long_queries(fam)]
            e.set_option("WH_FORCE_SPECG", "1")                                  # (the short ones too: special states in HBM)
            try:
                out["sg"] = (_run(e, res, "7"), _run(e, res, "8"))
            finally:
                e.set_option("WH_FORCE_SPECG", "")
        e.close()
    return out


def _assert_same_bits(new, old, ctx):
    assert np.array_equal(new[0], old[0]), ctx                                   # deci-bits
    assert np.array_equal(new[1], old[1]), ctx                                   # flags
    assert np.array_equal(_bits(new[2]), _bits(old[2])), ctx                     # Forward bits
    dn, do = new[3], old[3]
    for name in SCALARS:
        assert np.array_equal(_bits(dn[name]), _bits(do[name])), (ctx, name)
    used = np.arange(dn["domcorr"].shape[1])[None, :] < dn["nenv"][:, None]
    for name in PER_ENVELOPE:
        assert np.array_equal(_bits(dn[name])[used], _bits(do[name])[used]), (ctx, name)
    assert new[4] == old[4], (ctx, new[4], old[4])                               # the same path for every sweep
    assert (new[1] & 1).any(), ctx                                               # pairs were reported at all


@pytest.mark.gpu
@pytest.mark.parametrize("cells", sorted(CLASSES))
def test_row_pairs_equal_the_one_row_loops_of_the_ab_slot(runs, cells):
    new, old, _ = runs[cells]
    print("\n[%d cells] paths %s" % (cells, new[4]))
    _assert_same_bits(new, old, cells)
    lens = (new[3]["env_j"] - new[3]["env_i"] + 1)[np.arange(new[3]["domcorr"].shape[1])[None, :] < new[3]["nenv"][:, None]]
    assert (lens % 2 == 1).any() and (lens % 2 == 0).any(), cells


@pytest.mark.gpu
@pytest.mark.parametrize("cells", sorted(CLASSES))
def test_row_pairs_on_envelopes_of_two_and_three_rows(runs, cells):
    """Without the resolver the queries of two and three residues are one envelope each: sweeps shorter than one trip, and a
    trip without its second row."""
    new, old = runs[("nores", cells)]
    print("\n[%d cells, no resolver] paths %s" % (cells, new[4]))
    _assert_same_bits(new, old, ("nores", cells))
    d = new[3]
    lens = (d["env_j"] - d["env_i"] + 1)[np.arange(d["domcorr"].shape[1])[None, :] < d["nenv"][:, None]]
    assert (lens == 2).any() and (lens == 3).any(), sorted(set(lens.tolist()))[:6]


@pytest.mark.gpu
def test_row_pairs_long_query_kernels(runs):
    new, old = runs["sg"]
    print("\n[long queries] paths %s" % (new[4],))
    _assert_same_bits(new, old, "sg")
    assert new[4]["window256"] + new[4]["window512"] > 0, new[4]


@pytest.mark.gpu
def test_every_new_loop_ran(runs):
    """Over the whole set, and equally for both objects: both window widths of the envelope sweep, the windowed multihit sweep,
    and windows whose scan ended in doubt."""
    for side in (0, 1):
        tot = {}
        for cells in CLASSES:
            for key, val in runs[cells][side][4].items():
                tot[key] = tot.get(key, 0) + val
        print("\n%s: %s" % ("slot" if side else "default", tot))
        assert tot["window256"] > 0 and tot["window512"] > 0, tot
        assert tot["p2_window"] > 0 and tot["p2_window_in_doubt"] > 0, tot


@pytest.mark.gpu
@pytest.mark.parametrize("cells", sorted(CLASSES))
def test_per_split_slack_keeps_the_regions_of_the_full_width_sweep(runs, cells):
    win, _, full = runs[cells]
    assert full[4]["p2_window"] == 0 and full[4]["p2_window_in_doubt"] == 0, full[4]
    assert np.array_equal(win[1], full[1]), cells                                # flags (reported, multidomain, ...)
    assert np.array_equal(win[0], full[0]), cells                                # deci-bits
    dw, df = win[3], full[3]
    assert np.array_equal(dw["nregions"], df["nregions"]) and np.array_equal(dw["nenv"], df["nenv"]), cells
    used = np.arange(dw["domcorr"].shape[1])[None, :] < dw["nenv"][:, None]
    for name in ("env_i", "env_j"):
        assert np.array_equal(dw[name][used], df[name][used]), (cells, name)


@pytest.mark.gpu
def test_multidomain_regions_occur(runs):
    assert any((runs[cells][0][1] & 2).any() for cells in CLASSES)
    assert sum(runs[cells][0][4]["p2_window"] for cells in CLASSES) > 0
