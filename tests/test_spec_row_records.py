"""Row records and the compile-time unihit sweeps of the default scoring kernel against the A/B slot.

The default object of wh_score7.hip keeps a wave's per-row special states as one 6-word record per row and builds the
unihit length model into its envelope sweeps; the A/B slot (WH_SCORE_KERNEL=8) is the same source with the six arrays
and the run-time length model (K7B_FLAGS in witch_amd/csrc/Makefile).  Both changes are exact - the same six words
stored elsewhere, and operations that multiply by 0 or 1 or add a stored 0 - so every output must be the same BITS:
deci-bits, flags, Forward bits, every field of the detail records, and the path counters.

One small synthetic family per size class (4, 8, 16, 20, 24 cells per lane: no window and no band at 4, the in-place
window sweep with its HBM backup at 20 and 24), queries whose lengths straddle the 64-row chunks of the region scans
(1, 2, 63, 64, 65, 128, 129, 150), a two-copy query (several envelopes), a random one (none), an empty one and one with
a degenerate code; once with the defaults, once without the windowed multihit sweep (WH_NO_P2WIN) and once with the
envelope rows stored at full width (WH_SPILL_BAND=0).  The counters summed over the models prove that window,
full-width and band paths all ran, so the comparison cannot pass by every pair taking one path."""
import numpy as np
import pytest

from tests.test_gpu_parity import _need_gpu

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 63, 64, 65, 128, 129, 150)
# cells per lane -> root length of the family (a model of M nodes has 4 * ceil(M / 256) cells per lane)
CLASSES = {4: 200, 8: 450, 16: 900, 20: 1200, 24: 1450}
BAND_KEPT = 1 << 8                       # WH_PATH_BAND_KEPT (include/witch_hip.h)
SCALARS = ("fwd_bits", "seq_score", "pre_score", "seqbias_nats", "nregions", "nenv")
PER_ENVELOPE = ("env_i", "env_j", "envsc", "domcorr")

KNOBS = (None, "WH_NO_P2WIN", "WH_SPILL_BAND")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _queries(e, fam, cells):
    from witch_amd import synth
    rng = np.random.default_rng(500 + cells)
    seqs = []
    for n, L in enumerate(LENGTHS):
        seqs.append(synth.make_queries(fam, 40 + n, 1, L)[1][0].astype(np.uint8))
    seqs += [s_.astype(np.uint8) for s_ in synth.make_queries(fam, 60, 12, 150)[1]]       # more pairs than one workgroup has waves
    frag = synth.make_queries(fam, 61, 1, 70)[1][0].astype(np.uint8)
    seqs.append(np.concatenate([frag, rng.integers(0, 4, size=10).astype(np.uint8), frag]))   # two copies
    seqs.append(rng.integers(0, 4, size=120).astype(np.uint8))                               # unrelated
    seqs.append(np.zeros(0, dtype=np.uint8))                                                 # empty
    text = synth.to_text(synth.make_queries(fam, 62, 1, 100)[1][0], "dna")
    seqs.append(e.digitize(text[:50] + "N" + text[51:]))                                      # a degenerate code
    assert seqs[-1].max() >= 4
    return seqs


def _run(e, res, offs, slot):
    import torch
    rec = torch.zeros((len(offs) - 1, e.H), dtype=torch.int16, device="cuda")
    e.set_option("WH_SCORE_KERNEL", slot)
    e.set_path_buffer16(rec)
    try:
        deci, flags, fwd, det = e.score(res, offs, want_fwd=True, want_detail=True)
        paths = e.last_score_paths()
    finally:
        e.set_path_buffer16(None)
        e.set_option("WH_SCORE_KERNEL", "")
    return deci, flags, fwd, np.ctypeslib.as_array(det).copy(), paths, rec.cpu().numpy().astype(np.int32) & 0xFFFF


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Every class scored by both slots under the three settings, once for the tests below:
    {(cells, knob): (default slot, A/B slot)}; each side = (deci, flags, fwd, detail, path counters, path record)."""
    _need_gpu()
    from witch_amd import synth
    from witch_amd.ehmm import EHMM, pack_queries
    out = {}
    for cells, root_len in sorted(CLASSES.items()):
        fam = synth.make_family(8100 + cells, root_len, 8, "dna", 0.03, 1e-4)
        eh = synth.make_ehmm(fam, 2, str(tmp_path_factory.mktemp("m%d" % cells)), witch_layout=False)
        e = EHMM(eh.paths, hmm_index=eh.index, nseq=eh.nseq)
        assert all(4 * -(-int(m) // 256) == cells for m in e.M), (cells, list(e.M))
        res, offs = pack_queries(_queries(e, fam, cells))
        for knob in KNOBS:
            if knob:
                e.set_option(knob, "1" if knob == "WH_NO_P2WIN" else "0")
            try:
                out[(cells, knob)] = (_run(e, res, offs, "7"), _run(e, res, offs, "8"))
            finally:
                if knob:
                    e.set_option(knob, "")
        e.close()
    return out


@pytest.mark.parametrize("knob", KNOBS, ids=lambda k: k or "defaults")
@pytest.mark.parametrize("cells", sorted(CLASSES))
def test_row_records_equal_the_arrays_of_the_ab_slot(runs, cells, knob):
    new, old = runs[(cells, knob)]
    ctx = (cells, knob)
    print("\n[%d cells, %s] paths %s" % (cells, knob or "defaults", new[4]))
    assert np.array_equal(new[0], old[0]), ctx                                   # deci-bits
    assert np.array_equal(new[1], old[1]), ctx                                   # flags
    assert np.array_equal(_bits(new[2]), _bits(old[2])), ctx                     # Forward bits
    dn, do = new[3], old[3]
    for name in SCALARS:
        assert np.array_equal(_bits(dn[name]), _bits(do[name])), ctx + (name,)
    used = np.arange(dn["domcorr"].shape[1])[None, :] < dn["nenv"][:, None]
    for name in PER_ENVELOPE:
        assert np.array_equal(_bits(dn[name])[used], _bits(do[name])[used]), ctx + (name,)
    assert new[4] == old[4], ctx                                                 # the same path for every sweep
    assert np.array_equal(new[5], old[5]), ctx                                   # ... pair by pair
    assert (new[1] & 1).any(), ctx                                               # pairs were reported at all
    if knob == "WH_NO_P2WIN":
        assert new[4]["p2_window"] == 0, ctx
    if knob == "WH_SPILL_BAND":
        assert not (new[5] & BAND_KEPT).any(), ctx
    if cells == 4:
        assert new[4]["window256"] + new[4]["window512"] + new[4]["p2_window"] == 0 and not (new[5] & BAND_KEPT).any(), ctx


def test_every_path_ran(runs):
    """Window, full-width and band paths were all taken, by envelope and by multihit sweeps, and some pair had several envelopes."""
    tot = {}
    for (cells, knob), (new, old) in runs.items():
        for key, val in new[4].items():
            tot[key] = tot.get(key, 0) + val
        tot["band_kept"] = tot.get("band_kept", 0) + int(((new[5] & BAND_KEPT) != 0).sum())
        tot["multi_env"] = tot.get("multi_env", 0) + int((new[3]["nenv"] > 1).sum())
        if cells >= 20 and knob is None:
            tot["p2_window_in_place"] = tot.get("p2_window_in_place", 0) + new[4]["p2_window"]
    print("\npaths over all classes:", tot)
    assert tot["window256"] + tot["window512"] > 0 and tot["full_width"] > 0, tot
    assert tot["p2_window"] > 0 and tot["p2_window_in_place"] > 0, tot
    assert tot["band_kept"] > 0 and tot["multi_env"] > 0, tot
