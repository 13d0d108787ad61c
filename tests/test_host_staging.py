"""The host-pointer entry points stage their arrays through ONE set of slots in the handle (wh_host.h: Staging): every
slot serves a large array, then a small one, then a large one of another entry point's type, and every result must still be
the bytes of the matching *_dev entry point on torch tensors of its own (which never touch a staging slot).

On dna_synth (4 models of 152-156 nodes with STATS lines, 40 queries), one handle, three rounds: all 40 queries, the first
3, all 40 again.  Then: a residue code outside the alphabet is refused with its message and leaves the handle as it was, and
optional outputs left out leave the others equal."""
import ctypes as C

import numpy as np
import pytest

from tests.conftest import load_case

pytestmark = pytest.mark.gpu

BACKBONE = 400            # columns of the consensus backbone: more than the longest model has nodes


def _eq(what, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert got.tobytes() == want.tobytes(), what


def _pairs(e, idx, nu):
    """(query, model position) of the kept models of every query, in top-k order (as __graft_entry__.smoke)."""
    pq, ph = [], []
    for q in range(len(nu)):
        for r in range(int(nu[q])):
            pq.append(q)
            ph.append(e.pos_of_index[int(idx[q, r])])
    return np.asarray(pq, np.int64), np.asarray(ph, np.int32)


def _device_round(e, res, offs, k, retained, nongaps):
    """Every stage through the *_dev entry points, on tensors made here; all results as numpy arrays."""
    import torch
    from witch_amd._lib import PairDetail, check, lib
    from witch_amd.ehmm import EHMM
    dev = torch.device("cuda")
    L = lib()
    nq, H = len(offs) - 1, e.H
    maxlen = int(np.diff(offs).max())
    res_t, off_t = torch.from_numpy(res).to(dev), torch.from_numpy(offs).to(dev)
    st = e._stream()
    deci, flags, fwd = e.score_t(res_t, off_t, maxlen, want_fwd=True)
    det = torch.zeros(nq * H * C.sizeof(PairDetail), dtype=torch.uint8, device=dev)      # (score_t has no detail output)
    deci2, flags2 = torch.empty_like(deci), torch.empty_like(flags)
    check(L.wh_score_dev(e._h, res_t.data_ptr(), off_t.data_ptr(), nq, res_t.numel(), maxlen, deci2.data_ptr(), flags2.data_ptr(),
                         None, det.data_ptr(), st), "wh_score_dev")
    assert torch.equal(deci, deci2) and torch.equal(flags, flags2)
    idx, w, nk, nu = e.topk_t(deci, flags, k)
    pq, ph = _pairs(e, idx.cpu().numpy(), nu.cpu().numpy())
    co = np.zeros(len(pq) + 1, np.int64)
    co[1:] = np.cumsum(offs[pq + 1] - offs[pq])
    pq_t, ph_t, co_t = torch.from_numpy(pq).to(dev), torch.from_numpy(ph).to(dev), torch.from_numpy(co).to(dev)
    cols, pp = e.align_t(res_t, off_t, maxlen, pq_t, ph_t, co_t, int(co[-1]), want_pp=True)
    cols64 = torch.full((int(co[-1]),), -1, dtype=torch.int32, device=dev)
    pp64 = torch.zeros(int(co[-1]), dtype=torch.float64, device=dev)
    check(L.wh_align_pp64_dev(e._h, res_t.data_ptr(), off_t.data_ptr(), nq, res_t.numel(), maxlen, pq_t.data_ptr(), ph_t.data_ptr(),
                              len(pq), co_t.data_ptr(), cols64.data_ptr(), pp64.data_ptr(), st), "wh_align_pp64_dev")
    dom, dom_off, unl = e.domains_dev(res_t, off_t, maxlen, flags, det)
    o = EHMM.filter_opts(True, nobias=True)
    stage = torch.empty((nq, H), dtype=torch.uint8, device=dev)
    bias = torch.empty((nq, H), dtype=torch.float32, device=dev)
    msv, vit = torch.empty((nq, H), dtype=torch.int32, device=dev), torch.empty((nq, H), dtype=torch.int32, device=dev)
    check(L.wh_filter_dev(e._h, res_t.data_ptr(), off_t.data_ptr(), nq, res_t.numel(), maxlen, C.byref(o), stage.data_ptr(),
                          bias.data_ptr(), msv.data_ptr(), vit.data_ptr(), st), "wh_filter_dev")
    fdeci, fflags, fstage = torch.empty_like(deci), torch.empty_like(flags), torch.empty_like(stage)
    check(L.wh_score_filtered_dev(e._h, res_t.data_ptr(), off_t.data_ptr(), nq, res_t.numel(), maxlen, C.byref(o), fdeci.data_ptr(),
                                  fflags.data_ptr(), None, None, fstage.data_ptr(), st), "wh_score_filtered_dev")
    keep = torch.arange(k, device=dev)[None, :] < nu[:, None]
    pw = w[keep].contiguous()
    qpo = np.zeros(nq + 1, np.int64)
    qpo[1:] = np.cumsum(nu.cpu().numpy())
    ro = np.zeros(H + 1, np.int64)
    ro[1:] = np.cumsum([len(r) for r in retained])
    codes, mm = e.consensus_t(off_t, maxlen, torch.from_numpy(qpo).to(dev), ph_t, pw, co_t, cols, torch.from_numpy(ro).to(dev),
                              torch.from_numpy(np.concatenate(retained)).to(dev), torch.from_numpy(np.concatenate(nongaps)).to(dev),
                              BACKBONE, int(np.diff(qpo).max()))
    torch.cuda.synchronize()
    out = dict(deci=deci, flags=flags, fwd=fwd, det=det, idx=idx, w=w, nk=nk, nu=nu, cols=cols, pp=pp, cols64=cols64, pp64=pp64, dom=dom,
               dom_off=dom_off, unl=unl, stage=stage, bias=bias, msv=msv, vit=vit, fdeci=fdeci, fflags=fflags, fstage=fstage, codes=codes, mm=mm)
    out = {key: t.cpu().numpy() for key, t in out.items()}
    out.update(pq=pq, ph=ph, co=co, qpo=qpo, pw=pw.cpu().numpy())
    return out


def _host_round(e, res, offs, k, retained, nongaps, want):
    """The host-pointer entry points in the order that hands every slot from one array type to another, against <want>."""
    deci, flags, fwd, det = e.score(res, offs, want_fwd=True, want_detail=True)
    _eq("score: decibits", deci, want["deci"])
    _eq("score: flags", flags, want["flags"])
    _eq("score: fwd_bits", fwd, want["fwd"])
    _eq("score: detail", np.frombuffer(bytes(det), np.uint8), want["det"])
    idx, w, nk, nu = e.topk(deci, flags, k)
    for name, got in (("idx", idx), ("w", w), ("nk", nk), ("nu", nu)):
        _eq("topk: " + name, got, want[name])
    pq, ph = _pairs(e, idx, nu)
    _eq("pairs", pq, want["pq"])
    _eq("pairs", ph, want["ph"])
    cols, co, pp = e.align(res, offs, pq, ph, want_pp=True)
    _eq("align: col_offsets", co, want["co"])
    _eq("align_pp: cols", cols, want["cols"])
    _eq("align_pp: pp", pp, want["pp"])
    cols64, _, pp64 = e.align(res, offs, pq, ph, want_pp="float64")
    _eq("align_pp64: cols", cols64, want["cols64"])
    _eq("align_pp64: pp", pp64, want["pp64"])
    dom, dom_off, unl = e.domains(res, offs, flags, det, want_unlisted=True)
    _eq("domains: dom_off", dom_off, want["dom_off"])
    _eq("domains: n_unlisted", unl, want["unl"])
    _eq("domains: records", dom.view(np.uint8).reshape(len(dom), dom.dtype.itemsize), want["dom"])
    stage, bias, msv, vit = e.filter(res, offs, nobias=True, want_raw=True)
    for name, got in (("stage", stage), ("bias", bias), ("msv", msv), ("vit", vit)):
        _eq("filter: " + name, got, want[name])
    fdeci, fflags, fstage = e.score(res, offs, filters=True, nobias=True, want_stage=True)
    _eq("score_filtered: decibits", fdeci, want["fdeci"])
    _eq("score_filtered: flags", fflags, want["fflags"])
    _eq("score_filtered: stage", fstage, want["fstage"])
    codes, mm = e.consensus(offs, want["qpo"], ph, want["pw"], co, cols, retained, nongaps, BACKBONE)
    _eq("consensus: codes", codes, want["codes"])
    _eq("consensus: minmax", mm, want["mm"])
    return len(pq), len(dom)


def test_every_slot_serves_large_small_and_other_arrays():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from witch_amd._lib import WitchHipError
    from witch_amd.ehmm import EHMM, pack_queries
    case = load_case("dna_synth")
    e = EHMM(case.hmm_paths, hmm_index=case.hmm_index, nseq=case.nseq)
    try:
        assert e.H == 4 and len(case.qseqs) == 40
        seqs = [e.digitize(s) for s in case.qseqs]
        rng = np.random.default_rng(5)
        retained = [np.sort(rng.choice(BACKBONE, size=int(m), replace=False)).astype(np.int32) for m in e.M]
        nongaps = [rng.integers(1, 60, size=int(m)).astype(np.int32) for m in e.M]
        first = None
        for n in (40, 3, 40):
            res, offs = pack_queries(seqs[:n])
            want = _device_round(e, res, offs, case.k, retained, nongaps)
            npairs, ndom = _host_round(e, res, offs, case.k, retained, nongaps, want)
            assert npairs > 0 and ndom > 0 and (want["stage"] & 4).any(), "a stage of the round had nothing to do"
            if first is None:
                first = want
        for key in first:                       # the third round is the first again
            _eq("round 3: " + key, want[key], first[key])
        # a residue code outside the alphabet (Kp = 18 for DNA): refused before anything is staged, with its message
        bad = res.copy()
        bad[7] = 18
        with pytest.raises(WitchHipError) as ei:
            e.score(bad, offs, want_fwd=True, want_detail=True)
        assert "(-1)" in str(ei.value) and "residue code 18 at position 7 is not in the alphabet" in str(ei.value)
        deci, flags, fwd, det = e.score(res, offs, want_fwd=True, want_detail=True)
        _eq("after the refused call: decibits", deci, want["deci"])
        _eq("after the refused call: flags", flags, want["flags"])
        _eq("after the refused call: fwd_bits", fwd, want["fwd"])
        _eq("after the refused call: detail", np.frombuffer(bytes(det), np.uint8), want["det"])
        # optional outputs left out: the others are the same
        deci, flags, det = e.score(res, offs, want_detail=True)
        _eq("without fwd_bits: decibits", deci, want["deci"])
        _eq("without fwd_bits: flags", flags, want["flags"])
        _eq("without fwd_bits: detail", np.frombuffer(bytes(det), np.uint8), want["det"])
        stage, bias = e.filter(res, offs, nobias=True)
        _eq("without the raw scores: stage", stage, want["stage"])
        _eq("without the raw scores: bias", bias, want["bias"])
    finally:
        e.close()
