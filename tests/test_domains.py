"""Per-domain results on the GPU: wh_score then wh_domains (EHMM.domains) against the float64 reference of
tests/domains_reference.py and hmmsearch's --domtblout lines (tests/golden/domains).

Against the reference, on EVERY domain: index / of, envelope and hmm / ali coordinates identical; bits and bias_bits within
2e-3 bit (the float32 envsc of the scoring kernels is within 1e-4 bit of the oracle's on these cases; the rest is float32
rounding of sums of a few hundred nats); oasc / Ld within wh_align_pp's documented 2e-4 + 3e-6 Ld; lnP within lambda x 2e-3.
Against HMMER: the conditions of tests/test_domains_host.py for the strong stratum (its acc >= 0.95), the weak one counted.
"""
import os

import numpy as np
import pytest

from tests import domains_reference as dr
from tests.conftest import load_case

pytestmark = pytest.mark.gpu

BITS_TOL = 2e-3
INT_FIELDS = ("index", "of", "env_i", "env_j", "ali_i", "ali_j", "hmm_i", "hmm_j")


def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _run(paths, seqs, **kw):
    """Score and take the domains: (records, dom_off, n_unlisted, flags, detail, handle's H)."""
    from witch_amd.ehmm import EHMM, pack_queries
    e = EHMM(paths)
    try:
        res, offs = pack_queries(seqs)
        deci, flags, det = e.score(res, offs, want_detail=True)
        recs, dom_off, unl = e.domains(res, offs, flags, det, want_unlisted=True)
        return recs, dom_off, unl, flags, det, e.H
    finally:
        e.close()


def _by_pair(recs, dom_off, nq, H):
    out = {}
    for q in range(nq):
        for h in range(H):
            p = q * H + h
            rows = recs[dom_off[p]:dom_off[p + 1]]
            assert np.all(rows["pair"] == p)
            out[(q, h)] = [{k: r[k].item() for k in recs.dtype.names} for r in rows]
    return out


def _check_against_reference(tag, got, want, paths):
    """Every domain of every pair; returns their number."""
    from witch_amd.shim.formats import hmm_header
    lam = [hmm_header(p)["flambda"] for p in paths]
    worst = [0.0, 0.0, 0.0]
    n = 0
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        g, w = got[key], want[key]
        assert len(g) == len(w), (tag, key, len(g), len(w))
        for a, b in zip(g, w):
            assert [a[k] for k in INT_FIELDS] == [b[k] for k in INT_FIELDS], (tag, key, a, {k: b[k] for k in INT_FIELDS})
            Ld = b["env_j"] - b["env_i"] + 1
            d = (abs(a["bits"] - b["bits"]), abs(a["bias_bits"] - b["bias_bits"]), abs(a["oasc"] - b["oasc"]) / Ld)
            worst = [max(x, y) for x, y in zip(worst, d)]
            assert d[0] <= BITS_TOL and d[1] <= BITS_TOL, (tag, key, a, b["bits"], b["bias_bits"])
            assert d[2] <= 2e-4 + 3e-6 * Ld, (tag, key, a["oasc"] / Ld, b["oasc"] / Ld)
            if b["lnP"] != b["lnP"]:
                assert a["lnP"] != a["lnP"], (tag, key, "lnP of a model without a STATS line")
            else:
                assert a["lnP"] <= 0.0 and abs(a["lnP"] - b["lnP"]) <= abs(lam[key[1]]) * BITS_TOL + 1e-6 * abs(b["lnP"]), (tag, key, a["lnP"], b["lnP"])
            n += 1
    print("%s: %d domains, largest |bits - ref| %.2g, |bias - ref| %.2g, |acc - ref| %.2g" % (tag, n, *worst))
    return n


@pytest.mark.parametrize("name", dr.CASES)
def test_domains_against_reference_and_hmmer(name):
    _need_gpu()
    case = load_case(name)
    fx = dr.load_fixture(name)
    seqs, want = dr.case_reference(name)
    paths = case.hmm_paths[:len(fx["models"])]
    recs, dom_off, unl, flags, det, H = _run(paths, seqs)
    assert not unl.any()
    got = _by_pair(recs, dom_off, len(seqs), H)
    assert _check_against_reference(name, got, want, paths) > 0
    st = dr.compare_with_fixture(name, got, multi_from=want)
    assert st["strong"] > 0 and not st["strong_rule_misses"], st["strong_rule_misses"]
    assert dr.multi_class_ok(st), (st["multi"], st["multi_differ"], st["multi_two"])
    assert st["strong_acc_5e3"] >= 0.99 * st["strong"]


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    paths, names, seqs = dr.shapes_case(str(tmp_path_factory.mktemp("dom_shapes")))
    want, info = dr.reference_for(paths, seqs)
    return paths, names, seqs, want, info


def test_shapes_csr_edges_envelope_ends_overlap_resolver_and_lane_trips(shapes):
    _need_gpu()
    from witch_amd._lib import FLAG_MULTI, FLAG_REPORTED
    paths, names, seqs, want, info = shapes
    recs, dom_off, unl, flags, det, H = _run(paths, seqs)
    got = _by_pair(recs, dom_off, len(seqs), H)
    assert _check_against_reference("shapes", got, want, paths) > 0
    n = {k: len(v) for k, v in got.items()}
    q = {nm: i for i, nm in enumerate(names)}
    # what the case is built for, checked on the device's own records
    assert n[(0, 0)] == n[(0, 1)] == 0 and n[(len(seqs) - 1, 0)] == n[(len(seqs) - 1, H - 1)] == 0        # first and last pairs: no domain
    assert n[(q["none1"], 0)] == 0 and n[(q["whole"], 0)] == 1 and n[(q["short"], 0)] == 1                  # an empty pair between two others
    assert dom_off[0] == 0 and dom_off[1] == 0 and dom_off[-1] == dom_off[-2] == len(recs)
    whole = got[(q["whole"], 0)][0]
    assert (whole["env_i"], whole["env_j"]) == (1, len(seqs[q["whole"]])) and whole["env_j"] > 64
    assert got[(q["short"], 0)][0]["env_j"] < 64
    t = got[(q["tandem"], 0)]
    assert len(t) == 2 and t[1]["env_i"] <= t[0]["env_j"], "two overlapping envelopes of one pair"
    assert flags[q["tandem"], 0] & FLAG_MULTI and flags[q["tandem"], 0] & FLAG_REPORTED, "a pair finished by the resolver"
    assert len(got[(q["chimera"], 0)]) == 2 and not unl.any()
    lnp = np.array([d["lnP"] for k, v in got.items() for d in v if k[1] == 1])
    assert len(lnp) > 0 and np.isnan(lnp).all(), "a model without a STATS LOCAL FORWARD line"
    assert not np.isnan([d["lnP"] for k, v in got.items() for d in v if k[1] == 0]).any()


def test_long_list_pair_lists_16_domains_and_counts_the_rest(tmp_path):
    """A pair with more regions than a detail record lists: 16 records, "of" the full count, n_unlisted the rest.  (The
    scoring kernels export the REGION count of such a pair, not its envelope count: the case has one envelope per region.)"""
    _need_gpu()
    from witch_amd._lib import WH_MAX_ENVELOPES
    paths, names, seqs = dr.long_list_case(str(tmp_path))
    want, info = dr.reference_for(paths, seqs, max_list=WH_MAX_ENVELOPES)
    recs, dom_off, unl, flags, det, H = _run(paths, seqs)
    got = _by_pair(recs, dom_off, len(seqs), H)
    for h in range(H):
        _, nreg, nenv = info[(0, h)]
        assert nreg == nenv > WH_MAX_ENVELOPES, "the case no longer has one envelope per region"
        assert len(got[(0, h)]) == WH_MAX_ENVELOPES and unl[0, h] == nenv - WH_MAX_ENVELOPES
        assert all(d["of"] == nenv for d in got[(0, h)])
        assert unl[1, h] == 0 and len(got[(1, h)]) == 1
    _check_against_reference("long list", got, want, paths)


def test_force_wide_gives_the_same_records(shapes, monkeypatch):
    """The default run's flags and detail records through a handle loaded under WH_FORCE_WIDE=4, where the envelopes'
    alignment goes through the several-waves kernels: the records are the default run's, bit for bit, except oasc, which
    stays within the bound of the reference (so the two runs are within twice the bound of each other)."""
    _need_gpu()
    from witch_amd.ehmm import EHMM, pack_queries
    paths, names, seqs, want, info = shapes
    res, offs = pack_queries(seqs)
    e = EHMM(paths)
    deci, flags, det = e.score(res, offs, want_detail=True)
    a, off_a = e.domains(res, offs, flags, det)
    e.close()
    monkeypatch.setenv("WH_FORCE_WIDE", "4")
    w = EHMM(paths)
    monkeypatch.delenv("WH_FORCE_WIDE")
    b, off_b = w.domains(res, offs, flags, det)
    w.close()
    assert np.array_equal(off_a, off_b) and len(a) == len(b) > 0
    for k in a.dtype.names:
        if k != "oasc":
            assert a[k].tobytes() == b[k].tobytes(), k
    Ld = (a["env_j"] - a["env_i"] + 1).astype(np.float64)
    assert np.all(np.abs(a["oasc"].astype(np.float64) - b["oasc"]) / Ld <= 2 * (2e-4 + 3e-6 * Ld))
    _check_against_reference("force wide", _by_pair(b, off_b, len(seqs), len(paths)), want, paths)


def test_device_entry_point_on_a_stream_and_repeatability():
    """wh_domains_dev on torch tensors and a side stream gives the bytes of wh_domains; a second call on the same handle the
    same bytes again; wh_ehmm_evparams and the timer slot of the stage."""
    _need_gpu()
    import ctypes as C
    import torch
    from witch_amd.ehmm import EHMM, pack_queries
    from witch_amd.shim.formats import hmm_header
    case = load_case("dna_hmmbuild")
    paths = case.hmm_paths[:3]
    e = EHMM(paths)
    tau, lam, present = e.evparams()
    hdrs = [hmm_header(p) for p in paths]
    assert present.all() and np.array_equal(tau, np.float32([h["ftau"] for h in hdrs])) and np.array_equal(lam, np.float32([h["flambda"] for h in hdrs]))
    seqs = [e.digitize(s) for s in case.qseqs[:20]]
    res, offs = pack_queries(seqs)
    deci, flags, det = e.score(res, offs, want_detail=True)
    e.set_timing(True)
    host, dom_off = e.domains(res, offs, flags, det)
    ms, launches = e.last_kernel_ms(5)
    assert len(host) > 0 and launches >= 4 and ms > 0.0
    again, _ = e.domains(res, offs, flags, det)
    assert host.tobytes() == again.tobytes()
    dev = torch.device("cuda")
    det_t = torch.from_numpy(np.frombuffer(bytes(det), dtype=np.uint8).copy()).to(dev)
    res_t, offs_t, flags_t = torch.from_numpy(res).to(dev), torch.from_numpy(offs).to(dev), torch.from_numpy(flags).to(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out_t, off_t, unl_t = e.domains_dev(res_t, offs_t, int(np.diff(offs).max()), flags_t, det_t)
    side.synchronize()
    e.close()
    assert np.array_equal(off_t.cpu().numpy(), dom_off) and not unl_t.any().item()
    assert out_t.cpu().numpy().tobytes() == host.tobytes()


def test_shim_writes_domtblout_like_hmmer(tmp_path):
    """hmmsearch --max -E 99999999 --domtblout F through the server on dna_hmmbuild/A_0_0: the lines of the strong stratum
    are HMMER's raw lines byte for byte, but for those whose only difference is a print boundary (counted)."""
    _need_gpu()
    import threading
    from witch_amd.shim.server import GpuBackend, Server, request
    case = load_case("dna_hmmbuild")
    m = dr.load_fixture("dna_hmmbuild")["models"][0]
    sock = str(tmp_path / "g.sock")
    if len(sock) > 100:
        import tempfile
        sock = os.path.join(tempfile.mkdtemp(prefix="wh_dom_", dir="/tmp"), "g.sock")
    srv = Server(GpuBackend(0), sock)
    ready = threading.Event()
    threading.Thread(target=srv.serve_forever, args=(ready,), daemon=True).start()
    assert ready.wait(10)
    fa = os.path.join(case.dir, "queries.fasta")
    st, msg = request(sock, "hmmsearch", ["--cpu", "1", "--noali", "-E", "99999999", "--max", "-o", "o.txt", "--domtblout", "d.tbl",
                                          case.hmm_paths[0], fa], cwd=str(tmp_path))
    assert st == 0, msg
    lines = open(tmp_path / "d.tbl").read().splitlines()
    assert lines[:3] == m["header"]
    body = [ln for ln in lines if not ln.startswith("#")]
    n, same, boundary, weak, weak_same = dr.check_strong_lines(body, m["lines"])
    assert n > 0 and same + boundary == n and boundary <= max(1, n // 20)
    text = open(tmp_path / "o.txt").read()
    assert text.count("\n>> ") == m["domZ"] and "Domain annotation for each sequence:" in text
    # without the option the backend computes no domains and the output has no domain section
    st, plain = request(sock, "hmmsearch", ["--cpu", "1", "--noali", "-E", "99999999", "--max", case.hmm_paths[0], fa], cwd=str(tmp_path))
    assert st == 0 and ">>" not in plain
