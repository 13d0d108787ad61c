"""hmmalign for a file of several sequences on the GPU (wh_msa_dev, wh_msa, the level-0 hmmalign): the assembly kernels
alone against the bundled binary's matrices, the whole call against the numpy assembly (tests/msa_reference.py) and
against the binary, the edges, and the server.  Fixtures: tests/golden/msa.

Against the binary a row is compared where that sequence's columns are hmmalign's; PP and PP_cons characters are compared
outside the guard band of tests/test_align_pp.py (a float64 reference value within the float32 path's tolerance tol32(L) of
a character boundary; for PP_cons the same bound on a mean: the largest tolerance among the sequences that contribute), one
step apart at most inside it, and at most 1 % of a case's characters may lie inside it (0.0 - 0.4 % on these cases,
counted on the CPU from the reference alone)."""
import os
import threading

import numpy as np
import pytest

from tests import msa_reference as mr
from tests import pp_reference as ppr
from tests.test_align_pp import BOUNDS, _need_gpu, _steps, tol32

pytestmark = pytest.mark.gpu
MAX_BAND = 0.01            # (tests/filters_common.py: MAX_SKIP)


class Case:
    """A fixture with its model on the device, made once per module."""

    def __init__(self, name):
        from witch_amd.ehmm import EHMM
        self.name = name
        self.fx = mr.load_fixture(name)
        self.M, self.names, self.texts, self.cols, self.digits, self.parsed = mr.fixture_inputs(name)
        self.e = EHMM([self.fx["hmm_path"]])
        assert int(self.e.M[0]) == self.M
        self.res, self.offs = self.e.digitize_many([t.upper() for t in self.texts])
        self.text = "".join(self.texts)


_cases = {}


def _case(name):
    _need_gpu()
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


def _tensors(cols, pps, texts):
    import torch
    dev = torch.device("cuda:0")
    offs = np.zeros(len(cols) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(c) for c in cols])
    cat = lambda xs, dt: np.concatenate([np.asarray(x, dtype=dt) for x in xs]) if len(xs) and offs[-1] else np.zeros(0, dtype=dt)   # noqa: E731
    text = np.frombuffer("".join(texts).encode(), dtype=np.uint8)
    return (torch.from_numpy(cat(cols, np.int32)).to(dev), torch.from_numpy(cat(pps, np.float32)).to(dev),
            torch.from_numpy(text.copy()).to(dev), torch.from_numpy(offs).to(dev))


def _same(got, want, what):
    for k in ("rows", "pp_rows", "pp_cons", "rf", "matmap"):
        assert np.array_equal(got[k], want[k]), (what, k)
    assert got["W"] == want["W"] and got["pathless"] == want["pathless"], what


# ------------------------------------------------------------------------------------------------ 1. the kernels alone
@pytest.mark.parametrize("name", mr.CASES)
def test_kernels_alone_reproduce_the_binary(name):
    """wh_msa_dev on the columns decoded from the binary's rows, posteriors at the middle of each PP character's interval:
    rows, PP rows, RF, matmap and W are the binary's, with and without --trim, from LDS and from global memory; PP_cons is
    the numpy assembly's (the same float32 sums in the same order)."""
    c = _case(name)
    pps = [mr.midpoints(d) for d in c.digits]
    t = _tensors(c.cols, pps, c.texts)
    for key, trim in (("sto", False), ("trim", True)):
        rows, gr, cons, rf = mr.parse_msa(c.fx["out"][key])
        want = mr.assemble(c.M, c.cols, pps, c.texts, trim=trim)
        for no_lds in (False, True):
            got = c.e.msa_t(*t, h=0, trim=trim, no_lds=no_lds)
            what = (name, key, "global" if no_lds else "lds")
            assert got["W"] == len(rf) and got["rf"].tobytes().decode() == rf, what
            assert np.array_equal(got["rows"], mr.matrix(rows, c.names)), what
            assert np.array_equal(got["pp_rows"], mr.matrix(gr, c.names)), what
            assert np.array_equal(got["matmap"], np.array([i for i, ch in enumerate(rf) if ch == "x"])), what
            _same(got, want, what)


# ------------------------------------------------------------------------------------------------ 2. end to end
@pytest.fixture(scope="module")
def shares():
    out = {}
    yield out
    if out:
        print("share of sequences whose columns differ from hmmalign's: " + ", ".join("%s %.4f" % kv for kv in sorted(out.items())))


@pytest.mark.parametrize("name", mr.CASES)
def test_end_to_end(name, shares):
    from oracle import oracle as orc
    c = _case(name)
    nq = len(c.names)
    got = c.e.msa(c.res, c.offs, c.text)
    cols, co, pp = c.e.align(c.res, c.offs, np.arange(nq), np.zeros(nq, dtype=np.int32), want_pp=True)
    mine = [cols[co[q]:co[q + 1]] for q in range(nq)]
    _same(got, mr.assemble(c.M, mine, [pp[co[q]:co[q + 1]] for q in range(nq)], c.texts), (name, "numpy assembly"))
    _same(c.e.msa(c.res, c.offs, c.text, trim=True),
          mr.assemble(c.M, mine, [pp[co[q]:co[q + 1]] for q in range(nq)], c.texts, trim=True), (name, "numpy assembly, trim"))
    # against the binary
    rows, gr, cons, rf = c.parsed
    same = [np.array_equal(mine[q], c.cols[q]) for q in range(nq)]
    shares[name] = 1.0 - sum(same) / nq
    print("%s: %d of %d sequences have columns that differ from hmmalign's" % (name, nq - sum(same), nq))
    ohm = orc.OracleHMM(c.fx["hmm_path"])
    model = ppr.Model(ohm)
    n_chars = n_band = 0
    ref_sum, ref_n, ref_tol = np.zeros(c.M), np.zeros(c.M, dtype=np.int64), np.zeros(c.M)
    dirty = np.zeros(c.M, dtype=bool)                 # nodes a sequence with other columns touches: no PP_cons comparison
    if all(same):
        assert got["W"] == len(rf) and got["rf"].tobytes().decode() == rf
    for q, n in enumerate(c.names):
        if not same[q]:
            for cc in (mine[q], c.cols[q]):
                dirty[cc[cc >= 0]] = True
            continue
        mine_row = got["rows"][q].tobytes().decode()
        assert mine_row == rows[n] if all(same) else mine_row.replace(".", "") == rows[n].replace(".", ""), (name, n)
        ref = ppr.path_posteriors(model, ohm.digitize(c.texts[q].upper()), c.cols[q])
        tol = tol32(len(ref))
        band = np.min(np.abs(ref[:, None] - BOUNDS[None, :]), axis=1) <= tol
        ours = [chr(ch) for ch in got["pp_rows"][q] if ch != ord(".")]
        assert len(ours) == len(c.digits[q])
        n_chars += len(ref)
        n_band += int(band.sum())
        for i, (x, y) in enumerate(zip(ours, c.digits[q])):
            assert x == y or (band[i] and _steps(x, y) == 1), (name, n, i, x, y, ref[i])
        m = c.cols[q] >= 0
        np.add.at(ref_sum, c.cols[q][m], ref[m])
        np.add.at(ref_n, c.cols[q][m], 1)
        np.maximum.at(ref_tol, c.cols[q][m], tol)
    bin_matmap = [i for i, ch in enumerate(rf) if ch == "x"]
    for k in range(c.M):
        x, y = chr(got["pp_cons"][got["matmap"][k]]), cons[bin_matmap[k]]
        if dirty[k]:
            continue
        if ref_n[k] == 0:
            assert x == y == ".", (name, k)
            continue
        mean = ref_sum[k] / ref_n[k]
        inb = np.min(np.abs(mean - BOUNDS)) <= ref_tol[k]
        n_chars += 1
        n_band += int(inb)
        assert x == y or (inb and _steps(x, y) == 1), (name, "PP_cons", k, x, y, mean)
    print("%s: %d characters compared with hmmalign's, %d in the guard band" % (name, n_chars, n_band))
    assert n_chars > 0 and n_band <= MAX_BAND * n_chars, (name, n_band, n_chars)


# ------------------------------------------------------------------------------------------------ 3. edges
def test_one_sequence_is_todays_stockholm():
    from witch_amd.shim import formats
    c = _case("dna_synth")
    for q in (0, 1, 7):
        res, offs = c.e.digitize_many([c.texts[q].upper()])
        got = c.e.msa(res, offs, c.texts[q])
        cols, co, pp = c.e.align(res, offs, np.zeros(1, np.int64), np.zeros(1, np.int32), want_pp=True)
        row = formats.stockholm_row(c.texts[q], cols, c.M, flank_at_end=True)
        gr, cons, rfl = formats.stockholm_pp_lines(row, pp)
        assert got["rows"][0].tobytes().decode() == row and got["pp_rows"][0].tobytes().decode() == gr
        assert got["pp_cons"].tobytes().decode() == cons and got["rf"].tobytes().decode() == rfl
        name = c.names[q]
        assert len(name) >= 4 and formats.format_msa([name], got["rows"], got["pp_rows"], got["pp_cons"], got["rf"]) == \
            formats.format_stockholm(name, row, pp=pp)


def test_no_sequences():
    c = _case("dna_synth")
    got = c.e.msa(np.zeros(0, np.uint8), np.zeros(1, np.int64), "")
    assert got["W"] == c.M and got["rows"].shape == (0, c.M) and got["pp_rows"].shape == (0, c.M) and got["pathless"] == 0
    assert got["rf"].tobytes() == b"x" * c.M and got["pp_cons"].tobytes() == b"." * c.M
    assert np.array_equal(got["matmap"], np.arange(c.M))
    got = c.e.msa_t(*_tensors([], [], []))
    assert got["W"] == c.M and got["rows"].shape == (0, c.M)


@pytest.mark.parametrize("no_lds", [False, True])
def test_synthetic_layouts(no_lds):
    """Columns written by hand, on the 156-node model: no insert anywhere (W = M); a W that is a multiple of 16 and one that is
    not, with rows that start at every alignment inside a 16-byte line; a sequence without a path, rendered as gaps and
    counted; a run longer than the workgroup is wide."""
    c = _case("dna_synth")
    M = c.M
    rng = np.random.default_rng(5)
    seq = lambda n: "".join("ACGT"[i] for i in rng.integers(0, 4, size=n))      # noqa: E731
    pps = lambda n: rng.random(n).astype(np.float32)                             # noqa: E731

    def run(cols, trim=False):
        texts = [seq(len(x)) for x in cols]
        pp = [pps(len(x)) for x in cols]
        got = c.e.msa_t(*_tensors(cols, pp, texts), trim=trim, no_lds=no_lds)
        _same(got, mr.assemble(M, cols, pp, texts, trim=trim), "synthetic")
        return got
    full = np.arange(M, dtype=np.int32)
    got = run([full, full[10:90], np.concatenate([full[:40], full[60:]])])
    assert got["W"] == M and got["rf"].tobytes() == b"x" * M
    for flank in (4, 5):                                # W = 160, 161
        cols = [np.concatenate([np.full(flank, -1, np.int32), full]), full[3:], full[:100], full[50:], full, full[7:20]]
        got = run(cols * 3)
        assert got["W"] == M + flank and (got["W"] % 16 == 0) == (flank == 4)
    lost = np.full(33, -1, dtype=np.int32)
    got = run([full, lost, np.concatenate([full[:70], np.full(300, -1, np.int32), full[70:]]), np.zeros(0, np.int32)])
    assert got["pathless"] == 1 and got["W"] == M + 300
    assert set(got["rows"][1].tobytes()) <= set(b"-.") and set(got["pp_rows"][1].tobytes()) == set(b".")
    assert set(got["rows"][3].tobytes()) <= set(b"-.")
    got = run([np.concatenate([np.full(5, -1, np.int32), full[20:60], np.full(9, -1, np.int32)]), full], trim=True)
    assert got["W"] == M


def test_a_model_beyond_3072_nodes(tmp_path):
    """The recipe of the long_model fixture of tests/golden/align_pp with 3 300 nodes: the alignment comes from the
    several-waves or the float64 kernel, the assembly does not care which."""
    _need_gpu()
    import copy
    from witch_amd import synth
    from witch_amd.ehmm import EHMM
    spec = copy.deepcopy(ppr.load_fixture("long_model")["spec"])
    spec["family"]["root_len"] = 3300
    spec["family"]["seed"] = 4242 + 3300
    spec["multicopy"]["keep"] = []
    fam, hp = ppr.long_model(spec, str(tmp_path))
    names, seqs, kinds = ppr.long_queries(spec, fam)
    e = EHMM([hp])
    M = int(e.M[0])
    assert M > 3072 and len(seqs) == 2
    texts = [synth.to_text(s.astype(np.int64), "dna") for s in seqs]
    res, offs = e.digitize_many(texts)
    got = e.msa(res, offs, "".join(texts))
    cols, co, pp = e.align(res, offs, np.arange(2), np.zeros(2, dtype=np.int32), want_pp=True)
    e.close()
    assert (cols >= 0).sum() > 100
    _same(got, mr.assemble(M, [cols[co[q]:co[q + 1]] for q in range(2)], [pp[co[q]:co[q + 1]] for q in range(2)], texts), "long model")


# ------------------------------------------------------------------------------------------------ 4. level 0
def test_level0_hmmalign_writes_the_binary_file(tmp_path):
    """hmmalign -o OUT HMM FASTA through a resident Server(GpuBackend) on dna_planted, whose columns are all hmmalign's: OUT is
    the binary's file byte for byte, but for PP / PP_cons characters inside the guard band; then with --trim."""
    _need_gpu()
    import shutil
    import tempfile
    from oracle import oracle as orc
    from witch_amd.shim import formats
    from witch_amd.shim.server import GpuBackend, Server, request
    name = "dna_planted"
    fx = mr.load_fixture(name)
    M, names, texts, cols, digits, _ = mr.fixture_inputs(name)
    ohm = orc.OracleHMM(fx["hmm_path"])
    model = ppr.Model(ohm)
    refs = [ppr.path_posteriors(model, ohm.digitize(t.upper()), cc) for t, cc in zip(texts, cols)]
    fa = tmp_path / "in.fa"
    fa.write_text("".join(">%s\n%s\n" % (n, s) for n, s in zip(names, texts)))
    d = tempfile.mkdtemp(prefix="wh_sock_", dir="/tmp")
    try:
        sock = os.path.join(d, "s.sock")
        srv = Server(GpuBackend(0), sock)
        ready = threading.Event()
        threading.Thread(target=srv.serve_forever, args=(ready,), daemon=True).start()
        assert ready.wait(10)
        for key, extra in (("sto", []), ("trim", ["--trim"])):
            status, body = request(sock, "hmmalign", extra + ["-o", "out_%s.sto" % key, fx["hmm_path"], str(fa)], cwd=str(tmp_path))
            assert status == 0 and body == "", body
            out = (tmp_path / ("out_%s.sto" % key)).read_text()
            rows, gr, cons, rf = mr.parse_msa(fx["out"][key])
            g_rows, g_gr, g_cons, g_rf = mr.parse_msa(out)
            assert g_rows == rows and g_rf == rf, key
            # the binary's matrices with this build's characters where the guard band allows another one: the file must be that
            patched, n_band, n_chars = {}, 0, 0
            for n, cc, dg, ref in zip(names, cols, digits, refs):
                keep = np.ones(len(cc), dtype=bool)
                if key == "trim":
                    hit = np.nonzero(cc >= 0)[0]
                    keep[:hit[0]] = False
                    keep[hit[-1] + 1:] = False
                band = (np.min(np.abs(ref[:, None] - BOUNDS[None, :]), axis=1) <= tol32(len(ref)))[keep]
                line, i = list(gr[n]), 0
                for at, ch in enumerate(gr[n]):
                    if ch != ".":
                        if band[i] and _steps(g_gr[n][at], ch) == 1:
                            line[at] = g_gr[n][at]
                        i += 1
                assert i == int(keep.sum())
                patched[n] = "".join(line)
                n_band += int(band.sum())
                n_chars += len(band)
            cons_p = list(cons)
            matcol = [i for i, ch in enumerate(rf) if ch == "x"]
            for k in range(M):
                vals = [(ref[np.nonzero(cc == k)[0][0]], tol32(len(ref))) for cc, ref in zip(cols, refs) if (cc == k).any()]
                if vals:
                    mean, tol = np.mean([v for v, _ in vals]), max(t for _, t in vals)
                    inb = np.min(np.abs(mean - BOUNDS)) <= tol
                    n_chars += 1
                    n_band += int(inb)
                    if inb and _steps(g_cons[matcol[k]], cons[matcol[k]]) == 1:
                        cons_p[matcol[k]] = g_cons[matcol[k]]
            assert n_band <= MAX_BAND * n_chars, (key, n_band, n_chars)
            want = formats.format_msa(names, [rows[n] for n in names], [patched[n] for n in names], "".join(cons_p), rf)
            assert out == want, key
            print("level 0, %s: %d bytes, %d of %d PP characters in the guard band, file %s the binary's" %
                  (key, len(out), n_band, n_chars, "is" if out == fx["out"][key] else "differs inside the band from"))
        status, body = request(sock, "hmmalign", ["--outformat", "afa", fx["hmm_path"], str(fa)], cwd=str(tmp_path))
        assert status == 0 and body == fx["out"]["afa"]
    finally:
        shutil.rmtree(d, ignore_errors=True)
