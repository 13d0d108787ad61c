"""hmmalign --mapali on the GPU (wh_msa_mapali_dev, wh_msa_mapali, the level-0 hmmalign --mapali): the mapping and assembly
kernels alone against the bundled binary's matrices, the whole call against the numpy restatement (tests/mapali_reference.py)
and against the binary, synthetic shapes at the sizes where the compaction can go wrong, and the server.  Fixtures:
tests/golden/mapali.

The rows of the alignment carry no posteriors and must equal the binary's byte for byte.  The new sequences' PP and PP_cons
characters fall under the guard-band rule of tests/test_msa_gpu.py, with its cap of 1 % of a case's characters."""
import os
import threading

import numpy as np
import pytest

from tests import mapali_reference as mp
from tests import msa_reference as mr
from tests import pp_reference as ppr
from tests.test_align_pp import BOUNDS, _need_gpu, _steps, tol32
from tests.test_msa_gpu import MAX_BAND, _same, _tensors

pytestmark = pytest.mark.gpu


class Part:
    """A fixture part with its model on the device, made once per module."""

    def __init__(self, name, i, tmpdir):
        from witch_amd.ehmm import EHMM
        self.p, self.d = mp.load_fixture(name)[i], mp.part_inputs(name, i)
        self.hmm = mp.hmm_file(self.p, tmpdir)
        self.e = EHMM([self.hmm])
        assert int(self.e.M[0]) == self.d["M"] and self.e.cksum(0) == self.d["cksum"]
        self.texts = self.p["seqs"]
        self.res, self.offs = self.e.digitize_many([t.upper() for t in self.texts])
        self.mapali = (self.d["names"], self.d["rows"])
        self.n_map = len(self.d["names"])


_parts = {}


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    return tmp_path_factory.mktemp("mapali_models")


def _part(name, i, models):
    _need_gpu()
    if (name, i) not in _parts:
        _parts[(name, i)] = Part(name, i, models)
    return _parts[(name, i)]


def _rows_t(rows):
    import torch
    return torch.from_numpy(np.frombuffer("".join(rows).encode(), dtype=np.uint8).reshape(len(rows), -1).copy()).to("cuda:0")


def _restate(c, cols, pps, trim=False):
    return mp.assemble(c.d["M"], c.d["map_cols"] + list(cols), [None] * c.n_map + list(pps), c.d["map_texts"] + c.texts, n_nopp=c.n_map, trim=trim)


def _pp_within_the_band(what, hmm, d, p, ours, ours_cons):
    """The new sequences' PP characters (ours: {name: the characters of its residues}) and the PP_cons line against the
    binary's: equal, or one step apart where the CPU oracle's float64 posterior (for PP_cons: the mean) lies within the
    float32 path's tolerance of a character boundary; at most MAX_BAND of the characters may lie there."""
    from oracle import oracle as orc
    rows, gr, cons, rf = d["parsed"]
    ohm = orc.OracleHMM(hmm)
    model = ppr.Model(ohm)
    M = d["M"]
    n_chars = n_band = 0
    ref_sum, ref_n, ref_tol = np.zeros(M), np.zeros(M, dtype=np.int64), np.zeros(M)
    for q, n in enumerate(p["names"]):
        ref = ppr.path_posteriors(model, ohm.digitize(p["seqs"][q].upper()), d["cols"][q])
        tol = tol32(len(ref))
        band = np.min(np.abs(ref[:, None] - BOUNDS[None, :]), axis=1) <= tol
        assert len(ours[n]) == len(d["digits"][q]), (what, n)
        n_chars += len(ref)
        n_band += int(band.sum())
        for j, (x, y) in enumerate(zip(ours[n], d["digits"][q])):
            assert x == y or (band[j] and _steps(x, y) == 1), (what, n, j, x, y, ref[j])
        m = d["cols"][q] >= 0
        np.add.at(ref_sum, d["cols"][q][m], ref[m])
        np.add.at(ref_n, d["cols"][q][m], 1)
        np.maximum.at(ref_tol, d["cols"][q][m], tol)
    assert len(ours_cons) == len(rf)
    matcol = [j for j, ch in enumerate(rf) if ch == "x"]
    assert all(ours_cons[j] == "." == cons[j] for j, ch in enumerate(rf) if ch != "x"), what
    for k in range(M):
        x, y = ours_cons[matcol[k]], cons[matcol[k]]
        if ref_n[k] == 0:
            assert x == y == ".", (what, k)
            continue
        mean = ref_sum[k] / ref_n[k]
        inb = np.min(np.abs(mean - BOUNDS)) <= ref_tol[k]
        n_chars += 1
        n_band += int(inb)
        assert x == y or (inb and _steps(x, y) == 1), (what, "PP_cons", k, x, y, mean)
    print("%s: %d characters compared with hmmalign's, %d in the guard band" % (what, n_chars, n_band))
    assert n_chars > 0 and n_band <= MAX_BAND * n_chars, (what, n_band, n_chars)


# ------------------------------------------------------------------------------------------------ 1. the kernels alone
@pytest.mark.parametrize("name,i", mp.all_parts())
def test_kernels_alone_reproduce_the_binary(name, i, models):
    """wh_msa_mapali_dev on the alignment's rows and on the new sequences' columns as decoded from the binary's output,
    posteriors at the middle of each PP character's interval: all rows, the PP rows, RF, matmap and W are the binary's, with
    and without --trim, from LDS and from global memory; PP_cons is the restatement's."""
    c = _part(name, i, models)
    pps = [mr.midpoints(x) for x in c.d["digits"]]
    t = _tensors(c.d["cols"], pps, c.texts)
    rows_t = _rows_t(c.d["rows"])
    names = c.d["names"] + c.p["names"]
    for key, trim in (("sto", False), ("trim", True)):
        rows, gr, cons, rf = mr.parse_msa(c.p["out"][key])
        want = _restate(c, c.d["cols"], pps, trim)
        for no_lds in (False, True):
            got = c.e.msa_t(*t, h=0, trim=trim, no_lds=no_lds, mapali_t=rows_t)
            what = (name, i, key, "global" if no_lds else "lds")
            assert got["W"] == len(rf) and got["rf"].tobytes().decode() == rf, what
            assert np.array_equal(got["rows"], mr.matrix(rows, names)), what
            assert np.array_equal(got["pp_rows"], mr.matrix(gr, c.p["names"])), what
            assert np.array_equal(got["matmap"], np.array([j for j, ch in enumerate(rf) if ch == "x"])), what
            _same(got, want, what)


# ------------------------------------------------------------------------------------------------ 2. end to end
@pytest.mark.parametrize("name,i", mp.all_parts())
def test_end_to_end(name, i, models):
    """wh_msa_mapali: equal to the restatement on this build's own alignment of the new sequences; against the binary the
    alignment's rows, RF and W byte for byte (every new sequence of these fixtures gets hmmalign's columns), the PP characters
    within the guard band."""
    c = _part(name, i, models)
    nq = len(c.texts)
    text = "".join(c.texts)
    got = c.e.msa(c.res, c.offs, text, mapali=c.mapali)
    cols, co, pp = c.e.align(c.res, c.offs, np.arange(nq), np.zeros(nq, dtype=np.int32), want_pp=True)
    mine = [cols[co[q]:co[q + 1]] for q in range(nq)]
    mypp = [pp[co[q]:co[q + 1]] for q in range(nq)]
    _same(got, _restate(c, mine, mypp), (name, i, "restatement"))
    _same(c.e.msa(c.res, c.offs, text, trim=True, no_lds=True, mapali=c.mapali), _restate(c, mine, mypp, trim=True), (name, i, "restatement, trim"))
    rows, gr, cons, rf = c.d["parsed"]
    assert all(np.array_equal(mine[q], c.d["cols"][q]) for q in range(nq)), (name, i, "columns differ from hmmalign's")
    assert got["W"] == len(rf) and got["rf"].tobytes().decode() == rf and got["pathless"] == 0
    names = c.d["names"] + c.p["names"]
    assert np.array_equal(got["rows"], mr.matrix(rows, names)), (name, i)
    ours = {n: "".join(chr(ch) for ch in got["pp_rows"][q] if ch != ord(".")) for q, n in enumerate(c.p["names"])}
    _pp_within_the_band((name, i), c.hmm, c.d, c.p, ours, got["pp_cons"].tobytes().decode())


def test_refusals_and_getters(models, tmp_path):
    from witch_amd.ehmm import EHMM
    c = _part("one_new", 0, models)
    bad = mp.part_inputs("mismatch", 0)
    with pytest.raises(RuntimeError) as ei:
        c.e.msa(c.res, c.offs, "".join(c.texts), mapali=(bad["names"], bad["rows"]))
    assert "wh_msa_mapali" in str(ei.value) and "checksum mismatch" in str(ei.value)
    with pytest.raises(RuntimeError) as ei:                  # alen short of the last MAP column
        c.e.msa(c.res, c.offs, "".join(c.texts), mapali=(c.d["names"], [r[:20] for r in c.d["rows"]]))
    assert "wh_msa_mapali" in str(ei.value) and "MAP column" in str(ei.value)
    with pytest.raises(RuntimeError) as ei:
        c.e.msa(c.res, c.offs, "".join(c.texts), mapali=(c.d["names"], [r.replace("g", "!") for r in c.d["rows"]]))
    assert "wh_msa_mapali" in str(ei.value)
    # a model without MAP / CKSUM lines
    text = mp.hmm_text(c.p)
    for drop, word in (("CKSUM", "CKSUM"), ("MAP   yes", "MAP")):
        path = tmp_path / ("no_%s.hmm" % word)
        path.write_text("".join(ln + "\n" for ln in text.splitlines() if not ln.startswith(drop)))
        e = EHMM([str(path)])
        if word == "CKSUM":
            assert e.cksum(0) is None
        with pytest.raises(RuntimeError) as ei:
            e.msa(c.res, c.offs, "".join(c.texts), mapali=c.mapali)
        assert "wh_msa_mapali" in str(ei.value) and word in str(ei.value)
        e.close()
    # no rows: wh_msa's result
    a, b = c.e.msa(c.res, c.offs, "".join(c.texts), mapali=([], [])), c.e.msa(c.res, c.offs, "".join(c.texts))
    _same(a, b, "n_map == 0")


# ------------------------------------------------------------------------------------------------ 3. synthetic shapes
SHAPES = [(n, alen) for n in (1, 65) for alen in (1, 63, 64, 65, 128, 129, 1025)]


@pytest.mark.parametrize("n_map,alen", SHAPES)
def test_synthetic_shapes(n_map, alen, tmp_path):
    """Alignments of tests/mapali_reference.synthetic_alignment (a row with no residue, one with no gap, one with residues in
    insert columns only; blocks 0 and M populated by the alignment only) and the model wh_hmmbuild makes of each: alen at the
    edges of the 64-column trips of the count and map kernels, one row and more rows than a wavefront has lanes; with three
    new sequences, with none (n_map > 0, nq == 0), with and without --trim and LDS."""
    _need_gpu()
    from witch_amd.ehmm import EHMM
    from witch_amd.gcmm.hmmbuild import hmmbuild_text
    names, rows = mp.synthetic_alignment(n_map, alen)
    text, M, _ = hmmbuild_text(rows, "dna", "syn", symfrac=0.5)
    path = tmp_path / "syn.hmm"
    path.write_text(text)
    _, _, cksum, mapc = mp.model_header(text)
    code = mp.colcode(mapc, alen)
    mcols, mtexts = mp.row_sequences(rows, code)
    if n_map >= 3:
        assert len(mcols[0]) == 0 and len(mcols[1]) == alen and (len(mcols[2]) == 0 or mcols[2].max() <= -2)
    if n_map >= 3 and alen >= 5:
        assert code[0] == -2 and code[-1] == -(M + 2)
    e = EHMM([str(path)])
    assert e.cksum(0) == cksum and np.array_equal(e.map_columns(0), mapc)
    full = mtexts[min(1, n_map - 1)]
    new = [full, "ac" + full[:alen // 2] + "gg" + full[alen // 2:], full[5:40]]
    for texts in ([], new) if M >= 16 else ([],):              # (alen 1: a model of one node, the rows alone)
        res, offs = e.digitize_many([t.upper() for t in texts])
        nq = len(texts)
        if nq:
            cols, co, pp = e.align(res, offs, np.arange(nq), np.zeros(nq, dtype=np.int32), want_pp=True)
            mine, mypp = [cols[co[q]:co[q + 1]] for q in range(nq)], [pp[co[q]:co[q + 1]] for q in range(nq)]
        else:
            mine, mypp = [], []
        for trim, no_lds in ((False, False), (True, True)):
            got = e.msa(res, offs, "".join(texts), trim=trim, no_lds=no_lds, mapali=(names, rows))
            want = mp.assemble(M, mcols + mine, [None] * n_map + mypp, mtexts + texts, n_nopp=n_map, trim=trim)
            _same(got, want, (n_map, alen, nq, trim))
            assert got["rows"].shape == (n_map + nq, got["W"]) and got["pp_rows"].shape == (nq, got["W"])
            if not trim and not nq:
                # a row without gaps reads back as itself, match residues upper case and inserts lower case
                k = min(1, n_map - 1)
                assert got["rows"][k].tobytes().decode().replace(".", "").upper() == rows[k]
    e.close()


def test_wh_msa_is_unchanged_by_explicit_codes(models):
    """The assembly kernels on the columns of a fixture of tests/golden/msa, through the --mapali entry point with no rows
    and through wh_msa_dev: the same bytes (tests/test_msa_gpu.py pins them to the binary)."""
    _need_gpu()
    from witch_amd.ehmm import EHMM
    M, names, texts, cols, digits, _ = mr.fixture_inputs("dna_planted")
    e = EHMM([mr.load_fixture("dna_planted")["hmm_path"]])
    pps = [mr.midpoints(d) for d in digits]
    t = _tensors(cols, pps, texts)
    import torch
    none = torch.zeros((0, 0), dtype=torch.uint8, device="cuda:0")
    for trim in (False, True):
        want = mr.assemble(M, cols, pps, texts, trim=trim)
        _same(e.msa_t(*t, trim=trim), want, "wh_msa_dev")
        _same(e.msa_t(*t, trim=trim, mapali_t=none), want, "wh_msa_mapali_dev, no rows")
    e.close()


# ------------------------------------------------------------------------------------------------ 4. level 0
@pytest.mark.parametrize("name", ["planted_sto", "one_new"])
def test_level0_hmmalign_mapali_writes_the_binary_file(name, tmp_path):
    """hmmalign --mapali ALN -o OUT HMM FASTA through a resident Server(GpuBackend): OUT is the binary's file byte for byte but
    for PP / PP_cons characters inside the guard band (none on these two cases unless the print below says so); the afa
    form; then an alignment with one residue altered: exit status 1 and HMMER's message."""
    _need_gpu()
    import shutil
    import tempfile
    from witch_amd.shim import formats
    from witch_amd.shim.server import GpuBackend, Server, request
    p, d = mp.load_fixture(name)[0], mp.part_inputs(name, 0)
    hmm = mp.hmm_file(p, tmp_path)
    aln = "aln.sto" if p["aln_format"] == "stockholm" else "aln.afa"
    (tmp_path / aln).write_text(p["aln"])
    (tmp_path / "bad.afa").write_text(mp.load_fixture("mismatch")[0]["aln"])
    fa = tmp_path / "new.fa"
    fa.write_text("".join(">%s\n%s\n" % z for z in zip(p["names"], p["seqs"])))
    sockdir = tempfile.mkdtemp(prefix="wh_sock_", dir="/tmp")
    try:
        sock = os.path.join(sockdir, "s.sock")
        srv = Server(GpuBackend(0), sock)
        ready = threading.Event()
        threading.Thread(target=srv.serve_forever, args=(ready,), daemon=True).start()
        assert ready.wait(10)
        for key, extra in (("sto", []), ("trim", ["--trim"]), ("pfam", ["--outformat", "Pfam"])):
            status, body = request(sock, "hmmalign", extra + ["--mapali", aln, "-o", "out_%s" % key, hmm, str(fa)], cwd=str(tmp_path))
            assert status == 0 and body == "", body
            out = (tmp_path / ("out_%s" % key)).read_text()
            want = p["out"][key]
            rows, gr, cons, rf = mr.parse_msa(want)
            g_rows, g_gr, g_cons, g_rf = mr.parse_msa(out)
            assert g_rows == rows and g_rf == rf and list(g_gr) == p["names"], key
            if key != "trim":
                _pp_within_the_band((name, key), hmm, d, p, {n: g_gr[n].replace(".", "") for n in p["names"]}, g_cons)
            # the file is the binary's with this build's PP characters
            names = d["names"] + p["names"]
            assert out == formats.format_msa(names, [rows[n] for n in names], [g_gr.get(n) for n in names], g_cons, rf,
                                             "Pfam" if key == "pfam" else "Stockholm", desc=d["desc"]), key
            print("level 0 --mapali, %s %s: %d bytes, file %s the binary's" % (name, key, len(out), "is" if out == want else "differs in PP characters from"))
        status, body = request(sock, "hmmalign", ["--mapali", aln, "--outformat", "afa", hmm, str(fa)], cwd=str(tmp_path))
        assert status == 0 and body == p["out"]["afa"]
        status, body = request(sock, "hmmalign", ["--mapali", "bad.afa", hmm, str(fa)], cwd=str(tmp_path))
        assert status == 1 and body.strip() == "--mapali MSA bad.afa isn't same as the one HMM came from (checksum mismatch)"
    finally:
        shutil.rmtree(sockdir, ignore_errors=True)
