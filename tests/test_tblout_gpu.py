"""hmmsearch --tblout on the GPU: the counting sweep (wh_seq_expect) against its float64 host replica at every class edge,
EHMM.seq_table and the shim's --tblout against the tables of the reference's bundled hmmsearch (tests/golden/tblout)."""
import math
import os

import numpy as np
import pytest

from tests import domains_reference as dr
from tests import tblout_common as tc
from tests.conftest import load_case

pytestmark = pytest.mark.gpu

TABLE_CASES = ("dna_hmmbuild", "amino_hmmbuild", "amino_multidomain")


def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ------------------------------------------------------------------------------------------------ 5. the sweep by shape
@pytest.mark.parametrize("alphabet", tc.CLASS_ALPHABETS)
def test_device_sweep_against_host_replica_at_every_class_edge(alphabet):
    """Models of 1, 2, 63, 64, 65 nodes, the last and first node count of every register class, 3 072 and 3 073 nodes (the
    hand-over to the any-size path); per model queries of 1, 3, 63, 64, 65, 128, 129 residues, a tandem and a chimera, a
    no-domain query first and last.  On every pair reg and clu equal the host replica's and exp agrees under the rule of
    tests/tblout_common.py."""
    _need_gpu()
    from witch_amd.ehmm import EHMM, seq_expect_host
    paths, res, offs, pairs, names = tc.class_call(alphabet)
    want = seq_expect_host(paths, res, offs, pairs)
    e = EHMM(paths)
    try:
        got = e.seq_expect(res, offs, pairs)
        again = e.seq_expect(res, offs, pairs[::-1].copy())
    finally:
        e.close()
    assert got.tobytes() == again[::-1].tobytes(), "the result of a pair depends on its place in the list"
    exempt = 0
    for nm, g, w in zip(names, got, want):
        assert (int(g["reg"]), int(g["clu"])) == (int(w["reg"]), int(w["clu"])), (alphabet, nm, g, w)
        ok, ex = tc.exp_ok(float(w["exp"]), "%.1f" % g["exp"])
        assert ok, (alphabet, nm, g, w)
        exempt += ex
    assert exempt <= tc.EXEMPT_CAP * len(names)
    # what the shapes are for, on the device's own results
    by = {nm: g for nm, g in zip(names, got)}
    assert sorted(set(M for M, _ in names)) == tc.CLASS_NODES and 3073 in tc.CLASS_NODES and 3072 in tc.CLASS_NODES
    assert names[0][1] == "call_first" and names[-1][1] == "call_last" and got[0]["reg"] == 0 and got[-1]["reg"] == 0
    big = [M for M in tc.CLASS_NODES if M >= 256]
    assert all(by[(M, "len1")]["reg"] == 0 for M in big), "pairs without a region between pairs with regions"
    assert all(by[(M, "tandem")]["clu"] >= 1 for M in big), "a tandem is a multidomain region"
    assert all(by[(M, "chimera")]["reg"] >= 1 for M in big) and any(by[(M, "chimera")]["reg"] == 2 for M in big)
    assert all(by[(M, "len%d" % n)]["reg"] >= 1 for M in big for n in (63, 64, 65, 128, 129))
    print("[%s] %d pairs on %d models: reg and clu equal, %d exp fields at a print boundary" % (alphabet, len(names), len(paths), exempt))


# ------------------------------------------------------------------------------------------------ 6. / 7. the table
def _line_ok(got, want):
    """A formatted row against HMMER's raw line under the rule of tests/domains_reference.check_strong_lines, whose strata are
    here the rows WITHOUT a clustered region (clu == 0: the strong stratum) and those with one (clu > 0: HMMER scores such a
    sequence from 200 seeded stochastic tracebacks per clustered region, the class that file counts apart).  Strong stratum:
    the line is HMMER's byte for byte, or differs only in printed float fields by one printed unit ("%.1f": 0.1; "%9.2g":
    the last printed digit) - an E-value HMMER prints as 0 must print as 0.  Weak stratum: the same columns may differ,
    score and bias by at most two printed units (the multidomain class of tests/domains_reference.compare_with_fixture).
    exp has its own rule; the integer columns are compared before.  Returns (differs, weak)."""
    gw, ww = got.split(), want.split()
    weak = int(ww[12]) > 0
    if got == want:
        return False, weak
    printed = {4: 2, 5: 1, 6: 1, 7: 2, 8: 1, 9: 1, 10: 1}          # column -> 1: "%.1f", 2: "%9.2g"
    diff = [c for c in range(len(ww)) if gw[c] != ww[c]]
    assert len(gw) == len(ww) and all(c in printed for c in diff), (got, want)
    for c in diff:
        g, w = float(gw[c]), float(ww[c])
        if printed[c] == 1:
            assert abs(g - w) < (0.2001 if weak else 0.1001), (got, want)
        elif not weak:
            assert w != 0.0 and abs(g - w) <= 0.11 * 10 ** (math.floor(math.log10(abs(w))) - 1) * 10, (got, want)
    return True, weak


def _table(case, h, seqs, **kw):
    """(rows, status, domain records, dom_off, flags, detail) of one model of a case, as the shim calls it."""
    from witch_amd.ehmm import EHMM, pack_queries
    e = EHMM([case.hmm_paths[h]])
    try:
        res, offs = pack_queries(seqs)
        deci, flags, det = e.score(res, offs, want_detail=True)
        rows = e.seq_table(res, offs, flags, det, **kw)
        st = e.last_seq_table_status()
        recs, dom_off = e.domains(res, offs, flags, det)
        return rows, st, recs, dom_off, flags, det
    finally:
        e.close()


@pytest.mark.parametrize("name", TABLE_CASES)
def test_seq_table_against_hmmsearch(name):
    """Every model of the case, searched alone as hmmsearch searches it: every integer column (reg clu ov env dom rep inc)
    equals HMMER's on every row; exp under the rule of tests/tblout_common.py; score, bias and the E-values identical as
    printed or one printed unit apart; no reg mismatch between the sweep and the scoring kernels, no capped row.  The best
    domain's bits, bias and lnP are wh_domains' values for that envelope, bit for bit."""
    _need_gpu()
    from witch_amd.shim import formats
    case, fx = load_case(name), tc.load_fixture(name)
    from tests.filters_common import digitize
    alph = {"dna": 0, "rna": 1, "amino": 2}.get(case.alphabet, case.alphabet)
    seqs = [digitize(alph, s.upper()) for s in case.qseqs]
    n = differ = exempt = nbest = nweak = weak_differ = 0
    for h, m in enumerate(fx["models"]):
        rows, st, recs, dom_off, flags, det = _table(case, h, seqs, E=99999999.0)
        assert st == {"rows": len(rows), "capped": 0, "reg_mismatch": 0, "any_size": 0}, (name, h, st)
        hdr = formats.hmm_header(case.hmm_paths[h])
        entries = formats.seq_table_entries(hdr, case.qnames, rows, len(seqs))
        assert [e["target"] for e in entries] == [r["target"] for r in m["rows"]], (name, h, "the rows or their order differ")
        for e, r, line in zip(entries, m["rows"], formats.format_tblout_lines(entries)):
            assert [e[k] for k in tc.INT_COLUMNS] == [int(r[k]) for k in tc.INT_COLUMNS], (name, h, r["raw"], e)
            ok, ex = tc.exp_ok(e["exp"], r["exp"])
            assert ok, (name, h, r["raw"], e["exp"])
            exempt += ex
            d, weak = _line_ok(line, r["raw"])
            differ += d and not weak
            nweak += weak
            weak_differ += d and weak
            n += 1
        # 7. the best domain of every row is the domain record of that envelope
        for row in rows:
            p, b = int(row["pair"]), int(row["best"])
            d = recs[dom_off[p] + b]
            assert (int(d["pair"]), int(d["index"])) == (p, b)
            for a, k in (("best_bits", "bits"), ("best_bias_bits", "bias_bits"), ("best_lnP", "lnP")):
                assert row[a].tobytes() == d[k].tobytes(), (name, h, p, a, row[a], d[k])
            assert float(row["best_bits"]) == max(float(x["bits"]) for x in recs[dom_off[p]:dom_off[p + 1]])
            nbest += 1
    print("[%s] %d rows, integer columns equal; %d without a clustered region, %d of them differ from HMMER's line by one printed "
          "unit; %d with one, %d of them differ; %d exp fields at a print boundary, %d best domains equal to the domain records bit "
          "for bit" % (name, n, n - nweak, differ, nweak, weak_differ, exempt, nbest))
    assert n == sum(len(m["rows"]) for m in fx["models"]) and exempt <= tc.EXEMPT_CAP * n and differ <= max(1, (n - nweak) // 20)


# ------------------------------------------------------------------------------------------------ 8. capped rows
def test_capped_rows_of_a_long_tandem_and_a_long_list(tmp_path):
    """A tandem of 18 copies (one multidomain region with more envelopes than a record lists) and the long-list query of
    tests/domains_reference.py (18 regions) come back with capped = 1 and reg = detail.nregions; a plain fragment does not."""
    _need_gpu()
    from witch_amd._lib import WH_MAX_ENVELOPES
    from witch_amd.ehmm import EHMM, pack_queries
    paths, names, seqs = dr.long_list_case(str(tmp_path))
    seqs = list(seqs) + [np.concatenate([seqs[1]] * 18)]
    e = EHMM(paths)
    try:
        res, offs = pack_queries(seqs)
        deci, flags, det = e.score(res, offs, want_detail=True)
        rows = e.seq_table(res, offs, flags, det)
        st = e.last_seq_table_status()
    finally:
        e.close()
    H = len(paths)
    by = {int(r["pair"]): r for r in rows}
    for h in range(H):
        long18, frag, tandem = by[0 * H + h], by[1 * H + h], by[2 * H + h]
        assert long18["capped"] == 1 and long18["reg"] == det[0 * H + h].nregions == 18 and long18["env"] == WH_MAX_ENVELOPES
        assert tandem["capped"] == 1 and tandem["reg"] == det[2 * H + h].nregions and tandem["env"] == WH_MAX_ENVELOPES and tandem["clu"] >= 1
        assert frag["capped"] == 0 and (frag["reg"], frag["env"], frag["dom"], frag["ov"]) == (1, 1, 1, 0)
    assert st["rows"] == len(rows) and st["capped"] == 2 * H and st["reg_mismatch"] == 0


def test_device_entry_points_on_a_stream(tmp_path):
    """wh_seq_table_dev / wh_seq_expect_dev on torch tensors and a side stream give the bytes of the host entry points;
    WH_ERANGE where the caller's capacity is too small; an empty pair list."""
    _need_gpu()
    import torch
    from witch_amd._lib import SEQ_EXPECT_FIELDS, SEQ_ROW_FIELDS, WitchHipError
    from witch_amd.ehmm import EHMM, pack_queries
    case = load_case("dna_hmmbuild")
    e = EHMM(case.hmm_paths[:3])
    try:
        seqs = [e.digitize(s) for s in case.qseqs[:20]]
        res, offs = pack_queries(seqs)
        deci, flags, det = e.score(res, offs, want_detail=True)
        host = e.seq_table(res, offs, flags, det)
        assert len(host) == int((flags & 1).sum()) > 0
        assert len(e.seq_expect(res, offs, [])) == 0
        dev = torch.device("cuda")
        det_t = torch.from_numpy(np.frombuffer(bytes(det), dtype=np.uint8).copy()).to(dev)
        res_t, offs_t, flags_t = torch.from_numpy(res).to(dev), torch.from_numpy(offs).to(dev), torch.from_numpy(flags).to(dev)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            rows_t = e.seq_table_t(res_t, offs_t, int(np.diff(offs).max()), flags_t, det_t)
            exp_t = e.seq_expect_t(res_t, offs_t, int(np.diff(offs).max()), torch.from_numpy(host["pair"].copy()).to(dev))
        side.synchronize()
        rows = np.frombuffer(rows_t.cpu().numpy().tobytes(), dtype=np.dtype(SEQ_ROW_FIELDS))
        exp = np.frombuffer(exp_t.cpu().numpy().tobytes(), dtype=np.dtype(SEQ_EXPECT_FIELDS))
        assert rows.tobytes() == host.tobytes()
        assert exp["exp"].tobytes() == host["exp"].tobytes() and np.array_equal(exp["clu"], host["clu"]) and np.array_equal(exp["reg"], host["reg"])
        with pytest.raises(WitchHipError):
            e.seq_table_t(res_t, offs_t, int(np.diff(offs).max()), flags_t, det_t, cap=len(host) - 1)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ 9. the shim
def test_shim_writes_tblout_like_hmmer(tmp_path):
    """hmmsearch --max -E 99999999 --tblout F through the server on dna_hmmbuild/A_0_0 gives HMMER's lines under the rules
    of test_seq_table_against_hmmsearch; a filtered run that also asks for --domtblout and -A writes all three files, its main
    output byte-identical to the same call without --tblout."""
    _need_gpu()
    import threading
    from witch_amd.shim.server import GpuBackend, Server, request
    case = load_case("dna_hmmbuild")
    m = tc.load_fixture("dna_hmmbuild")["models"][0]
    sock = str(tmp_path / "g.sock")
    if len(sock) > 100:
        import tempfile
        sock = os.path.join(tempfile.mkdtemp(prefix="wh_tbl_", dir="/tmp"), "g.sock")
    srv = Server(GpuBackend(0), sock)
    ready = threading.Event()
    threading.Thread(target=srv.serve_forever, args=(ready,), daemon=True).start()
    assert ready.wait(10)
    fa = os.path.join(case.dir, "queries.fasta")
    st, msg = request(sock, "hmmsearch", ["--cpu", "1", "--noali", "-E", "99999999", "--max", "-o", "o.txt", "--tblout", "t.tbl",
                                          case.hmm_paths[0], fa], cwd=str(tmp_path))
    assert st == 0, msg
    header, rows, trailer = tc.parse_tblout(open(tmp_path / "t.tbl").read())
    assert header == m["header"] and [r["target"] for r in rows] == [r["target"] for r in m["rows"]]
    differ = 0
    for g, w in zip(rows, m["rows"]):
        assert [g[k] for k in tc.INT_COLUMNS] == [w[k] for k in tc.INT_COLUMNS], (g["raw"], w["raw"])
        assert tc.exp_ok(float(g["exp"]), w["exp"])[0]
        d, weak = _line_ok(g["raw"], w["raw"])
        differ += d and not weak
    assert differ <= max(1, len(rows) // 20)
    assert trailer[0] == "#" and trailer[1:4] == m["trailer"][1:4] and trailer[-1] == "# [ok]" and any(t.startswith("# Date:") for t in trailer)
    plain_st, plain = request(sock, "hmmsearch", ["--cpu", "1", "--noali", "-E", "99999999", "--max", case.hmm_paths[0], fa], cwd=str(tmp_path))
    assert plain_st == 0 and plain == open(tmp_path / "o.txt").read()
    # a filtered search with all three files
    argv = ["--cpu", "1", "--noali", "-E", "99999999", "--nobias", "--domtblout", "d.tbl", "-A", "a.sto"]
    st, with_tbl = request(sock, "hmmsearch", argv + ["--tblout", "f.tbl", case.hmm_paths[0], fa], cwd=str(tmp_path))
    assert st == 0, with_tbl
    files = {f: open(tmp_path / f).read() for f in ("d.tbl", "a.sto", "f.tbl")}
    assert all(files.values())
    st, without = request(sock, "hmmsearch", argv + [case.hmm_paths[0], fa], cwd=str(tmp_path))
    assert st == 0 and without == with_tbl
    assert open(tmp_path / "d.tbl").read() == files["d.tbl"] and open(tmp_path / "a.sto").read() == files["a.sto"]
    frows = tc.parse_tblout(files["f.tbl"])[1]
    assert 0 < len(frows) <= len(rows) and set(r["target"] for r in frows) <= set(r["target"] for r in rows)
