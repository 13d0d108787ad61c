"""hmmsearch -A on the GPU (wh_domain_paths, wh_hits_msa_dev, wh_hits_msa, the level-0 hmmsearch): the hit selection alone on
hand-made device arrays against its numpy restatement (tests/hits_msa_reference.py), the domain paths against wh_domains and
wh_align, the whole chain against the bundled binary's -A files (tests/golden/hits_msa), and the shim.

Against the binary: the row names, their order, the "#=GS DE" lines and RF are compared; a row is compared by its match
columns and its insert residues; the names or rows that differ must be listed in the fixture's ref_mismatch (weak domains,
written by the generator from the CPU reference alone).  PP characters follow the guard band of tests/test_msa_gpu.py (the
float64 reference value within tol32(Ld) of a character boundary: one step apart at most; at most 1 % of a case's characters
in the band); a PP_cons character is compared where no contributing PP character lies in the band and no contributing row is
listed in ref_mismatch."""
import os
import threading

import numpy as np
import pytest

from tests import domains_reference as dr
from tests import hits_msa_reference as hr
from tests import msa_reference as mr
from tests.conftest import load_case
from tests.test_align_pp import BOUNDS, _need_gpu, _steps, tol32

pytestmark = pytest.mark.gpu
MAX_BAND = 0.01
KEYS = ("rows", "pp_rows", "pp_cons", "rf", "matmap")


# ------------------------------------------------------------------------------------------------ 1. the stage alone
class Shapes:
    """Two models (h = 1 is the one asked for) and hand-made records: per query its length, its sequence score relative to
    tau, and its domains on model 1 as (env_i, env_j, ali_i, ali_j, lnP); ali_i = 0: a domain without a path."""
    QUERIES = [
        # two included domains of one pair, overlapping envelopes, slices of 129 and 65 residues, ali inside env
        (300, +50.0, [(1, 140, 3, 131, -40.0), (120, 260, 130, 194, -30.0)]),
        (64, +50.0, [(1, 64, 1, 64, -40.0)]),                       # slice of 64: the envelope is the whole query
        (70, +50.0, [(2, 69, 5, 67, -40.0)]),                       # slice of 63
        (10, +50.0, [(3, 8, 5, 5, -40.0)]),                         # slice of 1
        (90, -1.0, [(1, 90, 2, 80, -40.0)]),                        # an excluded sequence with an includable domain
        (120, +50.0, [(1, 40, 0, 0, -40.0), (41, 120, 50, 114, -40.0)]),   # a pathless domain, then one of 65
        (30, None, []),                                             # not reported
        (100, +50.0, [(1, 50, 2, 49, -0.5), (51, 100, 52, 99, -40.0)]),    # an excluded domain, then an included one
    ]
    SPECIAL = [0.0499, 0.05, 0.9499, 0.95, 1.0, 0.0, 0.949999, 0.95000005, 0.15, 0.25, 0.849999]

    def __init__(self, device="cuda:0"):
        import torch
        from witch_amd import _lib
        from witch_amd.shim.formats import hmm_header
        case = load_case("dna_hmmbuild")
        hdr = hmm_header(case.hmm_paths[1])
        self.M = hdr["M"]
        self.tau, self.lam = float(np.float32(hdr["ftau"])), float(np.float32(hdr["flambda"]))     # (the library keeps them as floats)
        if device != "cpu":                                # (the construction itself needs no device: tests/test_hits_msa_host.py builds it too)
            from witch_amd.ehmm import EHMM
            self.e = EHMM(case.hmm_paths[:2])
            assert int(self.e.M[1]) == self.M
        rng = np.random.default_rng(20260101)
        H, nq = 2, len(self.QUERIES)
        self.nq = nq
        self.texts = ["".join("acgtACGT"[i] for i in rng.integers(0, 8, size=L)) for L, _, _ in self.QUERIES]
        offs = np.zeros(nq + 1, dtype=np.int64)
        offs[1:] = np.cumsum([q[0] for q in self.QUERIES])
        flags = np.zeros(nq * H, dtype=np.uint8)
        det = (_lib.PairDetail * (nq * H))()
        dom_off = np.zeros(nq * H + 1, dtype=np.int64)
        recs, env_off, cols, pps = [], [0], [], []
        self.doms, self.seq_lnp = [], []
        special = list(self.SPECIAL)
        for q, (L, rel, doms) in enumerate(self.QUERIES):
            for h in range(H):
                p = q * H + h
                mine = doms if h == 1 else doms[:1]                  # (model 0 has domains too: they are not model 1's)
                if rel is not None:
                    flags[p] = 1
                    det[p].seq_score = np.float32(self.tau + rel)
                    det[p].nenv = len(mine)
                out = []
                for t, (ei, ej, ai, aj, lnp) in enumerate(mine if rel is not None else []):
                    Ld = ej - ei + 1
                    c = np.full(Ld, -1, dtype=np.int32)
                    pp = rng.random(Ld).astype(np.float32)
                    if ai:
                        n = aj - ai + 1
                        # the slice's first and last residue are match states; of the others some are inserts
                        m = n if n <= 2 else max(2, min(n, self.M) - int(rng.integers(0, 4)))
                        inner = rng.choice(np.arange(1, n - 1), size=m - 2, replace=False) if n > 2 else np.zeros(0, dtype=np.int64)
                        at = np.unique(np.concatenate([[0, n - 1], inner])).astype(np.int64)
                        c[ai - ei + at] = np.sort(rng.choice(self.M, size=len(at), replace=False))
                        if h == 1 and special and n >= len(special) + 2:
                            pp[ai - ei + 1:ai - ei + 1 + len(special)] = special
                            special, self.special_row = [], (q, t)
                    rec = {"pair": p, "index": t, "of": len(mine), "env_i": ei, "env_j": ej, "ali_i": ai, "ali_j": aj,
                           "hmm_i": int(c[c >= 0].min()) + 1 if ai else 0, "hmm_j": int(c[c >= 0].max()) + 1 if ai else 0,
                           "bits": 1.0, "bias_bits": 0.0, "oasc": float(pp.sum()), "lnP": lnp}
                    recs.append(tuple(rec[k] for k, _ in _lib.DOMAIN_FIELDS))
                    env_off.append(env_off[-1] + Ld)
                    cols.append(c)
                    pps.append(pp)
                    out.append(dict(rec, cols=c, pp=pp))
                dom_off[p + 1] = dom_off[p] + len(out)
                if h == 1:
                    self.doms.append(out)
                    sc = float(np.float32(self.tau + rel)) if rel is not None else None
                    self.seq_lnp.append(None if sc is None else (0.0 if sc < self.tau else -self.lam * (sc - self.tau)))
        assert not special, "the quantisation values were not placed"
        dev = torch.device(device)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
        dom = np.array(recs, dtype=np.dtype(_lib.DOMAIN_FIELDS))
        self.t = dict(text_t=up(np.frombuffer("".join(self.texts).encode(), dtype=np.uint8).copy()), offsets_t=up(offs), flags_t=up(flags),
                      detail_t=up(np.frombuffer(bytes(det), dtype=np.uint8).copy()), dom_off_t=up(dom_off),
                      dom_t=up(dom.view(np.uint8).reshape(len(dom), -1)), env_off_t=up(np.array(env_off, dtype=np.int64)),
                      cols_t=up(np.concatenate(cols)), pp_t=up(np.concatenate(pps)))
        self.up = up

    def want(self, order, Z, domZ, incE, incdomE):
        rows = hr.select(order, self.seq_lnp, self.doms, hr.ln_thr(incE, Z), hr.ln_thr(incdomE, domZ))
        return hr.assemble_rows(self.M, rows, self.texts)

    def got(self, order, Z, domZ, incE, incdomE, no_lds=False):
        o = None if order is None else self.up(np.array(order, dtype=np.int32))
        return self.e.hits_msa_t(**self.t, Z=Z, domZ=domZ, incE=incE, incdomE=incdomE, h=1, order_t=o, no_lds=no_lds)


@pytest.fixture(scope="module")
def shapes():
    _need_gpu()
    s = Shapes()
    yield s
    s.e.close()


def _same(got, want, what):
    assert [tuple(int(x) for x in r) for r in got["row_recs"]] == [tuple(r) for r in want["row_recs"]], what
    assert got["W"] == want["W"], what
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), (what, k)


@pytest.mark.parametrize("order", ["none", "reversed", "shuffled"])
def test_stage_alone_against_numpy(shapes, order):
    """Slices of 1, 63, 64, 65 and 129 residues, ali inside env at both ends, two included domains of one pair with
    overlapping envelopes, an excluded sequence, an excluded and a pathless domain, an unreported pair, domains of the other
    model, the posteriors at the quantisation's edges: row records, rows, PP rows, PP_cons, RF and matmap bitwise."""
    s = shapes
    nat = list(range(s.nq))
    o = {"none": None, "reversed": nat[::-1], "shuffled": [3, 0, 7, 5, 1, 6, 2, 4]}[order]
    want = s.want(o or nat, 8, 6, 0.01, 0.01)
    got = s.got(o, 8, 6, 0.01, 0.01)
    assert sorted(int(r[3]) - int(r[2]) + 1 for r in got["row_recs"]) == [1, 48, 63, 64, 65, 65, 129]
    _same(got, want, order)
    _same(s.got(o, 8, 6, 0.01, 0.01, no_lds=True), want, (order, "global"))
    # the PP rows are the characters of the real posteriors, in HMMER's own arithmetic
    row = [i for i, r in enumerate(want["row_recs"]) if tuple(r[:2]) == s.special_row][0]
    cols = want["cols"][row]
    line = got["pp_rows"][row]
    first = [i for i, c in enumerate(line) if c != ord(".")][0]
    # (residues 1.. of the slice follow its first residue in the row where they are match states or inserts of block order)
    chars = "".join(chr(c) for c in line[first:] if c != ord("."))
    assert len(chars) == len(cols) and chars[1:1 + len(s.SPECIAL)] == "".join(hr.encode(p) for p in s.SPECIAL) == "0199*09*238"


def test_stage_alone_none_and_all_included(shapes):
    s = shapes
    nat = list(range(s.nq))
    got = s.got(None, 8, 6, 0.0, 0.0)
    assert len(got["row_recs"]) == 0 and got["W"] == s.M and got["rows"].shape == (0, s.M) and got["rf"].tobytes() == b"x" * s.M
    got = s.got(None, 8, 6, 1e-300, 1e-300)
    assert len(got["row_recs"]) == 0 and got["W"] == s.M
    want = s.want(nat, 8, 6, 1e9, 1e9)                    # everything with a path; the pathless domain never
    got = s.got(None, 8, 6, 1e9, 1e9)
    assert len(got["row_recs"]) == 9 and (5, 0, 0, 0) not in [tuple(int(x) for x in r) for r in got["row_recs"]]
    _same(got, want, "all")
    # the sequence threshold and the domain threshold are separate decisions
    _same(s.got(None, 8, 6, 1e9, 0.01), s.want(nat, 8, 6, 1e9, 0.01), "all sequences")
    _same(s.got(None, 8, 6, 0.01, 1e9), s.want(nat, 8, 6, 0.01, 1e9), "all domains")


def test_stage_alone_refuses(shapes):
    from witch_amd._lib import WitchHipError
    s = shapes
    for kw in ({"Z": 0.0, "domZ": 6}, {"Z": 8, "domZ": -1.0}):
        with pytest.raises(WitchHipError, match="wh_hits_msa_dev"):
            s.e.hits_msa_t(**s.t, h=1, **kw)
    with pytest.raises(WitchHipError, match="wh_hits_msa_dev"):
        s.e.hits_msa_t(**s.t, Z=8, domZ=6, h=2)
    with pytest.raises(WitchHipError, match="order"):
        s.got([0, 1, 2, 3, 4, 5, 6, 8], 8, 6, 0.01, 0.01)
    bad = dict(s.t)
    bad["dom_off_t"] = s.t["dom_off_t"].clone()
    bad["dom_off_t"][3] += 1                              # a dom_off that does not fit the records
    with pytest.raises(WitchHipError, match="dom_off"):
        s.e.hits_msa_t(**bad, Z=8, domZ=6, h=1)


# ------------------------------------------------------------------------------------------------ 2. wh_domain_paths
def test_domain_paths_are_wh_domains_and_wh_align():
    _need_gpu()
    from witch_amd.ehmm import EHMM, pack_queries
    case = load_case("dna_hmmbuild")
    e = EHMM(case.hmm_paths[:3])
    try:
        seqs = [e.digitize(s.upper()) for s in case.qseqs[:16]]
        res, offs = pack_queries(seqs)
        deci, flags, det = e.score(res, offs, want_detail=True)
        want, want_off = e.domains(res, offs, flags, det)
        recs, dom_off, env_off, cols, pp = e.domain_paths(res, offs, flags, det)
        assert np.array_equal(dom_off, want_off) and recs.tobytes() == want.tobytes() and len(recs) > 16
        assert np.array_equal(np.diff(env_off), recs["env_j"] - recs["env_i"] + 1) and len(cols) == len(pp) == env_off[-1]
        envs = [seqs[int(r["pair"]) // e.H][r["env_i"] - 1:r["env_j"]] for r in recs]
        eres, eoffs = pack_queries(envs)
        acols, aco, app = e.align(eres, eoffs, np.arange(len(envs)), (recs["pair"] % e.H).astype(np.int32), want_pp=True)
        assert np.array_equal(aco, env_off) and np.array_equal(acols, cols) and np.array_equal(app, pp)
        for r, lo in zip(recs, env_off[:-1]):
            hit = np.nonzero(cols[lo:lo + r["env_j"] - r["env_i"] + 1] >= 0)[0]
            assert (r["ali_i"], r["ali_j"]) == ((r["env_i"] + hit[0], r["env_i"] + hit[-1]) if len(hit) else (0, 0))
        # wh_domains itself is what it was: a second call gives the same bytes
        again, _ = e.domains(res, offs, flags, det)
        assert again.tobytes() == want.tobytes()
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ 3. against the binary
_backend = []


def _gpu_backend():
    _need_gpu()
    from witch_amd.shim.server import GpuBackend
    if not _backend:
        _backend.append(GpuBackend(0))
    return _backend[0]


def _reference_pp(case_name, h, names):
    """{(query name, ali_i, ali_j): (float64 posteriors of the slice, tolerance)} from the oracle's domain records."""
    seqs, dom = dr.case_reference(case_name)
    qn = dr.load_fixture(case_name)["queries"]
    out = {}
    for q, n in enumerate(qn):
        if n in names:
            for d in dom[(q, h)]:
                if d["ali_i"]:
                    i0 = d["ali_i"] - d["env_i"]
                    out[(n, d["ali_i"], d["ali_j"])] = (np.asarray(d["pp"][i0:d["ali_j"] - d["env_i"] + 1]), tol32(len(d["pp"])))
    return out


def compare_with_binary(tag, text, run, allowed, ref_pp, counts):
    """The conditions of the module's docstring for our -A text against the fixture's; returns True where the two files are
    byte-identical."""
    want = run["sto"]
    if text == want:
        return True
    ours, theirs = mr.parse_msa(text), mr.parse_msa(want)
    (on, od), (tn, td) = hr.parse_gs(text), hr.parse_gs(want)
    allowed = set(allowed)
    assert [n for n in on if n not in allowed] == [n for n in tn if n not in allowed], (tag, "names or their order")
    assert set(on) ^ set(tn) <= allowed, (tag, sorted(set(on) ^ set(tn)))
    assert [n.split("/")[0] for n in on] == [n.split("/")[0] for n in tn], (tag, "sequences or their order")
    assert ours[3].count("x") == theirs[3].count("x")
    M = ours[3].count("x")
    dirty, banded = np.zeros(M, dtype=bool), np.zeros(M, dtype=bool)
    for n in set(on) | set(tn):
        if n in allowed:
            for parsed in (ours, theirs):
                if n in parsed[0]:
                    dirty |= np.array([c != "-" for c, r in zip(parsed[0][n], parsed[3]) if r == "x"])
            continue
        assert od[n] == td[n], (tag, n, "DE")
        assert hr.match_and_inserts(ours[0][n], ours[3]) == hr.match_and_inserts(theirs[0][n], theirs[3]), (tag, n)
        name, rng_ = n.rsplit("/", 1)
        ai, aj = (int(x) for x in rng_.split("-"))
        ref, tol = ref_pp[(name, ai, aj)]
        band = np.min(np.abs(ref[:, None] - BOUNDS[None, :]), axis=1) <= tol
        cols, mine = mr.decode_row(ours[0][n], ours[1][n], ours[3])
        _, bins = mr.decode_row(theirs[0][n], theirs[1][n], theirs[3])
        assert len(mine) == len(bins) == len(ref), (tag, n)
        counts[0] += len(ref)
        counts[1] += int(band.sum())
        for i, (x, y) in enumerate(zip(mine, bins)):
            assert x == y or (band[i] and _steps(x, y) == 1), (tag, n, i, x, y, ref[i])
        banded[cols[(cols >= 0) & band]] = True
    oc = [c for c, r in zip(ours[2], ours[3]) if r == "x"]
    tc = [c for c, r in zip(theirs[2], theirs[3]) if r == "x"]
    for k in range(M):
        if not dirty[k] and not banded[k]:
            assert oc[k] == tc[k], (tag, "PP_cons", k, oc[k], tc[k])
    if not allowed:
        assert ours[3] == theirs[3], (tag, "RF")
    return False


def _hits_text(case_name, model, key):
    """Our -A text and trailer for a fixture run, through GpuBackend.search_hits and the shim's formatter."""
    from witch_amd.shim import formats
    case = load_case(case_name)
    run = model["runs"][key]
    at = {n: i for i, n in enumerate(case.qnames)}
    records = [(n, case.qseqs[at[n]]) for n in run["queries"]]
    inc = {"incE": 0.01, "incdomE": 0.01}
    for o, v in zip(run["args"][::2], run["args"][1::2]):
        if o in ("--incE", "--incdomE"):
            inc[o[2:]] = float(v)
    hdr, rows, domains, hits = _gpu_backend().search_hits(case.hmm_paths[model["h"]], records, inc, want_domains=True)
    text = formats.format_hits_msa([n for n, _ in records], hits["row_recs"], hits["rows"], hits["pp_rows"], hits["pp_cons"], hits["rf"],
                                   descriptions=run["desc"], notextw="--notextw" in run["args"])
    return text, formats.hits_msa_trailer(len(hits["row_recs"]), "ALI"), (hdr, rows, domains, hits, records, inc)


@pytest.mark.parametrize("case_name", list(hr.MODELS))
def test_end_to_end_against_the_binary(case_name):
    fx = hr.load_fixture(case_name)
    counts, identical, n_files = [0, 0], 0, 0
    for model in fx["models"]:
        ref_pp = _reference_pp(case_name, model["h"], set(fx["queries"]))
        for key in sorted(model["runs"]):
            run = model["runs"][key]
            text, trailer, ctx = _hits_text(case_name, model, key)
            tag = (case_name, model["h"], key)
            assert trailer == run["trailer"], tag
            allowed = model["ref_mismatch"] if key == "a" else model["ref_mismatch_b"]
            if key in ("inc", "none"):
                allowed = [n for n in allowed if n in run["sto"]]
            identical += compare_with_binary(tag, text, run, allowed, ref_pp, counts)
            n_files += 1
            if key == "a":
                # 4a. the rows of the alignment are the domains marked '!' in the shim's domain tables of the same call
                from witch_amd.shim import formats
                hdr, rows, domains, hits, records, inc = ctx
                ent = formats.domain_entries(hdr, rows, {n: len(t) for n, t in records}, domains, len(records), **inc)
                marked = ["%s/%d-%d" % (e["target"], e["ali_from"], e["ali_to"]) for e in ent if e["included"] and e["ali_from"]]
                assert marked == hr.parse_gs(text)[0] and len(marked) > 0, tag
    print("%s: %d of %d files byte-identical to the binary's; %d PP characters compared, %d in the guard band" %
          (case_name, identical, n_files, counts[0], counts[1]))
    assert counts[1] <= MAX_BAND * max(counts[0], 1), (case_name, counts)


# ------------------------------------------------------------------------------------------------ 4. level 0
def test_level0_hmmsearch_writes_the_file(tmp_path):
    """hmmsearch -A through a resident Server(GpuBackend): the file of (b) on amino_hmmbuild model 0, with the FASTA
    description, the trailer line behind "//", --domtblout in the same call, --notextw, and nothing included."""
    _need_gpu()
    import shutil
    import tempfile
    from witch_amd.shim.server import Server, request
    case_name = "amino_hmmbuild"
    fx = hr.load_fixture(case_name)
    model = fx["models"][0]
    case = load_case(case_name)
    run = model["runs"]["b"]
    at = {n: i for i, n in enumerate(case.qnames)}
    fa = tmp_path / "q.fa"
    fa.write_text("".join(">%s%s\n%s\n" % (n, " " + run["desc"][n] if n in run["desc"] else "", case.qseqs[at[n]]) for n in run["queries"]))
    hmm = case.hmm_paths[model["h"]]
    ref_pp = _reference_pp(case_name, model["h"], set(run["queries"]))
    d = tempfile.mkdtemp(prefix="wh_sock_", dir="/tmp")
    try:
        sock = os.path.join(d, "s.sock")
        srv = Server(_gpu_backend(), sock)
        ready = threading.Event()
        threading.Thread(target=srv.serve_forever, args=(ready,), daemon=True).start()
        assert ready.wait(10)
        base = ["--cpu", "1", "--noali", "-E", "99999999", "--max"]
        status, plain = request(sock, "hmmsearch", base + [hmm, str(fa)], cwd=str(tmp_path))
        assert status == 0
        for key, extra in (("b", []), ("notextw", ["--notextw"]), ("none", ["--incE", "1e-200", "--incdomE", "1e-200"]),
                           ("b", ["--domtblout", "d.tbl"])):
            status, body = request(sock, "hmmsearch", base + ["-A", "ALI"] + extra + [hmm, str(fa)], cwd=str(tmp_path))
            assert status == 0, body
            want = model["runs"][key]
            lines = body.splitlines()
            assert lines[lines.index("//") + 1] == want["trailer"] and lines[-1] == "[ok]", key
            if "--domtblout" not in extra:
                assert [ln for ln in lines if ln != want["trailer"]] == plain.splitlines(), "the tables of a call without -A"
            else:
                assert (tmp_path / "d.tbl").read_text().startswith("#")
            out = (tmp_path / "ALI").read_text()
            counts = [0, 0]
            same = compare_with_binary((key, tuple(extra)), out, want, model["ref_mismatch_b"], ref_pp, counts)
            assert counts[1] <= MAX_BAND * max(counts[0], 1)
            print("level 0, %s %s: %d bytes, file %s the binary's" % (key, extra, len(out), "is" if same else "differs inside the band from"))
    finally:
        shutil.rmtree(d, ignore_errors=True)
