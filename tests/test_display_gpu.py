"""hmmsearch's alignment display on the GPU (wh_domain_display_dev, wh_domain_display, the level-0 hmmsearch with
WITCH_HIP_ALIDISPLAY=1): the stage alone on hand-made device arrays against its restatement (tests/display_reference.py), the
whole path score -> domain_paths -> domain_display against the restatement applied to the device's own columns and
posteriors, the server's output against the bundled binary's section (tests/golden/display), and the one shared domain stage.

Against the binary, on every domain whose four coordinates are HMMER's and that is outside the fixture's recorded list: the
model, match and target lines are HMMER's bytes (test_three_lines_against_the_binary).  The PP line
(test_pp_line_against_the_binary) is HMMER's except at characters where the device's float32 posterior lies within
tests/test_align_pp.tol32(Ld) of a tenth boundary (x.x5); those are counted and printed.  The server's PP line is decoded
under the length model of the whole sequence, as hmmsearch decodes an envelope (EHMM.sequence_model_posteriors: the envelope
padded with residues no match state can emit).  Measured on the device: 664 domains, 74 424
characters, 0 differ - none inside the band either.  With the domain stage's own posteriors (hmmalign's, under the
envelope's length model) 114 characters on 63 domains differed beyond the band."""
import numpy as np
import pytest

from tests import display_reference as ref
from tests.conftest import load_case
from tests.test_align_pp import _need_gpu, tol32

pytestmark = pytest.mark.gpu
POISON = 0xA5


# ------------------------------------------------------------------------------------------------ 1. the stage alone
def _path(kind, M, rng):
    """The 0-based nodes (-1: insert) of the residues ali_i..ali_j of a hand-made path; first and last are match states."""
    if kind == "one":                                   # one column: hmm_i == hmm_j
        return [int(rng.integers(0, M))]
    if kind.startswith("match"):                        # n match states in a row: n columns
        n = int(kind[5:])
        a = int(rng.integers(0, M - n + 1))
        return list(range(a, a + n))
    if kind.startswith("cols"):                         # n columns of match, insert and delete states
        n = int(kind[4:])
        if n == 1:
            return [int(rng.integers(0, M))]
        n_nodes = max(2, min(M, (7 * n) // 10))        # columns that are nodes; the others are inserts
        typ = np.array(["m"] * n)
        inner = rng.permutation(np.arange(1, n - 1))
        typ[inner[:n - n_nodes]] = "i"
        rest = inner[n - n_nodes:]
        typ[rest[:len(rest) // 6]] = "d"
        nodes, k = [], int(rng.integers(0, M - n_nodes + 1)) - 1
        for t in typ:
            k += t != "i"
            if t != "d":
                nodes.append(k if t == "m" else -1)
        return nodes
    if kind == "insert_run":                            # inserts over the boundary between two trips of 64 residues
        return list(range(3, 63)) + [-1] * 11 + list(range(63, 80))
    if kind == "insert_run2":                           # ... and a run that fills a whole trip
        return list(range(0, 30)) + [-1] * 150 + list(range(30, 40))
    if kind == "delete_run":                            # more than 64 delete states between two match states
        return [1, 2, 2 + 71, 2 + 72, -1, 2 + 72 + 5]
    raise ValueError(kind)


def nodes_max(nodes):
    return max(x for x in nodes if x >= 0)


class Stage:
    """Hand-made records, columns and posteriors for the models of a fixture case: per query (length, reported, [(model
    position, env_i, ali_i, lnP, path kind)]); the envelope ends 2 residues behind ali_j where the query has room."""

    def __init__(self, case_name, H, h, queries, seed, identity=(), device="cuda:0"):
        from witch_amd import _lib
        case = load_case(case_name)
        self.H, self.h = H, h
        models = [ref.DisplayModel.from_path(p) for p in case.hmm_paths[:H]]
        self.model = models[h]
        self.alphabet = self.model.alphabet
        K = 4 if self.alphabet != 2 else 20
        Kp = self.model.Kp
        valid = [x for x in range(Kp) if x != K and x < Kp - 2]
        degen = [x for x in valid if x > K]
        rng = np.random.default_rng(seed)
        nq = len(queries)
        self.seqs = [rng.choice(valid, size=L).astype(np.uint8) for L, _, _ in queries]
        offs = np.zeros(nq + 1, dtype=np.int64)
        offs[1:] = np.cumsum([q[0] for q in queries])
        flags = np.zeros(nq * H, dtype=np.uint8)
        dom_off = np.zeros(nq * H + 1, dtype=np.int64)
        recs, env_off, cols, pps = [], [0], [], []
        self.kinds = []
        for q, (L, reported, doms) in enumerate(queries):
            for hh in range(H):
                p = q * H + hh
                flags[p] = 1 if reported else 0
                mine = [d for d in doms if d[0] == hh]
                for t, (_, ei, ai, lnp, kind) in enumerate(mine):
                    nodes = _path(kind, models[hh].M, rng) if kind else []
                    aj = ai + len(nodes) - 1 if kind else 0
                    ej = min(L, aj + 2) if kind else min(L, ei + 9)
                    assert 1 <= ei <= (ai or ei) and aj <= ej <= L, (q, kind)
                    c = np.full(ej - ei + 1, -1, dtype=np.int32)
                    if kind:
                        c[ai - ei:aj - ei + 1] = nodes
                    pp = rng.random(ej - ei + 1).astype(np.float32)
                    pp[:6] = [0.9499999, 0.95, 0.05, 0.0499999, 1.0, 0.0][:len(pp[:6])]
                    if kind and hh == h:
                        at = [i for i, x in enumerate(nodes) if x >= 0]
                        s = self.seqs[q]
                        # degenerate codes on a match and on an insert position, an identity against the consensus letter
                        s[ai - 1 + at[len(at) // 2]] = rng.choice(degen)
                        ins = [i for i, x in enumerate(nodes) if x < 0]
                        if ins:
                            s[ai - 1 + ins[0]] = rng.choice(degen)
                        for i in (at if (q, t) in identity else at[:1]):
                            s[ai - 1 + i] = self.model.code[nodes[i] + 1]
                    rec = {"pair": p, "index": t, "of": len(mine), "env_i": ei, "env_j": ej, "ali_i": ai if kind else 0, "ali_j": aj,
                           "hmm_i": nodes[0] + 1 if kind else 0, "hmm_j": nodes_max(nodes) + 1 if kind else 0, "bits": 1.0, "bias_bits": 0.0,
                           "oasc": float(pp.sum()), "lnP": lnp}
                    recs.append(tuple(rec[k] for k, _ in _lib.DOMAIN_FIELDS))
                    env_off.append(env_off[-1] + len(c))
                    cols.append(c)
                    pps.append(pp)
                    if hh == h:
                        self.kinds.append((q, t, kind, lnp, reported))
                dom_off[p + 1] = dom_off[p] + len(mine)
        self.dom = np.array(recs, dtype=np.dtype(_lib.DOMAIN_FIELDS))
        self.flags, self.dom_off, self.env_off = flags, dom_off, np.array(env_off, dtype=np.int64)
        self.cols, self.pp = np.concatenate(cols), np.concatenate(pps)
        self.offs = offs
        if device == "cpu":                                # (the construction itself needs no device)
            return
        import torch
        from witch_amd.ehmm import EHMM
        self.e = EHMM(case.hmm_paths[:H])
        assert [int(m) for m in self.e.M] == [m.M for m in models]
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)      # noqa: E731
        self.t = dict(residues_t=up(np.concatenate(self.seqs)), offsets_t=up(offs), flags_t=up(flags), dom_off_t=up(dom_off),
                      dom_t=up(self.dom.view(np.uint8).reshape(len(self.dom), -1)), env_off_t=up(self.env_off), cols_t=up(self.cols),
                      pp_t=up(self.pp))

    def want(self, domE, domZ):
        return ref.display(self.model, self.seqs, self.flags, self.dom, self.dom_off, self.env_off, self.cols, self.pp, self.H, self.h, domE, domZ)

    def got(self, domE, domZ, **kw):
        return self.e.domain_display_t(**self.t, domE=domE, domZ=domZ, h=self.h, poison=POISON, **kw)


KINDS = ["one", "match63", "match64", "match65", "cols129", "cols1", "cols63", "cols64", "cols65", "insert_run", "insert_run2", "delete_run"]


def _queries(H, h):
    other = (h + 1) % H
    q = []
    for i, kind in enumerate(KINDS):
        doms = [(h, 3, 5, -40.0, kind)]
        if H > 1 and i % 3 == 0:
            doms.append((other, 1, 2, -40.0, "match63"))              # a domain of another model: not this model's
        q.append((330, True, doms))
    # selected and unselected domains alternating in one pair (lnP -40 / -0.25 against ln(domE / domZ) = ln(1e-3 / 6) = -8.7)
    q.append((400, True, [(h, 1 + 40 * t, 3 + 40 * t, -40.0 if t % 2 == 0 else -0.25, "cols%d" % (20 + t)) for t in range(8)]))
    # the two overlapping envelopes of one pair of tests/test_domains.py: 1-43 and 41-80
    q.append((80, True, [(h, 1, 2, -40.0, "match40"), (h, 41, 43, -40.0, "match36")]))
    q.append((90, False, [(h, 1, 2, -40.0, "match63")]))                # not reported
    q.append((60, True, [(h, 1, 0, -40.0, None), (h, 11, 12, -40.0, "match40")]))   # a domain without a path, then one with
    q.append((70, True, [(h, 2, 4, float("nan"), "cols50")]))           # no E-value (a model without STATS): selected
    return q


@pytest.fixture(scope="module", params=["dna", "amino"])
def stage(request):
    _need_gpu()
    if request.param == "dna":
        s = Stage("dna_hmmbuild", 2, 1, _queries(2, 1), 20261021, identity={(1, 0)})
    else:
        s = Stage("amino_hmmbuild", 1, 0, _queries(1, 0), 20261022, identity={(1, 0), (2, 0)})
    yield s
    s.e.close()


def _untouched(got):
    raw, tot, ns = got["raw"], got["total"], got["nsel"]
    assert np.all(raw["lines"][:, tot:] == POISON), "a byte beyond disp_off[nsel] was written"
    assert np.all(raw["disp_off"][ns + 1:] == -1) and np.all(raw["recs"][ns:] == POISON)


def test_stage_alone_against_the_restatement(stage):
    """Every shape of KINDS, alternating selection, overlapping envelopes, an unreported pair, a pathless domain, a NaN
    lnP, domains of another model, degenerate codes, identities: records, CSR and the four lines byte for byte, nothing
    written beyond them."""
    s = stage
    got, want = s.got(1e-3, 6.0), s.want(1e-3, 6.0)
    assert ref.same(got, want) is None, ref.same(got, want)
    _untouched(got)
    lens = np.diff(want["disp_off"])
    assert {1, 63, 64, 65, 129} <= set(int(x) for x in lens), sorted(set(int(x) for x in lens))
    assert want["nsel"] == len(KINDS) + 4 + 2 + 1 + 1
    text = want["match"].tobytes().decode()
    assert "+" in text and any(c.islower() for c in text) and (s.alphabet != 2 or any(c.isupper() for c in text))
    assert b"-" * 65 in want["target"].tobytes()                     # the delete run of more than 64 nodes
    # room for exactly the lines: served; one byte less: refused, nothing rendered
    exact = s.got(1e-3, 6.0, cap=int(want["disp_off"][-1]))
    assert ref.same(exact, want) is None
    from witch_amd._lib import WitchHipError
    with pytest.raises(WitchHipError, match="wh_domain_display_dev"):
        s.got(1e-3, 6.0, cap=int(want["disp_off"][-1]) - 1)


def test_stage_alone_thresholds(stage):
    s = stage
    # no pair reported: WH_OK, nothing selected, nothing rendered
    t = dict(s.t, flags_t=s.t["flags_t"] * 0)
    none = s.e.domain_display_t(**t, domE=10.0, domZ=6.0, h=s.h, poison=POISON)
    assert none["nsel"] == 0 and none["total"] == 0 and list(none["disp_off"]) == [0]
    assert np.all(none["raw"]["lines"] == POISON)
    # domE = 0: the one domain without an E-value (lnP NaN) alone
    zero = s.got(0.0, 6.0)
    assert ref.same(zero, s.want(0.0, 6.0)) is None and zero["nsel"] == 1
    _untouched(zero)
    for domE, domZ in ((10.0, 6.0), (1e-12, 1.0)):
        got, want = s.got(domE, domZ), s.want(domE, domZ)
        assert ref.same(got, want) is None, (domE, ref.same(got, want))
        _untouched(got)
    assert s.want(1e-12, 1.0)["nsel"] == s.want(1e-3, 6.0)["nsel"] == s.want(10.0, 6.0)["nsel"] - 4


def test_stage_alone_refuses(stage):
    from witch_amd._lib import WitchHipError
    s = stage
    for kw in ({"domE": 10.0, "domZ": 0.0}, {"domE": -1.0, "domZ": 6.0}):
        with pytest.raises(WitchHipError, match="wh_domain_display_dev"):
            s.e.domain_display_t(**s.t, h=s.h, **kw)
    with pytest.raises(WitchHipError, match="out of range"):
        s.e.domain_display_t(**s.t, domE=10.0, domZ=6.0, h=s.H)
    bad = dict(s.t)
    bad["cols_t"] = s.t["cols_t"].clone()
    d = next(i for i in range(len(s.dom)) if s.dom[i]["ali_i"] and s.dom[i]["ali_j"] - s.dom[i]["ali_i"] >= 4 and s.dom[i]["pair"] % s.H == s.h)
    at = int(s.env_off[d]) + int(s.dom[d]["ali_i"] - s.dom[d]["env_i"])
    bad["cols_t"][at + 2] = bad["cols_t"][at]                           # a path whose nodes do not rise
    with pytest.raises(WitchHipError, match="path"):
        s.e.domain_display_t(**bad, domE=10.0, domZ=6.0, h=s.h)
    bad = dict(s.t)
    bad["dom_off_t"] = s.t["dom_off_t"].clone()
    bad["dom_off_t"][3] += 1
    with pytest.raises(WitchHipError, match="dom_off"):
        s.e.domain_display_t(**bad, domE=10.0, domZ=6.0, h=s.h)


def test_models_out_of_scope_are_refused_by_name(tmp_path):
    """An edited copy of a fixture model: "RF yes" and a header without CONS are refused with the header key named; the
    handle's getter gives the file's column."""
    _need_gpu()
    from witch_amd._lib import WitchHipError
    from witch_amd.ehmm import EHMM, pack_queries
    case = load_case("dna_hmmbuild")
    text = open(case.hmm_paths[0]).read()
    (tmp_path / "rf.hmm").write_text(text.replace("RF    no", "RF    yes"))
    (tmp_path / "nocons.hmm").write_text(text.replace("CONS  yes", "CONS  no"))
    e = EHMM([case.hmm_paths[0], str(tmp_path / "rf.hmm"), str(tmp_path / "nocons.hmm")])
    assert e.consensus_letters(0) == ref.consensus_column(case.hmm_paths[0])[0] == e.consensus_letters(1) and e.consensus_letters(2) is None
    res, offs = pack_queries([e.digitize(s) for s in case.qseqs[:3]])
    deci, flags, det = e.score(res, offs, want_detail=True)
    assert e.domain_display(res, offs, flags, det, h=0)["nsel"] > 0
    for h, key in ((1, "RF yes"), (2, "CONS")):
        with pytest.raises(WitchHipError, match="wh_domain_display.*" + key):
            e.domain_display(res, offs, flags, det, h=h)
    e.close()


# ------------------------------------------------------------------------------------------------ 2. the whole path
@pytest.mark.parametrize("case_name,H,nq,hs", [("dna_hmmbuild", 8, 50, (0, 3, 7)), ("amino_hmmbuild", 4, 44, (0, 1, 2, 3)),
                                              ("amino_multidomain", 1, None, (0,))])
def test_whole_path_against_the_restatement(case_name, H, nq, hs):
    """score -> domain_paths -> domain_display: the device's lines are the restatement applied to the device's own columns
    and posteriors, byte for byte on every domain, and the records are wh_domains' bit for bit."""
    _need_gpu()
    from witch_amd.ehmm import EHMM, pack_queries
    case = load_case(case_name)
    e = EHMM(case.hmm_paths[:H])
    seqs = [e.digitize(s.upper()) for s in (case.qseqs if nq is None else case.qseqs[:nq])]
    res, offs = pack_queries(seqs)
    deci, flags, det = e.score(res, offs, want_detail=True)
    dom, dom_off, env_off, cols, pp = e.domain_paths(res, offs, flags, det)
    plain, _ = e.domains(res, offs, flags, det)
    n = 0
    for h in hs:
        domZ = max(int((flags[:, h] & 1).sum()), 1)
        got = e.domain_display(res, offs, flags, det, domE=10.0, domZ=domZ, h=h, want_domains=True)
        assert got["domains"].tobytes() == plain.tobytes() == dom.tobytes()
        want = ref.display(ref.DisplayModel.from_path(case.hmm_paths[h]), seqs, flags, dom, dom_off, env_off, cols, pp, H, h, 10.0, domZ)
        assert ref.same(got, want) is None, (case_name, h, ref.same(got, want))
        n += got["nsel"]
    e.set_timing(True)
    e.domain_display(res, offs, flags, det, h=hs[0])
    ms9, n9 = e.last_kernel_ms(9)
    ms5, _ = e.last_kernel_ms(5)
    print("[%s] %d domains displayed; display stage %.3f ms in %d launches, domain stage %.3f ms" % (case_name, n, ms9, n9, ms5))
    assert n > 0 and n9 == 4 and ms9 > 0
    e.close()


# ------------------------------------------------------------------------------------------------ 3. against the binary
_BACKEND = {}


def _server():
    from witch_amd.shim.server import GpuBackend, Server
    if "be" not in _BACKEND:
        _BACKEND["be"] = GpuBackend(0)
    srv = Server.__new__(Server)
    srv.backend = _BACKEND["be"]
    return srv


def _coords(lines):
    """(hmm from, hmm to, ali from, ali to) of a domain's block lines (header, then four lines per block, a blank between)."""
    return lines[1].split()[1], lines[-4].split()[-1], lines[3].split()[1], lines[-2].split()[-1]


@pytest.fixture(scope="module")
def binary_runs(tmp_path_factory):
    """Every run of the fixtures through the level-0 server with the opt-in set: [(case, h, run, HMMER's parsed section, ours,
    recorded list, {(name, domain number): (device posteriors of ali_i..ali_j without the delete columns' gaps, Ld)})]."""
    _need_gpu()
    import os
    tmp = tmp_path_factory.mktemp("display")
    old = os.environ.get("WITCH_HIP_ALIDISPLAY")
    os.environ["WITCH_HIP_ALIDISPLAY"] = "1"
    out = []
    try:
        srv = _server()
        for case_name in ref.MODELS:
            fx, case = ref.load_fixture(case_name), load_case(case_name)
            names = fx["queries"]
            fa = tmp / (case_name + ".fa")
            fa.write_text("".join(">%s\n%s\n" % (n, s) for n, s in zip(names, case.qseqs[:len(names)])))
            for model in fx["models"]:
                hp = case.hmm_paths[model["h"]]
                e, _ = srv.backend.model(hp)
                from witch_amd.ehmm import pack_queries
                seqs = [e.digitize(s.upper()) for s in case.qseqs[:len(names)]]
                res, offs = pack_queries(seqs)
                deci, flags, det = e.score(res, offs, want_detail=True)
                dom, dom_off, env_off, cols, pp = e.domain_paths(res, offs, flags, det)
                pp = e.sequence_model_posteriors(res, offs, dom, env_off, cols, pp, h=0)      # (what the server's display prints)
                for run, r in model["runs"].items():
                    text = srv.run_hmmsearch(["--max", "-E", "99999999"] + r["args"] + [hp, str(fa)], str(tmp))
                    _, ours, order = ref.parse_section(ref.section(text))
                    _, theirs, order_t = ref.parse_section(r["section"])
                    assert order == order_t, (case_name, model["h"], run)
                    post = {}
                    for q, name in enumerate(names):
                        nd = 0
                        for d in range(int(dom_off[q]), int(dom_off[q + 1])):
                            shown = ours.get(name, {"domains": {}})["domains"]
                            lnp = float(dom[d]["lnP"])
                            domE = float(r["args"][r["args"].index("--domE") + 1]) if "--domE" in r["args"] else 10.0
                            if int(dom[d]["ali_i"]) and lnp <= ref.ln_thr(domE, max(int((flags[:, 0] & 1).sum()), 1)):
                                nd += 1
                                a = int(env_off[d]) + int(dom[d]["ali_i"] - dom[d]["env_i"])
                                post[(name, nd)] = (pp[a:a + int(dom[d]["ali_j"] - dom[d]["ali_i"]) + 1], int(dom[d]["env_j"] - dom[d]["env_i"]) + 1)
                                assert nd in shown, (case_name, model["h"], run, name, nd)
                    out.append((case_name, model["h"], run, theirs, ours, model["ref_mismatch"][run], post))
    finally:
        if old is None:
            del os.environ["WITCH_HIP_ALIDISPLAY"]
        else:
            os.environ["WITCH_HIP_ALIDISPLAY"] = old
    return out


def _compared(binary_runs):
    """(case, h, run, name, number, HMMER's block lines, ours, posteriors, Ld) of every domain to compare."""
    for case_name, h, run, theirs, ours, listed, post in binary_runs:
        for name, t in theirs.items():
            for d, lines in t["domains"].items():
                o = ours[name]
                if [name, d] in listed or d not in o["domains"]:
                    continue
                if _coords(o["domains"][d]) != _coords(lines):
                    continue
                yield case_name, h, run, name, d, lines, o["domains"][d], post[(name, d)]


def test_three_lines_against_the_binary(binary_runs):
    n = 0
    for case_name, h, run, name, d, his, mine, _ in _compared(binary_runs):
        assert len(his) == len(mine), (case_name, h, run, name, d)
        for a, b in zip(his[1:], mine[1:]):
            if not a.endswith(" PP"):
                assert a == b, (case_name, h, run, name, d, a, b)
        n += 1
    print("model, match and target lines (names, coordinates, blocks): HMMER's bytes on %d domains" % n)
    assert n >= 600


def test_pp_line_against_the_binary(binary_runs):
    """See the module's docstring."""
    n = n_chars = n_band = 0
    beyond = []
    for case_name, h, run, name, d, his, mine, (pp, Ld) in _compared(binary_runs):
        a = "".join(ln.split()[0] for ln in his[1:] if ln.endswith(" PP"))
        b = "".join(ln.split()[0] for ln in mine[1:] if ln.endswith(" PP"))
        assert len(a) == len(b), (case_name, h, run, name, d)
        r = 0
        for x, y in zip(a, b):
            if y == ".":
                assert x == "."
                continue
            p = float(pp[r])
            r += 1
            n_chars += 1
            if x != y:
                dist = abs((p + 0.05) * 10.0 - round((p + 0.05) * 10.0)) / 10.0
                if dist <= tol32(Ld):
                    n_band += 1
                else:
                    beyond.append((case_name, h, run, name, d, x, y, round(p, 5)))
        n += 1
    print("PP line: %d domains, %d characters, %d differ within the bound of a tenth boundary, %d differ beyond it (%d domains)" %
          (n, n_chars, n_band, len(beyond), len(set(b[:5] for b in beyond))))
    assert not beyond, beyond[:10]


# ------------------------------------------------------------------------------------------------ 4. one stage shared
def test_one_domain_stage_serves_the_three_files(tmp_path, monkeypatch):
    """--domtblout, -A and the display on one line: the same three files as the three lines alone, from ONE domain stage."""
    _need_gpu()
    from witch_amd.ehmm import EHMM
    case = load_case("amino_hmmbuild")
    hp = case.hmm_paths[0]
    fa = tmp_path / "q.fa"
    fa.write_text("".join(">%s\n%s\n" % (n, s) for n, s in zip(case.qnames, case.qseqs)))
    srv = _server()
    base = ["--max", "-E", "99999999"]
    monkeypatch.setenv("WITCH_HIP_ALIDISPLAY", "1")
    calls = []
    real = EHMM.domain_paths
    monkeypatch.setattr(EHMM, "domain_paths", lambda self, *a, **k: (calls.append("paths"), real(self, *a, **k))[1])
    for nm in ("domains", "domain_paths_t", "hits_msa", "domain_display"):
        monkeypatch.setattr(EHMM, nm, (lambda nm: lambda self, *a, **k: pytest.fail("a second domain stage: EHMM.%s" % nm))(nm))
    e, _ = srv.backend.model(hp)
    e.set_timing(True)
    srv.run_hmmsearch(base + ["-o", "all.out", "--domtblout", "all.dom", "-A", "all.sto", "--tblout", "all.tbl", hp, str(fa)], str(tmp_path))
    assert calls == ["paths"]
    ms5, n5 = e.last_kernel_ms(5)
    ms9, n9 = e.last_kernel_ms(9)
    print("one line with the display, --domtblout, -A and --tblout: domain stage %.3f ms (%d launches), display %.3f ms" % (ms5, n5, ms9))
    srv.run_hmmsearch(base + ["-o", "ali.out", hp, str(fa)], str(tmp_path))
    assert calls == ["paths"] * 2 and e.last_kernel_ms(5)[1] == n5       # the display alone: the same one stage
    e.set_timing(False)
    monkeypatch.undo()
    srv.run_hmmsearch(base + ["--noali", "-o", "d.out", "--domtblout", "one.dom", hp, str(fa)], str(tmp_path))
    srv.run_hmmsearch(base + ["--noali", "-o", "a.out", "-A", "one.sto", hp, str(fa)], str(tmp_path))
    for a, b in (("all.dom", "one.dom"), ("all.sto", "one.sto"), ("all.out", None)):
        ta = open(tmp_path / a).read()
        if b is not None:
            assert ta == open(tmp_path / b).read().replace("one.", "all."), (a, b)
    # the main output of the combined line: the display's own, with -A's line behind "//"
    strip = lambda t: [ln for ln in t.splitlines() if not ln.startswith("# Alignment of")]      # noqa: E731
    assert strip(open(tmp_path / "all.out").read()) == strip(open(tmp_path / "ali.out").read())
    assert "# Alignment of" in open(tmp_path / "all.out").read()
