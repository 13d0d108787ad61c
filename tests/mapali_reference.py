"""Plain numpy restatement of hmmalign --mapali: the reference of wh_msa_mapali (tests/test_mapali_host.py checks it against
the bundled binary's outputs, tests/test_mapali_gpu.py checks the kernels against it), and the readers of the fixtures under
tests/golden/mapali (tests/golden/make_golden_mapali.py).

Rules: the rows of the alignment the model was built from come first.  A residue of such a row goes
by its alignment column: the column MAP gives node k is node k's (upper case); a column between those of nodes k and k + 1 is
an insert of block k (lower case; block 0 before node 1's column, block M behind node M's), whatever the row has or lacks in
the node columns around it.  All the residues a row has in one block form one run, laid out by the rule of the new
sequences' runs (block 0 right-justified, block M left-justified, else the first n // 2 flush left and the rest flush
right); widths are the maximum over rows and new sequences; trim drops blocks 0 and M of the rows too.  A row of the
alignment has no PP row and no part in PP_cons."""
import functools
import gzip
import json
import os

import numpy as np

from tests.msa_reference import GOLDEN, pp_char

CASES = ["planted", "planted_sto", "edges", "amino", "rows65", "one_new"]


@functools.lru_cache(maxsize=None)
def load_fixture(name):
    """The parts of a fixture; callers do not modify them."""
    with gzip.open(os.path.join(GOLDEN, "mapali", name + ".json.gz"), "rt") as f:
        return json.load(f)["parts"]


def all_parts():
    return [(name, i) for name in CASES for i in range(len(load_fixture(name)))]


def hmm_file(part, tmpdir):
    """The part's model as a file: the committed one, or its text written below tmpdir."""
    if part["hmm"]:
        return os.path.join(GOLDEN, part["hmm"])
    path = os.path.join(str(tmpdir), "model_%08x.hmm" % (hash(part["hmm_text"]) & 0xFFFFFFFF))
    if not os.path.exists(path):
        with open(path, "w") as f:
            f.write(part["hmm_text"])
    return path


def hmm_text(part):
    if part["hmm"]:
        with open(os.path.join(GOLDEN, part["hmm"])) as f:
            return f.read()
    return part["hmm_text"]


def model_header(text):
    """(M, alphabet, CKSUM or None, MAP columns int [M], 1-based) of a HMMER3/f text."""
    M, alph, cksum, cols, body = 0, "", None, [], False
    lines = text.splitlines()
    for i, line in enumerate(lines):
        w = line.split()
        if not w:
            continue
        if not body:
            if w[0] == "LENG":
                M = int(w[1])
            elif w[0] == "ALPH":
                alph = w[1].lower()
            elif w[0] == "CKSUM":
                cksum = int(w[1])
            elif w[0] == "HMM":
                body = True
                K = len(w) - 1
        elif w[0].isdigit() and len(w) >= K + 2 and int(w[0]) == len(cols) + 1:
            cols.append(int(w[K + 1]))
    assert len(cols) == M
    return M, alph, cksum, np.array(cols, dtype=np.int64)


def parse_alignment(text):
    """An aligned-FASTA or Stockholm text -> (names, rows, {name: "#=GS DE" text})."""
    names, rows, desc = [], {}, {}
    sto = text.lstrip().startswith("# STOCKHOLM")
    cur = None
    for line in text.splitlines():
        if sto:
            if line.startswith("#=GS"):
                w = line.split(None, 3)
                if w[2] == "DE":
                    desc[w[1]] = w[3]
            elif line.strip() and not line.startswith(("#", "//")):
                n, t = line.split()
                if n not in rows:
                    names.append(n)
                    rows[n] = ""
                rows[n] += t
        elif line.startswith(">"):
            cur = line[1:].split()[0]
            names.append(cur)
            rows[cur] = ""
        elif cur is not None:
            rows[cur] += line.strip()
    return names, [rows[n] for n in names], desc


def checksum(rows, alph):
    """hmmbuild's CKSUM: Jenkins' one-at-a-time hash over Easel's digital codes, gaps included."""
    syms = "ACDEFGHIKLMNPQRSTVWY-BJZOUX*~" if alph == "amino" else "ACGT-RYMKSWHBVDN*~"
    code = {c: i for i, c in enumerate(syms)}
    code.update({"_": code["-"], ".": code["-"]})
    if alph != "amino":
        code.update({"U": code["T"], "X": code["N"], "I": code["A"]})
    h = 0
    for r in rows:
        for ch in r.upper():
            h = (h + code[ch]) & 0xFFFFFFFF
            h = (h + (h << 10)) & 0xFFFFFFFF
            h ^= h >> 6
    h = (h + (h << 3)) & 0xFFFFFFFF
    h ^= h >> 11
    return (h + (h << 15)) & 0xFFFFFFFF


def colcode(map_cols, alen):
    """Per alignment column: node - 1, or -(k + 2) for an insert column of block k."""
    code = np.empty(alen, dtype=np.int32)
    k = 0
    for c in range(alen):
        if k < len(map_cols) and map_cols[k] == c + 1:
            code[c] = k
            k += 1
        else:
            code[c] = -(k + 2)
    return code


def row_sequences(rows, code):
    """The rows compacted to their residues (letters): per row (codes int32, characters)."""
    cols, texts = [], []
    for r in rows:
        keep = [i for i, ch in enumerate(r) if ch.isalpha()]
        cols.append(code[keep].astype(np.int32) if keep else np.zeros(0, dtype=np.int32))
        texts.append("".join(r[i] for i in keep))
    return cols, texts


def assemble(M, cols, pps, texts, n_nopp=0, trim=False):
    """tests/msa_reference.assemble with the explicit block codes -(k + 2) and <n_nopp> leading sequences without posteriors
    (pps[q] is ignored for them).  rows uint8 [nq, W]; pp_rows uint8 [nq - n_nopp, W]; pathless counts the others only."""
    nq = len(cols)
    width = np.zeros(M + 1, dtype=np.int64)
    cells, pathless = [], 0
    for q, c in enumerate(cols):
        c = np.asarray(c, dtype=np.int64)
        L, out, r = len(c), [], 0
        match = (c >= 0) & (c < M)
        named = (c <= -2) & (c >= -(M + 2))
        while r < L:
            if match[r]:
                r += 1
                continue
            e = r + 1
            if named[r]:
                while e < L and c[e] == c[r]:
                    e += 1
                blk = int(-(c[r] + 2))
                nfl, cfl = blk == 0, blk == M
                if trim and (nfl or cfl):
                    blk = -1
            else:
                while e < L and not match[e] and not named[e]:
                    e += 1
                nfl, cfl = r == 0, e == L
                if nfl and cfl:
                    blk = -1
                    pathless += q >= n_nopp
                elif nfl:
                    blk = -1 if trim else 0
                elif cfl:
                    blk = -1 if trim else M
                else:
                    blk = int(c[r - 1]) + 1 if match[r - 1] else int(-(c[r - 1] + 2))
            n = e - r
            if blk >= 0:
                width[blk] = max(width[blk], n)
                for i in range(n):
                    out.append((r + i, blk, i - n if nfl else i if cfl else i if i < n // 2 else i - n))
            r = e
        cells.append(out)
    first = np.zeros(M + 2, dtype=np.int64)
    first[1:] = np.cumsum(width) + np.arange(1, M + 2)
    first[M + 1] -= 1
    W = int(first[M + 1])
    matmap = (first[:M] + width[:M]).astype(np.int32)
    rf = np.full(W, ord("."), dtype=np.uint8)
    rf[matmap] = ord("x")
    rows = np.empty((nq, W), dtype=np.uint8)
    rows[:] = np.where(rf == ord("x"), ord("-"), ord("."))[None, :]
    pp_rows = np.full((nq - n_nopp, W), ord("."), dtype=np.uint8)
    s = np.zeros(M, dtype=np.float32)
    cnt = np.zeros(M, dtype=np.int64)
    for q in range(nq):
        c = np.asarray(cols[q], dtype=np.int64)
        t = texts[q]
        p = np.asarray(pps[q], dtype=np.float32) if q >= n_nopp else None
        for r in range(len(c)):
            if 0 <= c[r] < M:
                at = matmap[c[r]]
                rows[q, at] = ord(t[r].upper())
                if p is not None:
                    pp_rows[q - n_nopp, at] = ord(pp_char(p[r]))
                    s[c[r]] = np.float32(s[c[r]] + p[r])
                    cnt[c[r]] += 1
        for r, blk, k in cells[q]:
            at = first[blk] + (k if k >= 0 else width[blk] + k)
            rows[q, at] = ord(t[r].lower())
            if p is not None:
                pp_rows[q - n_nopp, at] = ord(pp_char(p[r]))
    pp_cons = np.full(W, ord("."), dtype=np.uint8)
    for k in range(M):
        if cnt[k]:
            pp_cons[matmap[k]] = ord(pp_char(np.float32(s[k]) / np.float32(cnt[k])))
    return {"W": W, "rows": rows, "pp_rows": pp_rows, "pp_cons": pp_cons, "rf": rf, "matmap": matmap, "pathless": int(pathless)}


@functools.lru_cache(maxsize=None)
def part_inputs(name, i):
    """A part decoded once: dict with M, alph, cksum, map (MAP columns), names / rows / desc of the alignment, code (colcode),
    map_cols / map_texts (the rows as sequences), and, from the binary's default output, the new sequences' cols / digits and
    the parsed output (rows, pps, cons, rf)."""
    from tests import msa_reference as mr
    p = load_fixture(name)[i]
    M, alph, cksum, mapc = model_header(hmm_text(p))
    names, rows, desc = parse_alignment(p["aln"])
    code = colcode(mapc, len(rows[0]))
    mcols, mtexts = row_sequences(rows, code)
    out = {"M": M, "alph": alph, "cksum": cksum, "map": mapc, "names": names, "rows": rows, "desc": desc, "code": code,
           "map_cols": mcols, "map_texts": mtexts}
    if "out" in p:
        parsed = mr.parse_msa(p["out"]["sto"])
        cols, digits = [], []
        for n in p["names"]:
            c, d = mr.decode_row(parsed[0][n], parsed[1][n], parsed[3])
            cols.append(c)
            digits.append(d)
        out.update({"cols": cols, "digits": digits, "parsed": parsed})
    return out


def synthetic_alignment(n_map, alen, seed=0):
    """A DNA alignment for the shape tests: two columns in three dense (match columns under symfrac 0.5), every third sparse
    (insert columns), the first and the last column sparse when there are five or more (blocks 0 and M hold residues of
    the alignment only); with three rows or more, row 0 has no residue, row 1 no gap, row 2 residues in sparse columns only."""
    rng = np.random.default_rng(1000 * n_map + alen + seed)
    sparse = np.array([c % 3 == 2 for c in range(alen)])
    if alen >= 5:
        sparse[0] = sparse[-1] = True
    rows = []
    for i in range(n_map):
        keep = np.where(sparse, rng.random(alen) < 0.15, rng.random(alen) < 0.9)
        if n_map >= 3 and i == 0:
            keep[:] = False
        elif i == 1 or n_map == 1:
            keep[:] = True
        elif i == 2:
            keep = sparse.copy()
        rows.append("".join("ACGT"[rng.integers(0, 4)] if k else "-" for k in keep))
    return ["m%d" % i for i in range(n_map)], rows
