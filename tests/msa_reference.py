"""Plain numpy assembly of hmmalign's multi-sequence alignment: the reference of wh_msa (tests/test_msa_host.py checks it
against the bundled binary's own rows, tests/test_msa_gpu.py checks the kernels against it), and the readers of the
fixtures under tests/golden/msa (tests/golden/make_golden_msa.py).

Layout rules: every node is a column; block k (0..M) between nodes k and k + 1 is as wide as the longest insert run any
sequence has there; N-flank residues (block 0) right-justified, C-flank residues (block M) left-justified, an internal run
of n residues: the first n // 2 flush left, the rest flush right; trim drops both flanks.  PP_cons: on a match column the
character of the float32 mean (sum in sequence order) of the posteriors of the sequences with a residue there."""
import functools
import gzip
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["dna_synth", "dna_planted", "amino", "dna_65", "sub30_two"]
CHARS = "0123456789*"


@functools.lru_cache(maxsize=None)
def load_fixture(name):
    with gzip.open(os.path.join(GOLDEN, "msa", name + ".json.gz"), "rt") as f:
        fx = json.load(f)
    fx["hmm_path"] = os.path.join(GOLDEN, fx["hmm"])
    return fx


def parse_msa(text):
    """hmmalign's Stockholm or Pfam text -> (rows {name: row}, pp_rows {name: row}, PP_cons, RF or None)."""
    rows, pps, cons, rf = {}, {}, "", ""
    for line in text.splitlines():
        if line.startswith("#=GR"):
            w = line.split()
            pps[w[1]] = pps.get(w[1], "") + w[3]
        elif line.startswith("#=GC PP_cons"):
            cons += line.split()[2]
        elif line.startswith("#=GC RF"):
            rf += line.split()[2]
        elif line.strip() and not line.startswith(("#", "//")):
            n, s = line.split()
            rows[n] = rows.get(n, "") + s
    return rows, pps, cons, rf or None


def decode_row(row, pp, rf):
    """Per residue of a row: the 0-based node (or -1) by the RF line, and its PP character."""
    cols, digits, k = [], [], -1
    for c, p, r in zip(row, pp, rf):
        if r == "x":
            k += 1
        if c not in "-.":
            cols.append(k if r == "x" else -1)
            digits.append(p)
    return np.array(cols, dtype=np.int32), "".join(digits)


def char_interval(ch):
    """[lo, hi] of the posteriors hmmalign prints as <ch>."""
    if ch == "*":
        return 0.95, 1.0
    d = CHARS.index(ch)
    return max(0.0, d / 10.0 - 0.05), d / 10.0 + 0.05


def midpoints(digits):
    """float32 posteriors in the middle of each character's interval (each encodes back to its character)."""
    return np.array([sum(char_interval(c)) / 2.0 for c in digits], dtype=np.float32)


def pp_char(p):
    """formats.pp_char, restated: float64 arithmetic on the (float32) value."""
    v = float(p) + 0.05
    return "*" if v >= 1.0 else CHARS[min(9, max(0, int(v * 10.0)))]


def assemble(M, cols, pps, texts, trim=False):
    """cols / pps / texts: per sequence its per-residue nodes (int, -1: none), posteriors (float32) and characters.
    Returns {"W", "rows", "pp_rows" (uint8 [nq, W]), "pp_cons", "rf" (uint8 [W]), "matmap" (int32 [M]), "pathless"}."""
    nq = len(cols)
    width = np.zeros(M + 1, dtype=np.int64)
    cells = []                                   # per sequence: [(residue, block, k)], k < 0: from the block's right end
    pathless = 0
    for c in cols:
        c = np.asarray(c, dtype=np.int64)
        L, out, r = len(c), [], 0
        match = (c >= 0) & (c < M)
        while r < L:
            if match[r]:
                r += 1
                continue
            e = r
            while e < L and not match[e]:
                e += 1
            n, nfl, cfl = e - r, r == 0, e == L
            if nfl and cfl:
                blk = -1
                pathless += 1
            elif nfl:
                blk = -1 if trim else 0
            elif cfl:
                blk = -1 if trim else M
            else:
                blk = int(c[r - 1]) + 1
            if blk >= 0:
                width[blk] = max(width[blk], n)
                for i in range(n):
                    out.append((r + i, blk, i - n if nfl else i if cfl else i if i < n // 2 else i - n))
            r = e
        cells.append(out)
    first = np.zeros(M + 2, dtype=np.int64)
    first[1:] = np.cumsum(width) + np.arange(1, M + 2)
    first[M + 1] -= 1                            # (no column behind block M)
    W = int(first[M + 1])
    matmap = (first[:M] + width[:M]).astype(np.int32)
    rf = np.full(W, ord("."), dtype=np.uint8)
    rf[matmap] = ord("x")
    rows = np.empty((nq, W), dtype=np.uint8)
    rows[:] = np.where(rf == ord("x"), ord("-"), ord("."))[None, :]
    pp_rows = np.full((nq, W), ord("."), dtype=np.uint8)
    s = np.zeros(M, dtype=np.float32)
    cnt = np.zeros(M, dtype=np.int64)
    for q in range(nq):
        c = np.asarray(cols[q], dtype=np.int64)
        p = np.asarray(pps[q], dtype=np.float32)
        t = texts[q]
        for r in range(len(c)):
            if 0 <= c[r] < M:
                at = matmap[c[r]]
                rows[q, at] = ord(t[r].upper())
                pp_rows[q, at] = ord(pp_char(p[r]))
                s[c[r]] = np.float32(s[c[r]] + p[r])            # float32, in sequence order
                cnt[c[r]] += 1
        for r, blk, k in cells[q]:
            at = first[blk] + (k if k >= 0 else width[blk] + k)
            rows[q, at] = ord(t[r].lower())
            pp_rows[q, at] = ord(pp_char(p[r]))
    pp_cons = np.full(W, ord("."), dtype=np.uint8)
    for k in range(M):
        if cnt[k]:
            pp_cons[matmap[k]] = ord(pp_char(np.float32(s[k]) / np.float32(cnt[k])))
    return {"W": W, "rows": rows, "pp_rows": pp_rows, "pp_cons": pp_cons, "rf": rf, "matmap": matmap, "pathless": pathless}


def cons_interval(M, cols, digits):
    """Per node the characters between which the binary's PP_cons character must lie, given only the PP CHARACTERS of the
    sequences: every posterior lies in its character's interval, so the mean lies between the means of the interval ends.
    Returns (lo, hi) lists of characters, '.' where no sequence has a residue."""
    lo, hi, cnt = np.zeros(M), np.zeros(M), np.zeros(M, dtype=np.int64)
    for c, d in zip(cols, digits):
        for r, k in enumerate(c):
            if 0 <= k < M:
                a, b = char_interval(d[r])
                lo[k] += a
                hi[k] += b
                cnt[k] += 1
    # (1e-6: the binary's own float32 sums)
    return ([pp_char(max(0.0, lo[k] / cnt[k] - 1e-6)) if cnt[k] else "." for k in range(M)],
            [pp_char(min(1.0, hi[k] / cnt[k] + 1e-6)) if cnt[k] else "." for k in range(M)])


@functools.lru_cache(maxsize=None)
def fixture_inputs(name):
    """A fixture decoded once: (M, names, texts, cols, digits, parsed default output).  Callers do not modify it."""
    fx = load_fixture(name)
    rows, pps, cons, rf = parse_msa(fx["out"]["sto"])
    M = rf.count("x")
    cols, digits = [], []
    for n in fx["names"]:
        c, d = decode_row(rows[n], pps[n], rf)
        cols.append(c)
        digits.append(d)
    return M, fx["names"], fx["seqs"], cols, digits, (rows, pps, cons, rf)


def matrix(rows, names):
    """{name: row} -> uint8 [nq, W]."""
    return np.array([np.frombuffer(rows[n].encode(), dtype=np.uint8) for n in names], dtype=np.uint8).reshape(len(names), -1)
