#!/usr/bin/env python3
"""hmmalign --mapali: the alignment a model was built from as rows of the output, followed by the new sequences, for
wh_msa_mapali (tests/test_mapali_host.py, tests/test_mapali_gpu.py, tests/mapali_reference.py).

RUNS ONLY IN THE BUILD CONTAINER (needs /root/reference): the reference's bundled `hmmbuild` (where a case needs a new model)
and `hmmalign --mapali ALN [options] HMM FASTA`, four calls per case - default Stockholm, --trim, --outformat Pfam,
--outformat afa.  Stored under tests/golden/mapali/<case>.json.gz: {"parts": [{"aln": the alignment file's text,
"aln_format": "afa" | "stockholm", "hmm": model file below tests/golden or null, "hmm_text": the model's text where it is new,
"names", "seqs": the new sequences, "out": {"sto", "trim", "pfam", "afa"}}]}; the `mismatch` case holds {"status", "stderr"}
in place of "out".  Cases:
  planted      the 7 x 34 probe of DESIGN.md section 4.12 (an insert behind a deleted node, an insert before a row's first
               match residue, blocks 0 and M populated by the alignment only, a row of inserts only ...) with three new
               sequences, and its sibling without r6 with two
  planted_sto  the probe as Stockholm: '.' gaps, upper case, a "#=GS r0 DE" line, interleaved in blocks of 20 columns
  edges        hmmbuild_cases/dna_fragment_edges (50 columns, 48 nodes) with 3 new sequences
  amino        hmmbuild_cases/amino_mixed with 3 protein sequences
  rows65       the afa output of msa/dna_65 (65 rows, more than 128 columns, real insert columns) as a NEW alignment, its model
               by the bundled hmmbuild's defaults, 5 new sequences
  one_new      the probe with the single new sequence n1
  mismatch     the probe with one residue altered: status 1 and the message
The maker prints, per case, the share of the new sequences' PP characters inside the float32 guard band of
tests/test_msa_gpu.py (computed with the CPU oracle's posteriors); the cap is 1 %.
"""
import gzip
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import msa_reference as mr  # noqa: E402

TOOLS = "/root/reference/witch_msa/tools/magus/tools/hmmer/"
OUT = os.path.join(HERE, "mapali")
OPTIONS = {"sto": [], "trim": ["--trim"], "pfam": ["--outformat", "Pfam"], "afa": ["--outformat", "afa"]}

PROBE = [("r0", "gt-ACGTAC--GTTGCA---ACGTGCATGCAAcg"), ("r1", "---ACGTACa-GTTGCA---ACGTGCATGCAA--"),
         ("r2", "-c-ACGTACagGTTGCAt--ACGTGCATGCAAc-"), ("r3", "----------gGTTGC-tct-CGTGCATG-----"),
         ("r4", "---ACGTAC--GTTGCA---ACGTGCATGCAA--"), ("r5", "a--ACG--Cg-GTTGCA--cACGTGCATGC---t"),
         ("r6", "---ACGTACag------tc---------------")]
SIBLING = [r for r in PROBE if r[0] != "r6"]
SIBLING[3] = ("r3", "---ACG-ACagGTTGC-tct-CGTGCATGCAA--")
N1 = ("n1", "GTACGTTGCAACGTG")


def afa(records):
    return "".join(">%s\n%s\n" % r for r in records)


def stockholm(records, block=20):
    out = ["# STOCKHOLM 1.0", "", "#=GS r0 DE the first row of the probe", ""]
    alen = len(records[0][1])
    for a in range(0, alen, block):
        for n, s in records:
            out.append("%-4s %s" % (n, s[a:a + block].upper().replace("-", ".")))
        out.append("")
    out.append("//")
    return "\n".join(out) + "\n"


def write(tmp, name, text):
    p = os.path.join(tmp, name)
    with open(p, "w") as f:
        f.write(text)
    return p


def hmmbuild(tmp, molecule, name, aln_path):
    hmm = os.path.join(tmp, name + ".hmm")
    subprocess.run([TOOLS + "hmmbuild", "--" + molecule, "-n", name, "-o", "/dev/null", hmm, aln_path], check=True)
    with open(hmm) as f:
        return f.read()


def part(tmp, aln_text, aln_format, hmm_rel, hmm_text, records, run=True):
    aln = write(tmp, "aln." + ("sto" if aln_format == "stockholm" else "afa"), aln_text)
    hmm = os.path.join(HERE, hmm_rel) if hmm_rel else write(tmp, "model_%d.hmm" % len(os.listdir(tmp)), hmm_text)
    fa = write(tmp, "new.fa", afa(records))
    p = {"aln": aln_text, "aln_format": aln_format, "hmm": hmm_rel, "hmm_text": None if hmm_rel else hmm_text,
         "names": [n for n, _ in records], "seqs": [s for _, s in records]}
    if run:
        p["out"] = {k: subprocess.run([TOOLS + "hmmalign", "--mapali", aln] + v + [hmm, fa], check=True, stdout=subprocess.PIPE,
                                      text=True).stdout for k, v in OPTIONS.items()}
    else:
        r = subprocess.run([TOOLS + "hmmalign", "--mapali", aln, hmm, fa], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        p["status"], p["stderr"], p["stdout"] = r.returncode, r.stderr.replace(aln, "ALN"), r.stdout.replace(aln, "ALN")
    return p, hmm


def band_share(p, hmm):
    """(characters of the new sequences' PP lines and of PP_cons at the nodes they touch, those inside the guard band), by
    the CPU oracle's posteriors: the count tests/test_mapali_gpu.py caps at 1 %."""
    from oracle import oracle as orc
    from tests import pp_reference as ppr
    from tests.test_align_pp import BOUNDS, tol32
    rows, pps, cons, rf = mr.parse_msa(p["out"]["sto"])
    ohm = orc.OracleHMM(hmm)
    model = ppr.Model(ohm)
    M = rf.count("x")
    n_chars = n_band = 0
    ref_sum, ref_n, ref_tol = np.zeros(M), np.zeros(M, dtype=np.int64), np.zeros(M)
    for n, s in zip(p["names"], p["seqs"]):
        cols, digits = mr.decode_row(rows[n], pps[n], rf)
        ref = ppr.path_posteriors(model, ohm.digitize(s.upper()), cols)
        n_chars += len(ref)
        n_band += int((np.min(np.abs(ref[:, None] - BOUNDS[None, :]), axis=1) <= tol32(len(ref))).sum())
        m = cols >= 0
        np.add.at(ref_sum, cols[m], ref[m])
        np.add.at(ref_n, cols[m], 1)
        np.maximum.at(ref_tol, cols[m], tol32(len(ref)))
    for k in np.nonzero(ref_n)[0]:
        n_chars += 1
        n_band += int(np.min(np.abs(ref_sum[k] / ref_n[k] - BOUNDS)) <= ref_tol[k])
    return n_chars, n_band


def dump(name, parts_hmms):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps({"parts": [p for p, _ in parts_hmms]}, separators=(",", ":")).encode())
    n_chars = n_band = 0
    for p, hmm in parts_hmms:
        if "out" in p:
            a, b = band_share(p, hmm)
            n_chars, n_band = n_chars + a, n_band + b
    print("%s: %d bytes; %d PP and PP_cons characters of new sequences, %d in the guard band (%.2f %%)" %
          (name, os.path.getsize(path), n_chars, n_band, 100.0 * n_band / max(n_chars, 1)))


def mutate(rng, s, alphabet, n):
    s = list(s)
    for at in rng.choice(len(s), size=min(n, len(s)), replace=False):
        s[at] = alphabet[rng.integers(0, len(alphabet))]
    return "".join(s)


def ungapped(row):
    return "".join(c for c in row if c not in "-._~").upper()


def read_afa(path_or_text, is_text=False):
    text = path_or_text if is_text else open(path_or_text).read()
    out = []
    for line in text.splitlines():
        if line.startswith(">"):
            out.append([line[1:].split()[0], ""])
        elif out:
            out[-1][1] += line.strip()
    return [tuple(r) for r in out]


# per case: the seed of its mutations, the first (from 1) that leaves no more than 1 % of the case's PP and PP_cons characters
# in the guard band
SEEDS = {"edges": 3, "amino": 1, "rows65": 9}


def random_cases(tmp, seeds):
    """{case: [(part, model file)]} of the cases whose new sequences are mutated copies of the alignment's rows."""
    out = {}
    rng = np.random.default_rng(seeds["edges"])
    rnd = lambda n: "".join("ACGT"[i] for i in rng.integers(0, 4, size=n))      # noqa: E731
    rel = "hmmbuild_cases/dna_fragment_edges"
    rows = read_afa(os.path.join(HERE, rel + ".afa"))
    s0 = ungapped(rows[0][1])
    out["edges"] = [part(tmp, afa(rows), "afa", rel + ".hmm", None,
                         [("e0", mutate(rng, s0, "ACGT", 3)), ("e1", rnd(2) + mutate(rng, s0[5:30], "ACGT", 2)), ("e2", s0[:20] + rnd(3) + s0[20:] + rnd(2))])]
    rng = np.random.default_rng(seeds["amino"])
    rel = "hmmbuild_cases/amino_mixed"
    rows = read_afa(os.path.join(HERE, rel + ".afa"))
    aa = "ACDEFGHIKLMNPQRSTVWY"
    s1, s2 = ungapped(rows[1][1]).replace("B", "D"), ungapped(rows[2][1]).replace("Z", "E")
    out["amino"] = [part(tmp, afa(rows), "afa", rel + ".hmm", None,
                         [("p0", mutate(rng, s1, aa, 4)), ("p1", mutate(rng, s2[8:40], aa, 2)), ("p2", s1[:25] + "GS" + s1[25:])])]
    rng = np.random.default_rng(seeds["rows65"])
    rows = read_afa(mr.load_fixture("dna_65")["out"]["afa"], is_text=True)
    text = afa(rows)
    hmm65 = hmmbuild(tmp, "dna", "rows65", write(tmp, "rows65.afa", text))
    src = [ungapped(rows[t][1]) for t in (0, 3, 11, 20, 47)]
    new5 = [("x0", mutate(rng, src[0], "ACGT", 5)), ("x1", src[1][10:]), ("x2", rnd(4) + src[2]), ("x3", src[3][:60] + rnd(6) + src[3][60:]),
            ("x4", mutate(rng, src[4][5:-5], "ACGT", 3))]
    out["rows65"] = [part(tmp, text, "afa", None, hmm65, new5)]
    return out


def main():
    tmp = tempfile.mkdtemp(prefix="golden_mapali_")
    probe_hmm = hmmbuild(tmp, "dna", "probe", write(tmp, "probe.afa", afa(PROBE)))
    sib_hmm = hmmbuild(tmp, "dna", "sibling", write(tmp, "sibling.afa", afa(SIBLING)))
    new3 = [N1, ("n2", "ttACGTACAGGTTGCATCACGTGCATGCAAcgg"), ("n3", "ACGTACGTTGCAACGTGCATGC")]
    dump("planted", [part(tmp, afa(PROBE), "afa", None, probe_hmm, new3),
                     part(tmp, afa(SIBLING), "afa", None, sib_hmm, [N1, ("n2", "ACGACAGGTTGCATCTCGTGCATGCAAG")])])
    dump("planted_sto", [part(tmp, stockholm(PROBE), "stockholm", None, probe_hmm, new3)])
    dump("one_new", [part(tmp, afa(PROBE), "afa", None, probe_hmm, [N1])])
    bad = [list(r) for r in PROBE]
    bad[1][1] = bad[1][1][:12] + "C" + bad[1][1][13:]           # r1: GTTGCA -> GCTGCA
    dump("mismatch", [part(tmp, afa([tuple(r) for r in bad]), "afa", None, probe_hmm, [N1], run=False)])
    for name, parts in random_cases(tmp, SEEDS).items():
        dump(name, parts)


if __name__ == "__main__":
    main()
