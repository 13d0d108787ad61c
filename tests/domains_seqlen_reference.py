"""Reference for the domain records under the SEQUENCE's length model (wh_set_domain_length_model(WH_LENMODEL_SEQUENCE)):
hmmsearch configures the profile once for the whole sequence of L residues and keeps that configuration for every envelope,
so an envelope of Ld residues is aligned with N / C loops of L / (L + 2), not Ld / (Ld + 2).  Pure CPU, float64.

The oracle has no such argument; it does not need one.  An envelope followed by L - Ld residues of the alphabet's gap code
(match odds 0, flank odds 1) can only carry them in the C flank, where each multiplies EVERY path by the same loop
probability; that factor cancels in every posterior and in the optimal-accuracy choice, and what remains is the length
model of Ld + (L - Ld) = L residues.  So:
  columns       oracle.OracleHMM.align on the gap-padded envelope, its first Ld entries
  posteriors    tests/display_reference.envelope_posteriors(..., L) along that path
and everything that does not depend on the alignment (envelopes, bits, bias_bits, lnP) is tests/domains_reference's.
"""
import functools

import numpy as np

from tests import display_reference as disp
from tests import domains_reference as dr
from tests import pp_reference as ppr

GAP_CODE = {0: 4, 1: 4, 2: 20}          # alphabet (DNA, RNA, amino) -> digital code of '-'


def padded(sub, L, gap):
    """The envelope's residues followed by gap codes up to L residues."""
    return np.concatenate([np.asarray(sub, dtype=np.uint8), np.full(int(L) - len(sub), gap, dtype=np.uint8)])


def align_under(ohm, pmodel, sub, L):
    """(columns, float64 posteriors along them) of the residues <sub> under the unihit length model of L >= len(sub) residues:
    what wh_align_pp_len returns for a query <sub> with cfg_len = L."""
    sub = np.ascontiguousarray(sub, dtype=np.uint8)
    full = np.asarray(ohm.align(padded(sub, L, GAP_CODE[int(ohm.alphabet)])))
    assert np.all(full[len(sub):] < 0), "a gap code in a match state"
    cols = np.ascontiguousarray(full[:len(sub)])
    return cols, disp.envelope_posteriors(pmodel, sub, cols, L)


def seqlen_record(ohm, pmodel, dsq, rec):
    """<rec> (a record of domains_reference.pair_domains) re-aligned under the length model of the whole query <dsq>: a new
    dict, the alignment's fields replaced (ali_*, hmm_*, oasc, cols, pp), the others as they are."""
    ei, ej, L = int(rec["env_i"]), int(rec["env_j"]), len(dsq)
    cols, pp = align_under(ohm, pmodel, dsq[ei - 1:ej], L)
    hit = np.nonzero(cols >= 0)[0]
    out = dict(rec)
    out.update({"ali_i": ei + int(hit[0]) if len(hit) else 0, "ali_j": ei + int(hit[-1]) if len(hit) else 0,
                "hmm_i": int(cols[hit[0]]) + 1 if len(hit) else 0, "hmm_j": int(cols[hit[-1]]) + 1 if len(hit) else 0,
                "oasc": float(pp.sum()), "cols": cols, "pp": pp})
    return out


@functools.lru_cache(maxsize=None)
def reference_seqlen(name):
    """For a fixture case: (queries' residue codes, {(q, h): [domain records]}) like domains_reference.case_reference, every
    domain aligned under its sequence's length model.  Computed once per process and shared; callers do not modify it."""
    from oracle import oracle as orc
    from tests.conftest import load_case
    case = load_case(name)
    seqs, dom = dr.case_reference(name)
    H = 1 + max(h for _, h in dom)
    out = {}
    for h in range(H):
        ohm = orc.OracleHMM(case.hmm_paths[h])
        pmodel = ppr.Model(ohm)
        for q in range(len(seqs)):
            out[(q, h)] = [seqlen_record(ohm, pmodel, seqs[q], r) for r in dom[(q, h)]]
    return seqs, out


def changed_domains(name):
    """[(q, h, index)] of the case's domains whose path under the sequence's length model is not the envelope model's."""
    _, env = dr.case_reference(name)
    _, seq = reference_seqlen(name)
    return [(q, h, int(a["index"])) for (q, h) in sorted(env) for a, b in zip(env[(q, h)], seq[(q, h)]) if not np.array_equal(a["cols"], b["cols"])]
