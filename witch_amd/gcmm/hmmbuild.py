"""eHMM construction: the reference's `subset_alignment_and_hmmbuild`
(witch_msa/gcmm/algorithm.py:394-477) without the hmmbuild process - the model comes from wh_hmmbuild in
libwitch_hip.so (witch_amd/csrc/wh_build.cpp, host code; HMMER 3.1b2's algorithm for the reference's exact
command line `hmmbuild --cpu 1 --<molecule> --ere 0.59 --symfrac 0.0 --informat afa`).

The returned tuples are the reference's: the retained (not all-gap) backbone columns of the subset and the
non-gap count of every backbone column (algorithm.py:423-429, 476-477).
"""
import ctypes as C
import os

import numpy as np

from .._lib import lib, check

_MOLECULES = {"dna": b"dna", "rna": b"rna", "amino": b"amino"}


def hmmbuild_text(rows, molecule="dna", name="sub", ere=0.59, symfrac=0.0, fragthresh=0.5, stats=False):
    """rows: aligned sequences (str or bytes, equal length).  Returns (HMMER3/f text, M, Neff).
    stats=True adds hmmbuild's three STATS LOCAL lines (E-value calibration; include/witch_hip.h: WH_BUILD_STATS):
    only stock HMMER needs them, this path never reads them."""
    if molecule not in _MOLECULES:
        raise ValueError("molecule must be dna, rna or amino")
    rows = [r.encode("ascii") if isinstance(r, str) else bytes(r) for r in rows]
    if not rows:
        raise ValueError("empty alignment")
    alen = len(rows[0])
    if any(len(r) != alen for r in rows):
        raise ValueError("rows of an alignment must have equal length")
    arr = (C.c_char_p * len(rows))(*rows)
    text, n, M, neff = C.c_void_p(), C.c_int64(0), C.c_int32(0), C.c_double(0.0)
    check(lib().wh_hmmbuild2(_MOLECULES[molecule], len(rows), alen, arr, name.encode(), ere, symfrac, fragthresh,
                             1 if stats else 0, C.byref(text), C.byref(n), C.byref(M), C.byref(neff)), "wh_hmmbuild")
    try:
        out = C.string_at(text.value, n.value).decode("ascii")
    finally:
        lib().wh_free_text(text)
    return out, int(M.value), float(neff.value)


def default_calibration_device():
    """The HIP device a batch is calibrated on when the caller names none: the current one if the library can see a
    device, else -1 (the host)."""
    try:
        import torch
        if torch.cuda.is_available():
            return int(torch.cuda.current_device())
    except Exception:
        pass
    return -1


def hmmbuild_text_batch(list_of_rows, molecule="dna", names=None, ere=0.59, symfrac=0.0, fragthresh=0.5, stats=False,
                        device=None, want_stats_values=False, flags=0):
    """All models of an eHMM in one call (include/witch_hip.h: wh_hmmbuild_batch).  list_of_rows: one aligned row list per
    model.  Returns a list of (HMMER3/f text, M, Neff) - with want_stats_values (lambda, MSV mu, Viterbi mu, Forward tau)
    as a fourth entry.  Every text is what hmmbuild_text returns for the same rows.  stats=True calibrates the whole
    batch at once, on HIP device `device` (None: the current device if there is one, else the host; -1: the host).
    flags: further WH_BUILD_* bits (test hooks)."""
    if molecule not in _MOLECULES:
        raise ValueError("molecule must be dna, rna or amino")
    n = len(list_of_rows)
    if names is None:
        names = ["sub"] * n
    if len(names) != n:
        raise ValueError("one name per model")
    if device is None:
        device = default_calibration_device() if stats else -1
    enc = []
    for rows in list_of_rows:
        rows = [r.encode("ascii") if isinstance(r, str) else bytes(r) for r in rows]
        if not rows:
            raise ValueError("empty alignment")
        if any(len(r) != len(rows[0]) for r in rows):
            raise ValueError("rows of an alignment must have equal length")
        enc.append(rows)
    row_arrs = [(C.c_char_p * len(rows))(*rows) for rows in enc]
    rows_pp = (C.POINTER(C.c_char_p) * max(n, 1))(*[C.cast(a, C.POINTER(C.c_char_p)) for a in row_arrs])
    nseq = (C.c_int32 * max(n, 1))(*[len(rows) for rows in enc])
    alen = (C.c_int64 * max(n, 1))(*[len(rows[0]) for rows in enc])
    name_arr = (C.c_char_p * max(n, 1))(*[nm.encode() for nm in names])
    text = (C.c_void_p * max(n, 1))()
    tlen = (C.c_int64 * max(n, 1))()
    M = (C.c_int32 * max(n, 1))()
    neff = (C.c_double * max(n, 1))()
    sv = (C.c_double * (4 * max(n, 1)))()
    check(lib().wh_hmmbuild_batch(int(device), _MOLECULES[molecule], n, nseq, alen, rows_pp, name_arr, ere, symfrac, fragthresh,
                                  (1 if stats else 0) | int(flags), text, tlen, M, neff, sv), "wh_hmmbuild_batch")
    out = []
    try:
        for i in range(n):
            t = C.string_at(text[i], tlen[i]).decode("ascii")
            out.append((t, int(M[i]), float(neff[i])) + ((tuple(sv[4 * i:4 * i + 4]),) if want_stats_values else ()))
    finally:
        for i in range(n):
            lib().wh_free_text(text[i])
    return out


def _reduce_subset(names, rows, outdirprefix, label):
    """The reference's reduction of one subset (algorithm.py:423-429): all-gap columns deleted, the reduced alignment
    written to <outdirprefix>/<label>/hmmbuild.input.<label>.fasta.  Returns (directory, reduced rows, retained
    columns, non-gap counts)."""
    d = os.path.join(outdirprefix, label)
    os.makedirs(d, exist_ok=True)
    ax = np.stack([np.frombuffer((r.upper().encode("ascii") if isinstance(r, str) else bytes(r).upper()), dtype=np.uint8)
                   for r in rows])
    nongap = ax != ord("-")
    keep = np.nonzero(nongap.any(axis=0))[0]
    retained_columns = tuple(int(x) for x in keep)
    nongaps_per_column = tuple(int(x) for x in nongap[:, keep].sum(axis=0))
    reduced = [r.tobytes() for r in ax[:, keep]]
    with open(os.path.join(d, "hmmbuild.input.%s.fasta" % label), "w") as f:
        for n, r in zip(names, reduced):
            f.write(">%s\n%s\n" % (n, r.decode("ascii")))
    return d, reduced, retained_columns, nongaps_per_column


def subset_alignment_and_hmmbuild(names, rows, molecule, outdirprefix, label, ere=0.59, symfrac=0.0):
    """The reference's per-subset step (algorithm.py:394-477) for the backbone rows of ONE subset (names, rows:
    the subset's taxa and their backbone rows; the reference upper-cases sequences when it reads the backbone):
    all-gap columns are deleted first, the reduced alignment is written to
    <outdirprefix>/<label>/hmmbuild.input.<label>.fasta, the model built from it to
    <outdirprefix>/<label>/hmmbuild.model.<label>.  Returns the reference's tuple
    (model_path, label, retained_columns, nongaps_per_column): the backbone columns that survive, and the
    non-gap count of every surviving column."""
    d, reduced, retained_columns, nongaps_per_column = _reduce_subset(names, rows, outdirprefix, label)
    text, _, _ = hmmbuild_text(reduced, molecule, "hmmbuild.input.%s" % label, ere=ere, symfrac=symfrac)
    path = os.path.join(d, "hmmbuild.model.%s" % label)
    with open(path, "w") as f:
        f.write(text)
    return path, label, retained_columns, nongaps_per_column


def build_ehmm(names, rows, subsets, molecule, outdirprefix, threads=8, ere=0.59, symfrac=0.0, stats=False, device=None):
    """All models of an eHMM: `subsets` is a list of (label, row indices) over the backbone rows.  Returns the
    list of the reference's tuples in subset order.  wh_hmmbuild runs outside the GIL, so a thread pool scales
    with the host cores (the reference starts one hmmbuild process per subset, algorithm.py:152-154).
    stats=True: the model files carry hmmbuild's three STATS LOCAL lines, as the reference's do (stock HMMER refuses a
    file without them); all models are then built by ONE wh_hmmbuild_batch call, which calibrates them in one batch on
    HIP device `device` (None: the current device if there is one, else the host; -1: the host).  The input FASTA files,
    the model files' other lines and the returned tuples are the same either way."""
    from concurrent.futures import ThreadPoolExecutor
    if stats:
        red = [_reduce_subset([names[i] for i in idx], [rows[i] for i in idx], outdirprefix, label) for label, idx in subsets]
        built = hmmbuild_text_batch([r[1] for r in red], molecule, ["hmmbuild.input.%s" % label for label, _ in subsets],
                                    ere=ere, symfrac=symfrac, stats=True, device=device)
        out = []
        for (label, _), (d, _, retained, nongaps), (text, _, _) in zip(subsets, red, built):
            path = os.path.join(d, "hmmbuild.model.%s" % label)
            with open(path, "w") as f:
                f.write(text)
            out.append((path, label, retained, nongaps))
        return out

    def one(item):
        label, idx = item
        return subset_alignment_and_hmmbuild([names[i] for i in idx], [rows[i] for i in idx], molecule, outdirprefix,
                                             label, ere=ere, symfrac=symfrac)
    if threads <= 1 or len(subsets) <= 1:
        return [one(s) for s in subsets]
    with ThreadPoolExecutor(max_workers=threads) as ex:
        return list(ex.map(one, subsets))
