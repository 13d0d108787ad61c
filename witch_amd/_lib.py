"""ctypes binding of libwitch_hip.so (the C ABI in include/witch_hip.h).

The product path has NO fallback: if the HIP library is missing or a call fails,
an exception is raised.  Nothing here imports the CPU oracle.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libwitch_hip.so")
CSRC = os.path.join(_HERE, "csrc")

WH_MAX_ENVELOPES = 16
FLAG_REPORTED, FLAG_MULTI, FLAG_OVERRIDE, FLAG_TRUNC, FLAG_EXACT = 1, 2, 4, 8, 16
FLAG_FILTERED = 32
BIAS_FILTER_ON = 2       # wh_filter_opts.nobias: WH_BIAS_FILTER_ON
STAGE_MSV, STAGE_BIAS, STAGE_VIT, STAGE_VIT_RAN, STAGE_FWD = 1, 2, 4, 8, 16      # stage byte of wh_filter / wh_score_filtered
VIT_NOT_RUN, VIT_OVERFLOW, MSV_OVERFLOW = -32769, 32768, -1
ALPH_DNA, ALPH_RNA, ALPH_AMINO = 0, 1, 2
WH_OK, WH_EINVAL, WH_EIO, WH_ENODEV, WH_EHIP, WH_ERANGE, WH_ENOMEM = 0, -1, -2, -3, -4, -5, -6      # include/witch_hip.h
WH_BUILD_STATS, WH_BUILD_CALIB_NO_LDS = 1, 4
WH_MSA_TRIM, WH_MSA_NO_LDS, WH_MSA_CONS_HMMER = 1, 2, 4
WH_LENMODEL_ENVELOPE, WH_LENMODEL_SEQUENCE = 0, 1
PATH_P2_WIN, PATH_P2_FULL, PATH_P4_W256, PATH_P4_W512, PATH_P4_WFAIL, PATH_P4_FULL, PATH_DENSE, PATH_MULTI = 1, 2, 4, 8, 16, 32, 64, 128


class WitchHipError(RuntimeError):
    pass


class PairDetail(C.Structure):
    _fields_ = [
        ("fwd_bits", C.c_float), ("seq_score", C.c_float), ("pre_score", C.c_float),
        ("seqbias_nats", C.c_float), ("nregions", C.c_int32), ("nenv", C.c_int32),
        ("env_i", C.c_int32 * WH_MAX_ENVELOPES), ("env_j", C.c_int32 * WH_MAX_ENVELOPES),
        ("envsc", C.c_float * WH_MAX_ENVELOPES), ("domcorr", C.c_float * WH_MAX_ENVELOPES),
    ]


class Domain(C.Structure):
    """wh_domain (include/witch_hip.h); DOMAIN_DTYPE is the same layout for numpy."""
    _fields_ = [
        ("pair", C.c_int64), ("index", C.c_int32), ("of", C.c_int32), ("env_i", C.c_int32), ("env_j", C.c_int32),
        ("ali_i", C.c_int32), ("ali_j", C.c_int32), ("hmm_i", C.c_int32), ("hmm_j", C.c_int32),
        ("bits", C.c_float), ("bias_bits", C.c_float), ("oasc", C.c_float), ("lnP", C.c_float),
    ]


class FilterOpts(C.Structure):
    """wh_filter_opts (include/witch_hip.h): HMMER's thresholds F1, F2, F3 and nobias (1: --nobias, BIAS_FILTER_ON: the bias
    filter runs, 0: refused for now)."""
    _fields_ = [("F1", C.c_double), ("F2", C.c_double), ("F3", C.c_double), ("nobias", C.c_int32)]


class HitsOpts(C.Structure):
    """wh_hits_opts (include/witch_hip.h): the search space sizes and inclusion thresholds of hmmsearch -A."""
    _fields_ = [("Z", C.c_double), ("domZ", C.c_double), ("incE", C.c_double), ("incdomE", C.c_double)]


class SeqTableOpts(C.Structure):
    """wh_seq_table_opts (include/witch_hip.h): the search space sizes (<= 0: the number of targets / of reported sequences)
    and the reporting and inclusion thresholds of hmmsearch --tblout."""
    _fields_ = [("Z", C.c_double), ("domZ", C.c_double), ("E", C.c_double), ("domE", C.c_double), ("incE", C.c_double),
                ("incdomE", C.c_double)]


SEQ_EXPECT_FIELDS = [("exp", "<f4"), ("reg", "<i4"), ("clu", "<i4")]      # wh_seq_expect_rec
SEQ_ROW_FIELDS = [("pair", "<i8"), ("seq_lnP", "<f8"), ("seq_bits", "<f4"), ("seq_bias_bits", "<f4"), ("exp", "<f4"), ("reg", "<i4"),
                  ("clu", "<i4"), ("ov", "<i4"), ("env", "<i4"), ("dom", "<i4"), ("rep", "<i4"), ("inc", "<i4"), ("best", "<i4"),
                  ("best_bits", "<f4"), ("best_bias_bits", "<f4"), ("best_lnP", "<f4"), ("capped", "<i4"), ("reserved", "<i4")]      # wh_seq_row
HIT_ROW_FIELDS = [("query", "<i4"), ("index", "<i4"), ("ali_i", "<i4"), ("ali_j", "<i4")]      # wh_hit_row
DISPLAY_REC_FIELDS = [("query", "<i4"), ("index", "<i4")]      # wh_display_rec
DOMAIN_FIELDS = [("pair", "<i8"), ("index", "<i4"), ("of", "<i4"), ("env_i", "<i4"), ("env_j", "<i4"), ("ali_i", "<i4"),
                 ("ali_j", "<i4"), ("hmm_i", "<i4"), ("hmm_j", "<i4"), ("bits", "<f4"), ("bias_bits", "<f4"), ("oasc", "<f4"),
                 ("lnP", "<f4")]


# every symbol include/witch_hip.h declares: name -> (restype, argtypes)
_P = C.c_void_p
SYMBOLS = {
    "wh_version": (C.c_char_p, []),
    "wh_last_error": (C.c_char_p, []),
    "wh_init": (C.c_int, [C.c_int]),
    "wh_device_info": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int64)]),
    "wh_digitize": (C.c_int, [C.c_int, C.c_char_p, C.c_int64, _P]),
    "wh_ehmm_load": (_P, [C.POINTER(C.c_char_p), _P, _P, C.c_int]),
    "wh_hmmbuild": (C.c_int, [C.c_char_p, C.c_int32, C.c_int64, C.POINTER(C.c_char_p), C.c_char_p, C.c_double, C.c_double,
                            C.c_double, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "wh_hmmbuild2": (C.c_int, [C.c_char_p, C.c_int32, C.c_int64, C.POINTER(C.c_char_p), C.c_char_p, C.c_double, C.c_double,
                             C.c_double, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "wh_hmmbuild_batch": (C.c_int, [C.c_int, C.c_char_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.POINTER(C.c_char_p)),
                                  C.POINTER(C.c_char_p), C.c_double, C.c_double, C.c_double, C.c_int32, C.POINTER(C.c_void_p),
                                  C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "wh_free_text": (None, [C.c_void_p]),
    "wh_merge_sharded": (C.c_int, [C.c_int, _P, _P, C.c_int64, _P, _P, _P, C.c_int32, C.c_int32, _P, _P, C.POINTER(C.c_void_p),
                                 C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "wh_merge": (C.c_int, [C.c_int, _P, _P, C.c_int64, _P, _P, _P, C.c_int32, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                         C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "wh_msa": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int64)] + [C.POINTER(C.c_void_p)] * 5 + [C.POINTER(C.c_int64)]),
    "wh_msa_dev": (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int64)] + [C.POINTER(C.c_void_p)] * 5 +
                   [C.POINTER(C.c_int64), _P]),
    "wh_msa_mapali": (C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int32, C.c_int32, _P, C.c_int64, C.c_int64, C.POINTER(C.c_int64)] +
                      [C.POINTER(C.c_void_p)] * 5 + [C.POINTER(C.c_int64)]),
    "wh_msa_mapali_dev": (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, C.c_int64, C.c_int32, C.c_int32, _P, C.c_int64, C.c_int64,
                                    C.POINTER(C.c_int64)] + [C.POINTER(C.c_void_p)] * 5 + [C.POINTER(C.c_int64), _P]),
    "wh_alignment_checksum": (C.c_int, [C.c_char_p, _P, C.c_int32, C.c_int64, C.POINTER(C.c_uint32)]),
    "wh_ehmm_cksum": (C.c_int, [_P, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_int32)]),
    "wh_ehmm_free": (None, [_P]),
    "wh_ehmm_count": (C.c_int, [_P]),
    "wh_ehmm_alphabet": (C.c_int, [_P]),
    "wh_ehmm_info": (C.c_int, [_P, _P, _P, _P]),
    "wh_ehmm_map": (C.c_int, [_P, C.c_int, _P]),
    "wh_ehmm_max_query_len": (C.c_int, [_P]),
    "wh_query_len_cap": (C.c_int, [C.c_int, _P, C.c_int]),
    "wh_score": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, _P, _P]),
    "wh_score_dev": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64, C.c_int32, _P, _P, _P, _P, _P]),
    "wh_topk": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, _P, _P, _P, _P]),
    "wh_topk_dev": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int, _P, _P, _P, _P, _P]),
    "wh_align": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, C.c_int64, _P, _P]),
    "wh_align_dev": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64, C.c_int32, _P, _P, C.c_int64, _P, _P, _P]),
    "wh_align_pp": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, C.c_int64, _P, _P, _P]),
    "wh_align_pp_dev": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64, C.c_int32, _P, _P, C.c_int64, _P, _P, _P, _P]),
    "wh_align_pp64": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, C.c_int64, _P, _P, _P]),
    "wh_align_pp64_dev": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64, C.c_int32, _P, _P, C.c_int64, _P, _P, _P, _P]),
    "wh_align_pp_len": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, C.c_int64, _P, _P, _P, _P]),
    "wh_align_pp_len_dev": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64, C.c_int32, _P, _P, C.c_int64, _P, _P, _P, _P, _P]),
    "wh_set_domain_length_model": (C.c_int, [_P, C.c_int]),
    "wh_get_domain_length_model": (C.c_int, [_P]),
    "wh_domain_counts": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P]),
    "wh_domain_counts_dev": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, _P]),
    "wh_domains": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, _P, _P]),
    "wh_domains_dev": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64, C.c_int32, _P, _P, _P, _P, _P]),
    "wh_domain_paths": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, _P, _P, _P, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "wh_domain_paths_dev": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64, C.c_int32, _P, _P, _P, _P] + [C.POINTER(C.c_void_p)] * 3 +
                            [C.POINTER(C.c_int64), _P]),
    "wh_hits_msa": (C.c_int, [_P, _P, _P, _P, C.c_int64, _P, _P, _P, C.c_int32, _P, _P, C.c_int32, _P, C.POINTER(C.c_int64),
                              C.POINTER(C.c_void_p), C.POINTER(C.c_int64)] + [C.POINTER(C.c_void_p)] * 5),
    "wh_hits_msa_dev": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, _P, _P, _P, _P, _P, C.c_int32, _P, _P, C.c_int32, C.POINTER(C.c_int64),
                                  C.POINTER(C.c_void_p), C.POINTER(C.c_int64)] + [C.POINTER(C.c_void_p)] * 5 + [_P]),
    "wh_ehmm_consensus": (C.c_int, [_P, C.c_int, _P, C.POINTER(C.c_int32)]),
    "wh_hmm_consensus": (C.c_int, [C.c_char_p, _P, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "wh_domain_display": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, _P, C.c_int32, C.c_double, C.c_double, _P, C.POINTER(C.c_int64)] +
                          [C.POINTER(C.c_void_p)] * 6),
    "wh_domain_display_dev": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, _P, _P, _P, _P, C.c_int32, C.c_double, C.c_double, C.c_int64,
                                        _P, _P, _P, _P, _P, _P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _P]),
    "wh_filter": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, _P, _P, _P]),
    "wh_filter_dev": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64, C.c_int32, _P, _P, _P, _P, _P, _P]),
    "wh_filter_host": (C.c_int, [C.POINTER(C.c_char_p), C.c_int, _P, _P, C.c_int64, _P, _P, _P, _P, _P, _P]),
    "wh_score_filtered": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, _P, _P, _P, _P]),
    "wh_score_filtered_dev": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64, C.c_int32, _P, _P, _P, _P, _P, _P, _P]),
    "wh_last_filter_counts": (C.c_int, [_P, _P]),
    "wh_filter_log_differences": (C.c_int64, [C.c_uint32, C.c_uint32]),
    "wh_seq_expect": (C.c_int, [_P, _P, _P, C.c_int64, _P, C.c_int64, _P]),
    "wh_seq_expect_dev": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64, C.c_int32, _P, C.c_int64, _P, _P]),
    "wh_seq_expect_host": (C.c_int, [C.POINTER(C.c_char_p), C.c_int, _P, _P, C.c_int64, _P, C.c_int64, _P]),
    "wh_seq_table": (C.c_int, [_P, _P, _P, C.c_int64, _P, _P, _P, _P, C.c_int64]),
    "wh_seq_table_dev": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64, C.c_int32, _P, _P, _P, _P, C.c_int64, _P]),
    "wh_seq_table_host": (C.c_int, [C.c_int, _P, _P, _P, C.c_int64, _P, _P, _P, _P, _P, C.c_int64]),
    "wh_last_seq_table_status": (C.c_int, [_P, _P]),
    "wh_ehmm_evparams": (C.c_int, [_P, _P, _P, _P]),
    "wh_hmm_evparams": (C.c_int, [C.c_char_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int32)]),
    "wh_consensus": (C.c_int, [_P, _P, C.c_int64, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int32, _P, _P]),
    "wh_consensus_dev": (C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    "wh_last_align_status": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _P, C.c_int64]),
    "wh_last_align_paths": (C.c_int, [_P, _P]),
    "wh_last_score_paths": (C.c_int, [_P, _P]),
    "wh_last_score_counters": (C.c_int, [_P, _P]),
    "wh_set_path_buffer": (C.c_int, [_P, _P]),
    "wh_set_path_buffer16": (C.c_int, [_P, _P]),
    "wh_last_queue_reruns": (C.c_int, [_P]),
    "wh_last_region_overflow": (C.c_int, [_P, _P]),
    "wh_last_long_query_pairs": (C.c_int, [_P, _P]),
    "wh_last_long_score_pairs": (C.c_int, [_P, _P]),
    "wh_last_long_align_pairs": (C.c_int, [_P, _P]),
    "wh_last_score_launches": (C.c_int, [_P, _P, _P, _P, C.c_int]),
    "wh_last_score_shapes": (C.c_int, [_P, _P, _P, _P, C.c_int]),
    "wh_last_kernel_ms": (C.c_int, [_P, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "wh_set_timing": (C.c_int, [_P, C.c_int]),
    "wh_set_option": (C.c_int, [_P, C.c_char_p, C.c_char_p]),
}

_LIB = None


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile the HIP extension in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC, "-j4"] + (["-B"] if force else [])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or r.returncode != 0:
        print(r.stdout)
    if r.returncode != 0:
        raise WitchHipError("building libwitch_hip.so failed:\n" + r.stdout[-4000:])
    return LIB_PATH


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise WitchHipError(
                "libwitch_hip.so is missing (%s). Build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` or `make -C witch_amd/csrc`. There is no CPU fallback." % LIB_PATH)
        # PyTorch-ROCm bundles its own HIP runtime; two HIP runtimes in one process cannot
        # both own the GPU.  Importing torch first makes the loader bind this library to the
        # runtime torch already loaded (same SONAME) whenever torch is used in the process.
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            f = getattr(L, name)      # AttributeError if the library does not export it
            f.restype = res
            f.argtypes = args
        _LIB = L
    return _LIB


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().wh_last_error()
        raise WitchHipError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else "?"))
