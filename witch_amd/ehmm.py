"""EHMM: an ensemble of profile HMMs resident on one MI355X, and the three operators of
the hot path (score -> top-k weights -> align) over the C ABI of libwitch_hip.so.

Host entry points take/return numpy arrays (the library stages them over PCIe);
the ``*_t`` entry points take torch CUDA tensors already resident in HBM and enqueue
on torch's current stream - PyTorch is only the allocator/stream plumbing here.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import BIAS_FILTER_ON, DOMAIN_FIELDS, FilterOpts, PairDetail, WitchHipError, check, lib


def pack_queries(seqs):
    """list of uint8 arrays -> (residues uint8 [total], offsets int64 [n+1])"""
    offs = np.zeros(len(seqs) + 1, dtype=np.int64)
    if len(seqs):
        offs[1:] = np.cumsum([len(s) for s in seqs])
        res = np.concatenate([np.asarray(s, dtype=np.uint8) for s in seqs])
    else:
        res = np.zeros(0, dtype=np.uint8)
    return np.ascontiguousarray(res), offs


def alignment_checksum(molecule, rows):
    """hmmbuild's CKSUM of an alignment (wh_alignment_checksum): rows of one length (str or bytes), molecule "dna" | "rna" |
    "amino".  Host code, no GPU."""
    rows = [r.encode() if isinstance(r, str) else bytes(r) for r in rows]
    if not rows or len(set(len(r) for r in rows)) != 1:
        raise ValueError("alignment_checksum: the rows must be of one length")
    out = C.c_uint32(0)
    check(lib().wh_alignment_checksum(molecule.encode(), b"".join(rows), len(rows), len(rows[0]), C.byref(out)), "wh_alignment_checksum")
    return int(out.value)


def seq_expect_host(hmm_paths, residues, offsets, pairs):
    """The counts of hmmsearch --tblout without a device (wh_seq_expect_host: float64 scalar code over the model files): a
    structured array (exp, reg, clu), one record per entry of pairs (q * H + h)."""
    residues = np.ascontiguousarray(residues, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    pairs = np.ascontiguousarray(pairs, dtype=np.int64)
    n = len(hmm_paths)
    arr = (C.c_char_p * n)(*[str(p).encode() for p in hmm_paths])
    out = np.zeros(len(pairs), dtype=np.dtype(_lib.SEQ_EXPECT_FIELDS))
    check(lib().wh_seq_expect_host(arr, n, residues.ctypes.data, offsets.ctypes.data, len(offsets) - 1, pairs.ctypes.data, len(pairs),
                                   out.ctypes.data), "wh_seq_expect_host")
    return out


def seq_table_opts(Z=None, domZ=None, E=10.0, domE=10.0, incE=0.01, incdomE=0.01) -> _lib.SeqTableOpts:
    return _lib.SeqTableOpts(0.0 if Z is None else float(Z), 0.0 if domZ is None else float(domZ), float(E), float(domE), float(incE),
                             float(incdomE))


def seq_table_host(tau, lam, lengths, flags, detail, expect, Z=None, domZ=None, E=10.0, domE=10.0, incE=0.01, incdomE=0.01):
    """The row assembly of hmmsearch --tblout on host arrays, without a handle or a device (wh_seq_table_host): tau, lam
    float32 [H]; lengths int64 [nq]; flags uint8 [nq, H]; detail: PairDetail records; expect: (exp, reg, clu) of the reported
    pairs in pair order.  Returns the rows (SEQ_ROW_FIELDS)."""
    tau = np.ascontiguousarray(tau, dtype=np.float32)
    lam = np.ascontiguousarray(lam, dtype=np.float32)
    lengths = np.ascontiguousarray(lengths, dtype=np.int64)
    flags = np.ascontiguousarray(flags, dtype=np.uint8)
    expect = np.ascontiguousarray(expect, dtype=np.dtype(_lib.SEQ_EXPECT_FIELDS))
    H, nq = len(tau), len(lengths)
    cap = int((flags.reshape(-1) & 1).sum())
    out = np.zeros(cap, dtype=np.dtype(_lib.SEQ_ROW_FIELDS))
    o = seq_table_opts(Z, domZ, E, domE, incE, incdomE)
    n = lib().wh_seq_table_host(H, tau.ctypes.data, lam.ctypes.data, lengths.ctypes.data, nq, flags.ctypes.data, C.addressof(detail),
                                expect.ctypes.data, C.byref(o), out.ctypes.data, cap)
    check(min(n, 0), "wh_seq_table_host")
    return out[:n]


def hmm_consensus(hmm_path):
    """(the CONS column of a model file or None, {"CONS", "RF", "CS": bool} of its header) through the library's parser,
    without a handle or a device (wh_hmm_consensus)."""
    M, present = C.c_int32(0), C.c_int32(0)
    check(lib().wh_hmm_consensus(str(hmm_path).encode(), None, 0, C.byref(M), C.byref(present)), "wh_hmm_consensus")
    out = C.create_string_buffer(int(M.value) + 1)
    check(lib().wh_hmm_consensus(str(hmm_path).encode(), out, int(M.value), None, C.byref(present)), "wh_hmm_consensus")
    keys = {"CONS": bool(present.value & 1), "RF": bool(present.value & 2), "CS": bool(present.value & 4)}
    return (out.raw[:int(M.value)].decode("ascii") if keys["CONS"] else None), keys


class DevView:
    """An array in the library's device workspace, where a torch tensor is expected by the *_t methods: its address and its
    element count."""

    def __init__(self, ptr, n):
        self._ptr, self._n = ptr, int(n)

    def data_ptr(self):
        return self._ptr

    def numel(self):
        return self._n


class EHMM:
    def __init__(self, hmm_paths, hmm_index=None, nseq=None, device: int = 0):
        L = lib()
        check(L.wh_init(int(device)), "wh_init")
        n = len(hmm_paths)
        arr = (C.c_char_p * n)(*[str(p).encode() for p in hmm_paths])
        idx = np.ascontiguousarray(hmm_index if hmm_index is not None else np.arange(n), dtype=np.int32)
        ns = None if nseq is None else np.ascontiguousarray(nseq, dtype=np.int32)
        self._h = L.wh_ehmm_load(arr, idx.ctypes.data, None if ns is None else ns.ctypes.data, n)
        if not self._h:
            raise WitchHipError("wh_ehmm_load failed: %s" % L.wh_last_error().decode())
        self.device = int(device)
        self.paths = list(hmm_paths)
        self.H = L.wh_ehmm_count(self._h)
        self.alphabet = L.wh_ehmm_alphabet(self._h)
        self.M = np.zeros(self.H, dtype=np.int32)
        self.nseq = np.zeros(self.H, dtype=np.int32)
        self.index = np.zeros(self.H, dtype=np.int32)
        check(L.wh_ehmm_info(self._h, self.M.ctypes.data, self.nseq.ctypes.data, self.index.ctypes.data),
              "wh_ehmm_info")
        self.pos_of_index = {int(v): i for i, v in enumerate(self.index)}

    def close(self):
        if getattr(self, "_h", None):
            lib().wh_ehmm_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ helpers
    def digitize(self, text: str) -> np.ndarray:
        out = np.empty(len(text), dtype=np.uint8)
        bad = lib().wh_digitize(self.alphabet, text.encode(), len(text), out.ctypes.data)
        if bad != 0:
            raise ValueError("query contains %d characters outside the %s alphabet" %
                             (bad, "amino" if self.alphabet == 2 else "nucleic"))
        return out

    def digitize_many(self, texts):
        """Digitise a list of sequence texts in ONE library call: (residues uint8 [total], offsets int64 [n+1])."""
        lens = np.fromiter((len(t) for t in texts), dtype=np.int64, count=len(texts))
        offs = np.zeros(len(texts) + 1, dtype=np.int64)
        np.cumsum(lens, out=offs[1:])
        blob = "".join(texts).encode()
        if len(blob) != int(offs[-1]):
            raise ValueError("query sequences must be ASCII")
        out = np.empty(len(blob), dtype=np.uint8)
        bad = lib().wh_digitize(self.alphabet, blob, len(blob), out.ctypes.data) if len(blob) else 0
        if bad != 0:
            raise ValueError("queries contain %d characters outside the %s alphabet" %
                             (bad, "amino" if self.alphabet == 2 else "nucleic"))
        return out, offs

    def map_columns(self, h: int) -> np.ndarray:
        out = np.zeros(int(self.M[h]), dtype=np.int32)
        check(lib().wh_ehmm_map(self._h, int(h), out.ctypes.data), "wh_ehmm_map")
        return out

    def set_timing(self, on: bool):
        check(lib().wh_set_timing(self._h, 1 if on else 0), "wh_set_timing")

    def set_option(self, name: str, value: str = ""):
        """Development knob on a live handle (include/witch_hip.h: wh_set_option)."""
        check(lib().wh_set_option(self._h, name.encode(), str(value).encode()), "wh_set_option")

    _LENGTH_MODELS = ("envelope", "sequence")      # WH_LENMODEL_ENVELOPE, WH_LENMODEL_SEQUENCE

    def set_domain_length_model(self, model: str):
        """The length model the domain stage (domains, domain_paths, hits_msa, domain_display) aligns an envelope under:
        "envelope" (the default) - its own Ld residues, hmmalign's alignment; "sequence" - its whole sequence's L residues,
        hmmsearch's own alignment (include/witch_hip.h: wh_set_domain_length_model)."""
        if model not in self._LENGTH_MODELS:
            raise ValueError("domain length model %r: one of %s" % (model, ", ".join(map(repr, self._LENGTH_MODELS))))
        check(lib().wh_set_domain_length_model(self._h, self._LENGTH_MODELS.index(model)), "wh_set_domain_length_model")

    @property
    def domain_length_model(self) -> str:
        v = lib().wh_get_domain_length_model(self._h)
        if v < 0:
            check(v, "wh_get_domain_length_model")
        return self._LENGTH_MODELS[v]

    def last_kernel_ms(self, which: int):
        ms, n = C.c_double(0), C.c_int(0)
        check(lib().wh_last_kernel_ms(self._h, which, C.byref(ms), C.byref(n)), "wh_last_kernel_ms")
        return ms.value, n.value

    def last_score_launches(self):
        """[(cells per lane, kernel family, ms)] of the scoring launches of the last score call (timing mode)."""
        q = np.zeros(64, dtype=np.int32)
        kind = np.zeros(64, dtype=np.int32)
        ms = np.zeros(64, dtype=np.float64)
        n = lib().wh_last_score_launches(self._h, q.ctypes.data, kind.ctypes.data, ms.ctypes.data, 64)
        check(min(n, 0), "wh_last_score_launches")
        return [(int(q[t]), int(kind[t]), float(ms[t])) for t in range(min(n, 64))]

    def last_score_shapes(self):
        """[(cells per lane, waves per workgroup, multihit window mode 0 / 1 / 2)] of the one-wave scoring launches of the
        last scoring pass, timing mode or not (include/witch_hip.h: wh_last_score_shapes)."""
        q, waves, p2win = (np.zeros(64, dtype=np.int32) for _ in range(3))
        n = lib().wh_last_score_shapes(self._h, q.ctypes.data, waves.ctypes.data, p2win.ctypes.data, 64)
        check(min(n, 0), "wh_last_score_shapes")
        return [(int(q[t]), int(waves[t]), int(p2win[t])) for t in range(min(n, 64))]

    # ------------------------------------------------------------------ host (numpy) operators
    def last_score_paths(self):
        """Backward sweeps of the last score call by path: envelope sweeps {"window256", "window512", "window_rejected",
        "full_width"}, multihit sweeps {"p2_window", "p2_window_in_doubt"} (include/witch_hip.h: wh_last_score_paths)."""
        p6 = np.zeros(6, dtype=np.int64)
        check(lib().wh_last_score_paths(self._h, p6.ctypes.data), "wh_last_score_paths")
        return {"window256": int(p6[0]), "window512": int(p6[1]), "window_rejected": int(p6[2]), "full_width": int(p6[3]),
                "p2_window": int(p6[4]), "p2_window_in_doubt": int(p6[5])}

    def last_score_spill_bytes(self) -> int:
        """Bytes of Forward rows the envelope sweeps of the last score call stored (include/witch_hip.h: wh_last_score_counters)."""
        c8 = np.zeros(8, dtype=np.int64)
        check(lib().wh_last_score_counters(self._h, c8.ctypes.data), "wh_last_score_counters")
        return int(c8[6])

    def last_long_list_pairs(self) -> int:
        """Pairs of the last score call that had more regions than a scoring kernel's list holds (WH_MAX_ENVELOPES) and were
        scored again by the long-list pass (include/witch_hip.h: wh_last_score_counters, out8[7])."""
        c8 = np.zeros(8, dtype=np.int64)
        check(lib().wh_last_score_counters(self._h, c8.ctypes.data), "wh_last_score_counters")
        return int(c8[7])

    def last_region_overflow(self):
        """The big-region pass of the last score call: pairs it scored again because ONE multidomain region needed more
        domains per sampled trace, segments or significant clusters than the resolver's fixed lists hold, and the largest
        of each it met (all 0: no such region).  include/witch_hip.h: wh_last_region_overflow."""
        o4 = np.zeros(4, dtype=np.int64)
        check(lib().wh_last_region_overflow(self._h, o4.ctypes.data), "wh_last_region_overflow")
        return {"pairs": int(o4[0]), "max_domains": int(o4[1]), "max_segments": int(o4[2]), "max_clusters": int(o4[3])}

    def last_long_queries(self):
        """The long-query pass of the last score call: (pairs it scored again because their query is longer than the length
        cap of the resolver's main launches, the longest query among them); (0, 0) when every query of the call fitted
        the resolver's LDS block.  include/witch_hip.h: wh_last_long_query_pairs."""
        o2 = np.zeros(2, dtype=np.int64)
        check(lib().wh_last_long_query_pairs(self._h, o2.ctypes.data), "wh_last_long_query_pairs")
        return int(o2[0]), int(o2[1])

    def last_long_score(self):
        """The long-query scoring pass of the last score call: (pairs it scored because their query is longer than the length
        cap of the call's scoring launches, the longest query among them); (0, 0) when every size class planned the call's
        longest query.  include/witch_hip.h: wh_last_long_score_pairs."""
        o2 = np.zeros(2, dtype=np.int64)
        check(lib().wh_last_long_score_pairs(self._h, o2.ctypes.data), "wh_last_long_score_pairs")
        return int(o2[0]), int(o2[1])

    def last_long_align(self):
        """The same for the last align call: (pairs handed to the any-size float64 alignment kernel for their query's length,
        the longest query among them).  include/witch_hip.h: wh_last_long_align_pairs."""
        o2 = np.zeros(2, dtype=np.int64)
        check(lib().wh_last_long_align_pairs(self._h, o2.ctypes.data), "wh_last_long_align_pairs")
        return int(o2[0]), int(o2[1])

    def max_query_len(self) -> int:
        """Length up to which queries stay on the float32 kernels (include/witch_hip.h: wh_ehmm_max_query_len)."""
        n = lib().wh_ehmm_max_query_len(self._h)
        check(min(n, 0), "wh_ehmm_max_query_len")
        return int(n)

    def set_path_buffer(self, paths_t):
        """Registers a CUDA uint8 tensor of nq x H bytes that later score calls fill with WH_PATH_* bits per pair
        (staged launches only; None switches it off).  The caller keeps the tensor alive (include/witch_hip.h)."""
        check(lib().wh_set_path_buffer(self._h, paths_t.data_ptr() if paths_t is not None else None), "wh_set_path_buffer")
        self._path_t = paths_t

    def set_path_buffer16(self, paths_t):
        """Registers a contiguous CUDA int16 / uint16 tensor of nq x H elements that later score calls fill with the 16-bit
        WH_PATH_* record per pair (None switches it off): the default kernel writes it, as do the staged launches and the
        kernels without windows.  The caller keeps the tensor alive (include/witch_hip.h: wh_set_path_buffer16)."""
        if paths_t is not None:
            import torch
            if paths_t.dtype not in (torch.int16, getattr(torch, "uint16", torch.int16)) or not paths_t.is_cuda or not paths_t.is_contiguous():
                raise ValueError("set_path_buffer16: a contiguous CUDA tensor of torch.int16 or torch.uint16")
        check(lib().wh_set_path_buffer16(self._h, paths_t.data_ptr() if paths_t is not None else None), "wh_set_path_buffer16")
        self._path16_t = paths_t

    def last_queue_reruns(self) -> int:
        """Scoring passes the last score call repeated because the resolver's queue overflowed its estimate (0 or 1)."""
        n = lib().wh_last_queue_reruns(self._h)
        check(min(n, 0), "wh_last_queue_reruns")
        return int(n)

    @staticmethod
    def filter_opts(filters=True, nobias=False, bias=False) -> FilterOpts:
        """wh_filter_opts from filters = True (HMMER's defaults F1 = 0.02, F2 = 1e-3, F3 = 1e-5) or (F1, F2, F3).
        bias=True: HMMER's bias filter runs (WH_BIAS_FILTER_ON; opt-in for now, the default later); nobias=True: it does
        not (hmmsearch --nobias); neither: the library refuses the call; both: ValueError."""
        F = (0.02, 1e-3, 1e-5) if filters is True else tuple(float(x) for x in filters)
        if len(F) != 3:
            raise ValueError("filters: True or (F1, F2, F3)")
        if bias and nobias:
            raise ValueError("bias=True (the bias filter runs) and nobias=True (hmmsearch --nobias) exclude each other")
        return FilterOpts(F[0], F[1], F[2], BIAS_FILTER_ON if bias else 1 if nobias else 0)

    def filter(self, residues, offsets, filters=True, nobias=False, want_raw=False, bias=False):
        """hmmsearch's acceleration filters over every (query, model) pair (include/witch_hip.h: wh_filter): stage uint8
        [nq, H] (bit 0 passed MSV, 1 passed bias, 2 passed Viterbi, 3 the Viterbi sweep ran) and filter_bias_nats float32
        [nq, H]; with want_raw also the two filters' raw integer scores, int32 [nq, H] each.  The bias filter is an
        opt-in: bias=True runs it; without it nobias=False is still refused (WitchHipError), as hmmsearch without --nobias
        is by the level-0 program unless its server is told to run the stage."""
        residues = np.ascontiguousarray(residues, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        nq = len(offsets) - 1
        o = self.filter_opts(filters, nobias, bias)
        stage = np.zeros((nq, self.H), dtype=np.uint8)
        bias = np.zeros((nq, self.H), dtype=np.float32)
        msv = np.zeros((nq, self.H), dtype=np.int32) if want_raw else None
        vit = np.zeros((nq, self.H), dtype=np.int32) if want_raw else None
        check(lib().wh_filter(self._h, residues.ctypes.data, offsets.ctypes.data, nq, C.byref(o), stage.ctypes.data,
                              bias.ctypes.data, None if msv is None else msv.ctypes.data,
                              None if vit is None else vit.ctypes.data), "wh_filter")
        return (stage, bias, msv, vit) if want_raw else (stage, bias)

    def last_filter_counts(self):
        """The last filter / filtered score call: {"pairs", "msv", "bias", "vit", "fwd", "scored"} - pairs, pairs past each
        of the four stages, pairs handed to the scoring kernels (include/witch_hip.h: wh_last_filter_counts)."""
        c = np.zeros(6, dtype=np.int64)
        check(lib().wh_last_filter_counts(self._h, c.ctypes.data), "wh_last_filter_counts")
        return dict(zip(("pairs", "msv", "bias", "vit", "fwd", "scored"), (int(v) for v in c)))

    def score(self, residues, offsets, want_fwd=False, want_detail=False, filters=None, nobias=False, want_stage=False, bias=False):
        """filters=None: hmmsearch --max, as ever.  filters=True or (F1, F2, F3): behind hmmsearch's acceleration filters
        (wh_score_filtered): a pair that a stage rejects comes back with FLAG_FILTERED and without FLAG_REPORTED;
        want_stage appends the stage bytes [nq, H].  bias=True: with HMMER's bias filter (filter_opts)."""
        residues = np.ascontiguousarray(residues, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        nq = len(offsets) - 1
        deci = np.zeros((nq, self.H), dtype=np.int32)
        flags = np.zeros((nq, self.H), dtype=np.uint8)
        fwd = np.zeros((nq, self.H), dtype=np.float32) if want_fwd else None
        det = (PairDetail * (nq * self.H))() if want_detail else None
        stage = np.zeros((nq, self.H), dtype=np.uint8) if want_stage else None
        if filters is None or filters is False:
            if nobias or want_stage or bias:
                raise ValueError("nobias / bias / want_stage belong to a filtered call (filters=True or (F1, F2, F3))")
            check(lib().wh_score(self._h, residues.ctypes.data, offsets.ctypes.data, nq, deci.ctypes.data,
                                 flags.ctypes.data, None if fwd is None else fwd.ctypes.data,
                                 None if det is None else C.addressof(det)), "wh_score")
        else:
            o = self.filter_opts(filters, nobias, bias)
            check(lib().wh_score_filtered(self._h, residues.ctypes.data, offsets.ctypes.data, nq, C.byref(o), deci.ctypes.data,
                                          flags.ctypes.data, None if fwd is None else fwd.ctypes.data,
                                          None if det is None else C.addressof(det),
                                          None if stage is None else stage.ctypes.data), "wh_score_filtered")
        out = [deci, flags]
        if want_fwd:
            out.append(fwd)
        if want_detail:
            out.append(det)
        if want_stage:
            out.append(stage)
        return tuple(out)

    def topk(self, decibits, flags, k: int):
        decibits = np.ascontiguousarray(decibits, dtype=np.int32)
        flags = np.ascontiguousarray(flags, dtype=np.uint8)
        nq = decibits.shape[0]
        idx = np.full((nq, k), -1, dtype=np.int32)
        w = np.zeros((nq, k), dtype=np.float64)
        nk = np.zeros(nq, dtype=np.int32)
        nu = np.zeros(nq, dtype=np.int32)
        check(lib().wh_topk(self._h, decibits.ctypes.data, flags.ctypes.data, nq, int(k), idx.ctypes.data,
                            w.ctypes.data, nk.ctypes.data, nu.ctypes.data), "wh_topk")
        return idx, w, nk, nu

    def align(self, residues, offsets, pair_q, pair_h, want_pp=False, cfg_len=None):
        """cols (CSR over the residues of each pair) and col_offsets; with want_pp also pp (float32, CSR like cols): the
        posterior probability of each residue's state on the returned path (include/witch_hip.h: wh_align_pp);
        want_pp="float64": as float64 (wh_align_pp64), which the any-size float64 kernel fills unrounded.
        cfg_len (int32 per query, each >= 1; float32 posteriors or none): the length each query's unihit length model is
        configured for in place of its own (wh_align_pp_len) - the whole sequence's, for an envelope aligned as hmmsearch
        aligns it."""
        residues = np.ascontiguousarray(residues, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        pair_q = np.ascontiguousarray(pair_q, dtype=np.int64)
        pair_h = np.ascontiguousarray(pair_h, dtype=np.int32)
        lens = offsets[pair_q + 1] - offsets[pair_q] if len(pair_q) else np.zeros(0, np.int64)
        co = np.zeros(len(pair_q) + 1, dtype=np.int64)
        co[1:] = np.cumsum(lens)
        cols = np.full(int(co[-1]), -1, dtype=np.int32)
        if cfg_len is not None:
            if want_pp == "float64":
                raise ValueError("align: cfg_len comes with float32 posteriors (want_pp=True) or none")
            cfg_len = np.ascontiguousarray(cfg_len, dtype=np.int32)
            if cfg_len.shape != (len(offsets) - 1,):
                raise ValueError("align: cfg_len has one entry per query")
            pp = np.zeros(int(co[-1]), dtype=np.float32) if want_pp else None
            if len(pair_q):
                check(lib().wh_align_pp_len(self._h, residues.ctypes.data, offsets.ctypes.data, len(offsets) - 1,
                                            pair_q.ctypes.data, pair_h.ctypes.data, len(pair_q), co.ctypes.data,
                                            cols.ctypes.data, pp.ctypes.data if want_pp else None, cfg_len.ctypes.data), "wh_align_pp_len")
            return (cols, co, pp) if want_pp else (cols, co)
        if not want_pp:
            if len(pair_q):
                check(lib().wh_align(self._h, residues.ctypes.data, offsets.ctypes.data, len(offsets) - 1,
                                     pair_q.ctypes.data, pair_h.ctypes.data, len(pair_q), co.ctypes.data,
                                     cols.ctypes.data), "wh_align")
            return cols, co
        wide = want_pp == "float64"
        pp = np.zeros(int(co[-1]), dtype=np.float64 if wide else np.float32)
        if len(pair_q):
            check((lib().wh_align_pp64 if wide else lib().wh_align_pp)(self._h, residues.ctypes.data, offsets.ctypes.data, len(offsets) - 1,
                                    pair_q.ctypes.data, pair_h.ctypes.data, len(pair_q), co.ctypes.data,
                                    cols.ctypes.data, pp.ctypes.data), "wh_align_pp")
        return cols, co, pp

    @staticmethod
    def _msa_outputs():
        W, npl = C.c_int64(0), C.c_int64(0)
        ptrs = [C.c_void_p(None) for _ in range(5)]
        return W, npl, ptrs

    def _msa_collect(self, nq, h, W, npl, ptrs, n_map=0):
        """The malloc'ed buffers of wh_msa / wh_msa_dev (and their --mapali forms: n_map rows in front, without PP rows) as
        numpy arrays (copied; the buffers are released)."""
        W, M = int(W.value), int(self.M[h])
        sizes = [((n_map + nq) * W, np.uint8), (nq * W, np.uint8), (W, np.uint8), (W, np.uint8), (M, np.int32)]
        out = []
        for ptr, (n, dt) in zip(ptrs, sizes):
            nbytes = n * np.dtype(dt).itemsize
            out.append(np.frombuffer((C.c_char * nbytes).from_address(ptr.value), dtype=dt).copy() if nbytes else np.zeros(0, dtype=dt))
            lib().wh_free_text(ptr)
        rows, pp_rows, pp_cons, rf, matmap = out
        return {"W": W, "rows": rows.reshape(n_map + nq, W), "pp_rows": pp_rows.reshape(nq, W), "pp_cons": pp_cons, "rf": rf,
                "matmap": matmap, "pathless": int(npl.value)}

    @staticmethod
    def _mapali_rows(mapali):
        """mapali = (names, rows) -> uint8 [n_map, alen]: the rows (str, bytes or uint8 arrays) of one length."""
        rows = [r.encode() if isinstance(r, str) else bytes(bytearray(r)) for r in mapali[1]]
        if len(set(len(r) for r in rows)) > 1:
            raise ValueError("msa: the rows of the mapali alignment differ in length")
        return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), len(rows[0]) if rows else 0)

    def cksum(self, h=0):
        """The CKSUM line of model h (hmmbuild's checksum of the alignment it was built from), None where the file has none."""
        v, present = C.c_uint32(0), C.c_int32(0)
        check(lib().wh_ehmm_cksum(self._h, int(h), C.byref(v), C.byref(present)), "wh_ehmm_cksum")
        return int(v.value) if present.value else None

    def msa(self, residues, offsets, text, h=0, trim=False, no_lds=False, mapali=None):
        """hmmalign's alignment of ALL the sequences to model h (include/witch_hip.h: wh_msa): the sequences are aligned
        (wh_align_pp_dev) and the alignment is assembled on the device.  text: the sequences' characters as given, one
        byte per residue (bytes, str or uint8 array).  Returns {"W", "rows" uint8 [nq, W], "pp_rows" uint8 [nq, W],
        "pp_cons" uint8 [W], "rf" uint8 [W], "matmap" int32 [M], "pathless"}; trim: hmmalign --trim; no_lds: test hook
        (WH_MSA_NO_LDS).  mapali=(names, rows): hmmalign --mapali (wh_msa_mapali) - the rows of the alignment the model was
        built from come first in "rows" ([n_map + nq, W]); they have no PP rows ("pp_rows" stays [nq, W]).  An alignment that
        is not the model's (checksum mismatch) raises."""
        residues = np.ascontiguousarray(residues, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if isinstance(text, str):
            text = text.encode()
        text = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text, dtype=np.uint8)
        nq = len(offsets) - 1
        if len(text) != len(residues) or (nq and int(offsets[-1]) != len(residues)):
            raise ValueError("msa: residues, text and offsets disagree")
        W, npl, ptrs = self._msa_outputs()
        flags = (_lib.WH_MSA_TRIM if trim else 0) | (_lib.WH_MSA_NO_LDS if no_lds else 0)
        if mapali is not None:
            mrows = self._mapali_rows(mapali)
            check(lib().wh_msa_mapali(self._h, residues.ctypes.data, offsets.ctypes.data, text.ctypes.data, nq, int(h), flags,
                                      mrows.ctypes.data, mrows.shape[0], mrows.shape[1], C.byref(W), *[C.byref(p) for p in ptrs],
                                      C.byref(npl)), "wh_msa_mapali")
            return self._msa_collect(nq, int(h), W, npl, ptrs, n_map=mrows.shape[0])
        check(lib().wh_msa(self._h, residues.ctypes.data, offsets.ctypes.data, text.ctypes.data, nq, int(h), flags, C.byref(W),
                           *[C.byref(p) for p in ptrs], C.byref(npl)), "wh_msa")
        return self._msa_collect(nq, int(h), W, npl, ptrs)

    def evparams(self):
        """(tau float32 [H], lambda float32 [H], present bool [H]): the models' "STATS LOCAL FORWARD" parameters, NaN where a
        model file has no such line (include/witch_hip.h: wh_ehmm_evparams)."""
        tau = np.zeros(self.H, dtype=np.float32)
        lam = np.zeros(self.H, dtype=np.float32)
        present = np.zeros(self.H, dtype=np.int32)
        check(lib().wh_ehmm_evparams(self._h, tau.ctypes.data, lam.ctypes.data, present.ctypes.data), "wh_ehmm_evparams")
        return tau, lam, present.astype(bool)

    def seq_expect(self, residues, offsets, pairs):
        """exp, reg, clu of hmmsearch --tblout for the pairs q * H + h (include/witch_hip.h: wh_seq_expect): the two
        full-width multihit sweeps recomputed on the device; a structured array (exp, reg, clu)."""
        residues = np.ascontiguousarray(residues, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        pairs = np.ascontiguousarray(pairs, dtype=np.int64)
        out = np.zeros(len(pairs), dtype=np.dtype(_lib.SEQ_EXPECT_FIELDS))
        check(lib().wh_seq_expect(self._h, residues.ctypes.data, offsets.ctypes.data, len(offsets) - 1, pairs.ctypes.data, len(pairs),
                                  out.ctypes.data), "wh_seq_expect")
        return out

    def seq_table(self, residues, offsets, flags, detail, Z=None, domZ=None, E=10.0, domE=10.0, incE=0.01, incdomE=0.01):
        """The rows of hmmsearch's per-sequence table (--tblout), one per reported pair in pair order, from the flags and
        detail records of score(want_detail=True): a structured array with the fields of wh_seq_row (include/witch_hip.h:
        wh_seq_table).  Z / domZ None: the number of queries / of reported pairs."""
        residues = np.ascontiguousarray(residues, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        flags = np.ascontiguousarray(flags, dtype=np.uint8)
        nq = len(offsets) - 1
        cap = int((flags.reshape(-1) & 1).sum())
        out = np.zeros(cap, dtype=np.dtype(_lib.SEQ_ROW_FIELDS))
        o = seq_table_opts(Z, domZ, E, domE, incE, incdomE)
        n = lib().wh_seq_table(self._h, residues.ctypes.data, offsets.ctypes.data, nq, flags.ctypes.data, C.addressof(detail),
                               C.byref(o), out.ctypes.data, cap)
        check(min(n, 0), "wh_seq_table")
        return out[:n]

    def last_seq_table_status(self):
        """The last seq_table call: {"rows", "capped", "reg_mismatch", "any_size"} (wh_last_seq_table_status)."""
        c = np.zeros(4, dtype=np.int64)
        check(lib().wh_last_seq_table_status(self._h, c.ctypes.data), "wh_last_seq_table_status")
        return dict(zip(("rows", "capped", "reg_mismatch", "any_size"), (int(v) for v in c)))

    def domain_counts(self, flags, detail):
        """(counts int32 [nq, H], n_unlisted int32 [nq, H]) from the flags and detail records of score(want_detail=True)
        (include/witch_hip.h: wh_domain_counts)."""
        flags = np.ascontiguousarray(flags, dtype=np.uint8)
        nq = flags.size // self.H
        counts = np.zeros((nq, self.H), dtype=np.int32)
        unl = np.zeros((nq, self.H), dtype=np.int32)
        if nq:
            check(lib().wh_domain_counts(self._h, flags.ctypes.data, C.addressof(detail), nq, counts.ctypes.data,
                                         unl.ctypes.data), "wh_domain_counts")
        return counts, unl

    def domains(self, residues, offsets, flags, detail, want_unlisted=False):
        """The per-domain records of a scoring call: (records, dom_off) - a numpy structured array with the fields of
        wh_domain (pair, index, of, env_i, env_j, ali_i, ali_j, hmm_i, hmm_j, bits, bias_bits, oasc, lnP) and the CSR
        dom_off int64 [nq * H + 1]: pair q * H + h owns records dom_off[p] .. dom_off[p + 1].  flags, detail: what
        score(residues, offsets, want_detail=True) returned.  want_unlisted: also n_unlisted int32 [nq, H]
        (include/witch_hip.h: wh_domain_counts, wh_domains)."""
        residues = np.ascontiguousarray(residues, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        flags = np.ascontiguousarray(flags, dtype=np.uint8)
        nq = len(offsets) - 1
        counts, unl = self.domain_counts(flags, detail)
        dom_off = np.zeros(nq * self.H + 1, dtype=np.int64)
        np.cumsum(counts.reshape(-1), out=dom_off[1:])
        out = np.zeros(int(dom_off[-1]), dtype=np.dtype(DOMAIN_FIELDS))
        if nq:
            check(lib().wh_domains(self._h, residues.ctypes.data, offsets.ctypes.data, nq, flags.ctypes.data,
                                   C.addressof(detail), dom_off.ctypes.data, out.ctypes.data), "wh_domains")
        return (out, dom_off, unl) if want_unlisted else (out, dom_off)

    def domain_paths(self, residues, offsets, flags, detail):
        """domains() that also returns the alignment of every envelope (include/witch_hip.h: wh_domain_paths): (records,
        dom_off, env_off int64 [n + 1], cols int32, pp float32) - env_off is the CSR of the envelopes in record order, cols
        the 0-based node (-1: none) and pp the posterior of every envelope residue.  The records are domains()' bit for bit."""
        residues = np.ascontiguousarray(residues, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        flags = np.ascontiguousarray(flags, dtype=np.uint8)
        nq = len(offsets) - 1
        counts, _ = self.domain_counts(flags, detail)
        dom_off = np.zeros(nq * self.H + 1, dtype=np.int64)
        np.cumsum(counts.reshape(-1), out=dom_off[1:])
        n = int(dom_off[-1])
        out = np.zeros(n, dtype=np.dtype(DOMAIN_FIELDS))
        env_off = np.zeros(n + 1, dtype=np.int64)
        pc, pp = C.c_void_p(None), C.c_void_p(None)
        if nq:
            check(lib().wh_domain_paths(self._h, residues.ctypes.data, offsets.ctypes.data, nq, flags.ctypes.data,
                                        C.addressof(detail), dom_off.ctypes.data, out.ctypes.data, env_off.ctypes.data,
                                        C.byref(pc), C.byref(pp)), "wh_domain_paths")
        total = int(env_off[-1])
        cols = self._take(pc, total, np.int32)
        post = self._take(pp, total, np.float32)
        return out, dom_off, env_off, cols, post

    @staticmethod
    def _take(ptr, n, dt):
        """A malloc'ed buffer of the library as a numpy array (copied; the buffer is released)."""
        nbytes = n * np.dtype(dt).itemsize
        out = np.frombuffer((C.c_char * nbytes).from_address(ptr.value), dtype=dt).copy() if nbytes and ptr.value else np.zeros(0, dtype=dt)
        if ptr.value:
            lib().wh_free_text(ptr)
        return out

    @staticmethod
    def hits_opts(Z, domZ, incE=0.01, incdomE=0.01) -> _lib.HitsOpts:
        return _lib.HitsOpts(float(Z), float(domZ), float(incE), float(incdomE))

    def _hits_collect(self, h, nrows, recs, W, ptrs):
        n = int(nrows.value)
        rec = self._take(recs, n * 4, np.int32).view(np.dtype(_lib.HIT_ROW_FIELDS)) if n else np.zeros(0, dtype=np.dtype(_lib.HIT_ROW_FIELDS))
        m = self._msa_collect(n, h, W, C.c_int64(0), ptrs)
        del m["pathless"]
        m["row_recs"] = rec
        return m

    def hits_msa(self, residues, offsets, text, flags, detail, Z, domZ, incE=0.01, incdomE=0.01, h=0, order=None, no_lds=False,
                 want_domains=False):
        """hmmsearch -A: hmmalign's alignment of every domain of model h that satisfies the inclusion thresholds
        (include/witch_hip.h: wh_hits_msa) - the envelopes are aligned (wh_domain_paths_dev), the included domains chosen,
        ordered, sliced to ali_i..ali_j and assembled on the device.  flags, detail: what score(want_detail=True) returned;
        text: the sequences' characters as given; order: the queries in output order (None: query order).  Returns msa()'s
        dict without "pathless" and with "row_recs": a structured array (query, index, ali_i, ali_j) per row.  want_domains:
        also "domains" and "dom_off", what domains() returns - from the same alignment of the envelopes."""
        residues = np.ascontiguousarray(residues, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        flags = np.ascontiguousarray(flags, dtype=np.uint8)
        if isinstance(text, str):
            text = text.encode()
        text = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text, dtype=np.uint8)
        nq = len(offsets) - 1
        if len(text) != len(residues) or (nq and int(offsets[-1]) != len(residues)):
            raise ValueError("hits_msa: residues, text and offsets disagree")
        if order is not None:
            order = np.ascontiguousarray(order, dtype=np.int32)
            if len(order) != nq:
                raise ValueError("hits_msa: order must name every query once")
        counts, _ = self.domain_counts(flags, detail)
        dom_off = np.zeros(nq * self.H + 1, dtype=np.int64)
        np.cumsum(counts.reshape(-1), out=dom_off[1:])
        dom = np.zeros(int(dom_off[-1]), dtype=np.dtype(DOMAIN_FIELDS))
        o = self.hits_opts(Z, domZ, incE, incdomE)
        W, _, ptrs = self._msa_outputs()
        nrows, recs = C.c_int64(0), C.c_void_p(None)
        check(lib().wh_hits_msa(self._h, residues.ctypes.data, offsets.ctypes.data, text.ctypes.data, nq, flags.ctypes.data,
                                C.addressof(detail) if nq else None, dom_off.ctypes.data, int(h), None if order is None else order.ctypes.data,
                                C.byref(o), _lib.WH_MSA_NO_LDS if no_lds else 0, dom.ctypes.data if len(dom) else None,
                                C.byref(nrows), C.byref(recs), C.byref(W), *[C.byref(p) for p in ptrs]), "wh_hits_msa")
        m = self._hits_collect(int(h), nrows, recs, W, ptrs)
        if want_domains:
            m["domains"], m["dom_off"] = dom, dom_off
        return m

    def hits_msa_t(self, text_t, offsets_t, flags_t, detail_t, dom_off_t, dom_t, env_off_t, cols_t, pp_t, Z, domZ, incE=0.01,
                   incdomE=0.01, h=0, order_t=None, no_lds=False):
        """The hit selection and the assembly alone (wh_hits_msa_dev) on torch tensors resident on the device: the scoring
        call's flags and detail records (a uint8 tensor), dom_off int64 [nq * H + 1], the wh_domain records (uint8 [n, 56]), the
        envelope CSR int64 [n + 1] with its columns int32 and posteriors float32, order_t int32 [nq] or None.  Returns what
        hits_msa returns (numpy arrays)."""
        nq = offsets_t.numel() - 1
        o = self.hits_opts(Z, domZ, incE, incdomE)
        W, _, ptrs = self._msa_outputs()
        nrows, recs = C.c_int64(0), C.c_void_p(None)
        check(lib().wh_hits_msa_dev(self._h, text_t.data_ptr(), offsets_t.data_ptr(), nq, flags_t.data_ptr(), detail_t.data_ptr(),
                                    dom_off_t.data_ptr(), dom_t.data_ptr(), env_off_t.data_ptr(), cols_t.data_ptr(), pp_t.data_ptr(),
                                    int(h), None if order_t is None else order_t.data_ptr(), C.byref(o),
                                    _lib.WH_MSA_NO_LDS if no_lds else 0, C.byref(nrows), C.byref(recs), C.byref(W),
                                    *[C.byref(p) for p in ptrs], self._stream()), "wh_hits_msa_dev")
        return self._hits_collect(int(h), nrows, recs, W, ptrs)

    def consensus_letters(self, h=0):
        """The consensus letters of model h as its file prints them (the CONS column), None where the header does not say
        "CONS yes" (include/witch_hip.h: wh_ehmm_consensus)."""
        out = C.create_string_buffer(int(self.M[h]) + 1)
        present = C.c_int32(0)
        check(lib().wh_ehmm_consensus(self._h, int(h), out, C.byref(present)), "wh_ehmm_consensus")
        return out.raw[:int(self.M[h])].decode("ascii") if present.value else None

    @staticmethod
    def _display_result(nsel, off, recs, lines):
        """(disp_off int64 [nsel + 1], records, four uint8 arrays) -> domain_display's dict."""
        return {"nsel": int(nsel), "disp_off": off, "recs": recs, "model": lines[0], "match": lines[1], "target": lines[2], "pp": lines[3]}

    @staticmethod
    def display_lines(disp, names, H=1):
        """domain_display's dict as {name: {domain index within its pair: (model, match, target, pp) as str}}."""
        out = {}
        off = disp["disp_off"]
        for r, rec in enumerate(disp["recs"]):
            a, b = int(off[r]), int(off[r + 1])
            out.setdefault(names[int(rec["query"])], {})[int(rec["index"])] = tuple(
                disp[k][a:b].tobytes().decode("ascii") for k in ("model", "match", "target", "pp"))
        return out

    def domain_display(self, residues, offsets, flags, detail, domE=10.0, domZ=None, h=0, want_domains=False):
        """hmmsearch's alignment display (include/witch_hip.h: wh_domain_display): the envelopes are aligned
        (wh_domain_paths_dev) and the four lines under "== domain N" - model consensus, match line, target, PP - of every
        reportable domain of model h are rendered on the device.  flags, detail: what score(want_detail=True) returned;
        domZ None: the number of reported pairs of model h.  Returns {"nsel", "disp_off" int64 [nsel + 1], "recs" (query,
        index) per selected domain, "model", "match", "target", "pp": uint8 arrays of disp_off[nsel] characters};
        want_domains: also "domains" and "dom_off", what domains() returns - from the same alignment of the envelopes."""
        residues = np.ascontiguousarray(residues, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        flags = np.ascontiguousarray(flags, dtype=np.uint8)
        nq = len(offsets) - 1
        if domZ is None:
            domZ = max(int((flags.reshape(nq, self.H)[:, int(h)] & 1).sum()), 1) if nq else 1
        counts, _ = self.domain_counts(flags, detail)
        dom_off = np.zeros(nq * self.H + 1, dtype=np.int64)
        np.cumsum(counts.reshape(-1), out=dom_off[1:])
        dom = np.zeros(int(dom_off[-1]), dtype=np.dtype(DOMAIN_FIELDS))
        nsel = C.c_int64(0)
        ptrs = [C.c_void_p(None) for _ in range(6)]
        check(lib().wh_domain_display(self._h, residues.ctypes.data, offsets.ctypes.data, nq, flags.ctypes.data,
                                      C.addressof(detail) if nq else None, dom_off.ctypes.data, int(h), float(domE), float(domZ),
                                      dom.ctypes.data if len(dom) else None, C.byref(nsel), *[C.byref(p) for p in ptrs]), "wh_domain_display")
        n = int(nsel.value)
        off = self._take(ptrs[0], n + 1, np.int64) if n else np.zeros(1, dtype=np.int64)
        recs = self._take(ptrs[1], 2 * n, np.int32).view(np.dtype(_lib.DISPLAY_REC_FIELDS))
        total = int(off[-1])
        m = self._display_result(n, off, recs, [self._take(p, total, np.uint8) for p in ptrs[2:]])
        if want_domains:
            m["domains"], m["dom_off"] = dom, dom_off
        return m

    def sequence_model_posteriors(self, residues, offsets, recs, env_off, cols, pp, h=0):
        """The posteriors hmmsearch prints in a domain's PP line, for the domains of model h among the records of
        domain_paths(): hmmsearch decodes an envelope under the unihit length model of the WHOLE sequence's L residues, where
        domain_paths (hmmalign on the envelope alone: wh_align_pp) uses the envelope's own Ld.  The same kernels give the
        former exactly when the envelope is followed by L - Ld residues that no match state can emit (the alphabet's gap
        code: match odds 0): they can only sit in the C flank, where each multiplies EVERY path by the same loop
        probability, which cancels in a posterior, and the length model is that of Ld + (L - Ld) = L residues.  One
        wh_align_pp call on the padded envelopes whose sequence is longer than they are; a residue takes the new posterior
        where that alignment puts it in the state the domain's own path has (everywhere, on the fixtures' strong domains),
        else it keeps the old one.  Returns a copy of pp with those values replaced."""
        residues = np.ascontiguousarray(residues, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        out = np.array(pp, dtype=np.float32, copy=True)
        gap = 20 if self.alphabet == _lib.ALPH_AMINO else 4
        q = recs["pair"] // self.H
        L = offsets[q + 1] - offsets[q]
        Ld = (recs["env_j"] - recs["env_i"] + 1).astype(np.int64)
        pick = np.nonzero((recs["pair"] % self.H == int(h)) & (recs["ali_i"] != 0) & (L > Ld))[0]
        if len(pick) == 0:
            return out
        parts = []
        for d in pick:
            a = int(offsets[q[d]]) + int(recs["env_i"][d]) - 1
            parts.append(residues[a:a + int(Ld[d])])
            parts.append(np.full(int(L[d] - Ld[d]), gap, dtype=np.uint8))
        poffs = np.zeros(len(pick) + 1, dtype=np.int64)
        np.cumsum(L[pick], out=poffs[1:])
        cols2, co, pp2 = self.align(np.concatenate(parts), poffs, np.arange(len(pick)), np.full(len(pick), int(h), dtype=np.int32), want_pp=True)
        for i, d in enumerate(pick):
            a, b, n = int(env_off[d]), int(co[i]), int(Ld[d])
            same = (cols2[b:b + n] == cols[a:a + n]) & np.isfinite(pp2[b:b + n])
            out[a:a + n][same] = pp2[b:b + n][same]
        return out

    def domain_paths_t(self, residues_t, offsets_t, max_len: int, flags_t, detail_t):
        """domain_paths() on torch tensors resident on the device (wh_domain_counts_dev, wh_domain_paths_dev): (records as
        a uint8 tensor [n, 56], dom_off int64 [nq * H + 1], env_off int64 [n + 1], cols int32, pp float32).  The last three
        are DevView's of the handle's workspace (data_ptr(), numel()), valid until the next domains, domain_paths or hits_msa
        call on the handle: what hits_msa_t and domain_display_t take."""
        import torch
        nq = offsets_t.numel() - 1
        dev = residues_t.device
        counts = torch.empty((nq, self.H), dtype=torch.int32, device=dev)
        dom_off = torch.zeros(nq * self.H + 1, dtype=torch.int64, device=dev)
        if nq:
            check(lib().wh_domain_counts_dev(self._h, flags_t.data_ptr(), detail_t.data_ptr(), nq, counts.data_ptr(), None, self._stream()),
                  "wh_domain_counts_dev")
            dom_off[1:] = torch.cumsum(counts.reshape(-1), 0)
        n = int(dom_off[-1].item())
        out = torch.zeros((n, np.dtype(DOMAIN_FIELDS).itemsize), dtype=torch.uint8, device=dev)
        p_env, p_cols, p_pp, total = C.c_void_p(None), C.c_void_p(None), C.c_void_p(None), C.c_int64(0)
        if nq:
            check(lib().wh_domain_paths_dev(self._h, residues_t.data_ptr(), offsets_t.data_ptr(), nq, residues_t.numel(), int(max_len),
                                            flags_t.data_ptr(), detail_t.data_ptr(), dom_off.data_ptr(), out.data_ptr(), C.byref(p_env),
                                            C.byref(p_cols), C.byref(p_pp), C.byref(total), self._stream()), "wh_domain_paths_dev")
        t = int(total.value)
        return out, dom_off, DevView(p_env.value, n + 1), DevView(p_cols.value, t), DevView(p_pp.value, t)

    def domain_display_t(self, residues_t, offsets_t, flags_t, dom_off_t, dom_t, env_off_t, cols_t, pp_t, domE=10.0, domZ=1.0, h=0,
                         cap=None, poison=None):
        """The display stage alone (wh_domain_display_dev) on torch tensors resident on the device: the scoring call's residues,
        offsets and flags, dom_off int64 [nq * H + 1], the wh_domain records (uint8 [n, 56]), the envelope CSR int64 [n + 1]
        with its columns int32 and posteriors float32.  cap: bytes of each line array (default: n x M + the envelope
        residues, which always suffices).  Returns domain_display's dict (numpy arrays); with poison (a byte value the output
        arrays are filled with before the call) also "raw": the four whole arrays, disp_off and the records as numpy, for a
        caller that checks what was NOT written."""
        import torch
        nq = offsets_t.numel() - 1
        n = int(dom_t.shape[0])
        dev = offsets_t.device
        cap = n * (int(self.M[h]) if 0 <= int(h) < self.H else 0) + int(cols_t.numel()) if cap is None else int(cap)
        fill = 0 if poison is None else int(poison)
        off = torch.full((n + 1,), -1 if poison is not None else 0, dtype=torch.int64, device=dev)
        recs = torch.full((max(n, 1), 8), fill, dtype=torch.uint8, device=dev)
        lines = torch.full((4, max(cap, 1)), fill, dtype=torch.uint8, device=dev)
        nsel, total = C.c_int64(0), C.c_int64(0)
        check(lib().wh_domain_display_dev(self._h, residues_t.data_ptr(), offsets_t.data_ptr(), nq, flags_t.data_ptr(), dom_off_t.data_ptr(),
                                          dom_t.data_ptr(), env_off_t.data_ptr(), cols_t.data_ptr(), pp_t.data_ptr(), int(h), float(domE),
                                          float(domZ), cap, off.data_ptr(), recs.data_ptr(), lines[0].data_ptr(), lines[1].data_ptr(),
                                          lines[2].data_ptr(), lines[3].data_ptr(), C.byref(nsel), C.byref(total), self._stream()),
              "wh_domain_display_dev")
        torch.cuda.current_stream().synchronize()
        ns, tot = int(nsel.value), int(total.value)
        keep = slice(None) if poison is not None else slice(0, tot)      # (the whole arrays only for a caller that inspects them)
        h_off, h_recs, h_lines = off.cpu().numpy(), recs.cpu().numpy(), lines[:, keep].cpu().numpy()
        m = self._display_result(ns, h_off[:ns + 1].copy(), h_recs[:ns].reshape(-1).view(np.dtype(_lib.DISPLAY_REC_FIELDS)).copy(),
                                 [h_lines[t, :tot].copy() for t in range(4)])
        m["total"] = tot
        if poison is not None:
            m["raw"] = {"disp_off": h_off, "recs": h_recs, "lines": h_lines, "cap": cap}
        return m

    def last_align_status(self):
        """(pairs redone in log space, pair numbers the last align call returned UNALIGNED - all columns -1 -
        because the any-size kernel could not align them; include/witch_hip.h: wh_last_align_status)."""
        nlog, nun = C.c_int64(0), C.c_int64(0)
        check(lib().wh_last_align_status(self._h, C.byref(nlog), C.byref(nun), None, 0), "wh_last_align_status")
        pairs = np.zeros(nun.value, dtype=np.int64)
        if nun.value:
            check(lib().wh_last_align_status(self._h, None, None, pairs.ctypes.data, nun.value), "wh_last_align_status")
        return int(nlog.value), pairs

    def last_align_paths(self):
        """Pairs of the last align call by sweep path: {"window256", "window512", "window_rejected", "full_width"}
        (include/witch_hip.h: wh_last_align_paths)."""
        p4 = np.zeros(4, dtype=np.int64)
        check(lib().wh_last_align_paths(self._h, p4.ctypes.data), "wh_last_align_paths")
        return {"window256": int(p4[0]), "window512": int(p4[3]), "window_rejected": int(p4[1]), "full_width": int(p4[2])}

    def consensus(self, offsets, qpair_off, pair_h, pair_w, col_offsets, cols, retained, nongaps, backbone_length):
        """Weighted consensus DP (wh_consensus).  retained / nongaps: one int array per model."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        qpair_off = np.ascontiguousarray(qpair_off, dtype=np.int64)
        pair_h = np.ascontiguousarray(pair_h, dtype=np.int32)
        pair_w = np.ascontiguousarray(pair_w, dtype=np.float64)
        col_offsets = np.ascontiguousarray(col_offsets, dtype=np.int64)
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        ro = np.zeros(self.H + 1, dtype=np.int64)
        ro[1:] = np.cumsum([len(r) for r in retained])
        ret = np.ascontiguousarray(np.concatenate(retained), dtype=np.int32)
        ng = np.ascontiguousarray(np.concatenate(nongaps), dtype=np.int32)
        nq = len(offsets) - 1
        out = np.zeros(int(offsets[-1]), dtype=np.int32)
        mm = np.zeros(2 * nq, dtype=np.int32)
        check(lib().wh_consensus(self._h, offsets.ctypes.data, nq, qpair_off.ctypes.data, pair_h.ctypes.data,
                                 pair_w.ctypes.data, col_offsets.ctypes.data, cols.ctypes.data, ro.ctypes.data,
                                 ret.ctypes.data, ng.ctypes.data, int(backbone_length), out.ctypes.data,
                                 mm.ctypes.data), "wh_consensus")
        return out, mm.reshape(nq, 2)

    # ------------------------------------------------------------------ device (torch) operators
    @staticmethod
    def _stream():
        import torch
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def label_to_pos_t(self, labels_t):
        """hmm_index labels (as returned by topk_t) -> model positions 0..H-1, on the device."""
        import torch
        lut = getattr(self, "_lut_t", None)
        if lut is None or lut.device != labels_t.device:
            lut = torch.full((int(self.index.max()) + 1,), -1, dtype=torch.int32, device=labels_t.device)
            lut[torch.from_numpy(self.index.astype(np.int64)).to(labels_t.device)] = torch.arange(
                self.H, dtype=torch.int32, device=labels_t.device)
            self._lut_t = lut
        return lut[labels_t.long()].contiguous()

    def score_t(self, residues_t, offsets_t, max_len: int, want_fwd=False):
        import torch
        nq = offsets_t.numel() - 1
        dev = residues_t.device
        deci = torch.empty((nq, self.H), dtype=torch.int32, device=dev)
        flags = torch.empty((nq, self.H), dtype=torch.uint8, device=dev)
        fwd = torch.empty((nq, self.H), dtype=torch.float32, device=dev) if want_fwd else None
        check(lib().wh_score_dev(self._h, residues_t.data_ptr(), offsets_t.data_ptr(), nq, residues_t.numel(),
                                 int(max_len), deci.data_ptr(), flags.data_ptr(),
                                 None if fwd is None else fwd.data_ptr(), None, self._stream()), "wh_score_dev")
        return (deci, flags, fwd) if want_fwd else (deci, flags)

    def topk_t(self, deci_t, flags_t, k: int):
        import torch
        nq = deci_t.shape[0]
        dev = deci_t.device
        idx = torch.empty((nq, k), dtype=torch.int32, device=dev)
        w = torch.empty((nq, k), dtype=torch.float64, device=dev)
        nk = torch.empty(nq, dtype=torch.int32, device=dev)
        nu = torch.empty(nq, dtype=torch.int32, device=dev)
        check(lib().wh_topk_dev(self._h, deci_t.data_ptr(), flags_t.data_ptr(), nq, int(k), idx.data_ptr(),
                                w.data_ptr(), nk.data_ptr(), nu.data_ptr(), self._stream()), "wh_topk_dev")
        return idx, w, nk, nu

    def align_t(self, residues_t, offsets_t, max_len: int, pair_q_t, pair_h_t, col_offsets_t, total_cols: int,
                want_pp=False, cfg_len_t=None, use_len=False):
        """cols on the device; with want_pp (cols, pp) - pp float32, CSR like cols (wh_align_pp_dev).  cfg_len_t (int32 per
        query) or use_len: through wh_align_pp_len_dev, with that array or a null one."""
        import torch
        cols = torch.full((int(total_cols),), -1, dtype=torch.int32, device=residues_t.device)
        pp = torch.zeros((int(total_cols),), dtype=torch.float32, device=residues_t.device) if want_pp else None
        npairs = pair_q_t.numel()
        if npairs and (cfg_len_t is not None or use_len):
            check(lib().wh_align_pp_len_dev(self._h, residues_t.data_ptr(), offsets_t.data_ptr(), offsets_t.numel() - 1,
                                            residues_t.numel(), int(max_len), pair_q_t.data_ptr(), pair_h_t.data_ptr(),
                                            npairs, col_offsets_t.data_ptr(), cols.data_ptr(), pp.data_ptr() if want_pp else None,
                                            cfg_len_t.data_ptr() if cfg_len_t is not None else None, self._stream()), "wh_align_pp_len_dev")
        elif npairs and not want_pp:
            check(lib().wh_align_dev(self._h, residues_t.data_ptr(), offsets_t.data_ptr(), offsets_t.numel() - 1,
                                     residues_t.numel(), int(max_len), pair_q_t.data_ptr(), pair_h_t.data_ptr(),
                                     npairs, col_offsets_t.data_ptr(), cols.data_ptr(), self._stream()),
                  "wh_align_dev")
        elif npairs:
            check(lib().wh_align_pp_dev(self._h, residues_t.data_ptr(), offsets_t.data_ptr(), offsets_t.numel() - 1,
                                        residues_t.numel(), int(max_len), pair_q_t.data_ptr(), pair_h_t.data_ptr(),
                                        npairs, col_offsets_t.data_ptr(), cols.data_ptr(), pp.data_ptr(),
                                        self._stream()), "wh_align_pp_dev")
        return (cols, pp) if want_pp else cols

    def msa_t(self, cols_t, pp_t, text_t, offsets_t, h=0, trim=False, no_lds=False, mapali_t=None):
        """The assembly alone (wh_msa_dev) on torch tensors resident on the device: cols int32 and pp float32 as
        align_t(want_pp=True) returns them for the pairs (q, h), text uint8, offsets int64 [nq + 1].  Returns what msa
        returns (numpy arrays: the library hands the alignment back in host memory).  mapali_t: a uint8 tensor
        [n_map, alen] on the device, the rows of the alignment the model was built from (wh_msa_mapali_dev; the checksum is
        the caller's to verify: witch_amd.ehmm.alignment_checksum against cksum())."""
        nq = offsets_t.numel() - 1
        W, npl, ptrs = self._msa_outputs()
        flags = (_lib.WH_MSA_TRIM if trim else 0) | (_lib.WH_MSA_NO_LDS if no_lds else 0)
        if mapali_t is not None:
            n_map, alen = int(mapali_t.shape[0]), int(mapali_t.shape[1])
            mapali_t = mapali_t.contiguous()
            check(lib().wh_msa_mapali_dev(self._h, cols_t.data_ptr(), pp_t.data_ptr(), text_t.data_ptr(), offsets_t.data_ptr(), nq,
                                          int(cols_t.numel()), int(h), flags, mapali_t.data_ptr(), n_map, alen, C.byref(W),
                                          *[C.byref(p) for p in ptrs], C.byref(npl), self._stream()), "wh_msa_mapali_dev")
            return self._msa_collect(nq, int(h), W, npl, ptrs, n_map=n_map)
        check(lib().wh_msa_dev(self._h, cols_t.data_ptr(), pp_t.data_ptr(), text_t.data_ptr(), offsets_t.data_ptr(), nq,
                               int(cols_t.numel()), int(h), flags, C.byref(W), *[C.byref(p) for p in ptrs], C.byref(npl),
                               self._stream()), "wh_msa_dev")
        return self._msa_collect(nq, int(h), W, npl, ptrs)

    def seq_expect_t(self, residues_t, offsets_t, max_len: int, pairs_t):
        """seq_expect() on torch tensors resident on the device (wh_seq_expect_dev on torch's current stream): a uint8
        tensor [n, 12], the (exp, reg, clu) records - view it on the host with numpy's SEQ_EXPECT_FIELDS dtype."""
        import torch
        n = int(pairs_t.numel())
        out = torch.zeros((n, 12), dtype=torch.uint8, device=residues_t.device)
        check(lib().wh_seq_expect_dev(self._h, residues_t.data_ptr(), offsets_t.data_ptr(), offsets_t.numel() - 1, residues_t.numel(),
                                      int(max_len), pairs_t.data_ptr(), n, out.data_ptr(), self._stream()), "wh_seq_expect_dev")
        return out

    def seq_table_t(self, residues_t, offsets_t, max_len: int, flags_t, detail_t, cap=None, Z=None, domZ=None, E=10.0, domE=10.0,
                    incE=0.01, incdomE=0.01):
        """seq_table() on torch tensors resident on the device (wh_seq_table_dev): detail_t as for domains_dev.  Returns the
        rows as a uint8 tensor [n, 80] (numpy's SEQ_ROW_FIELDS dtype).  cap: room for so many rows (default: every pair)."""
        import torch
        nq = offsets_t.numel() - 1
        cap = nq * self.H if cap is None else int(cap)
        out = torch.zeros((cap, 80), dtype=torch.uint8, device=residues_t.device)
        o = seq_table_opts(Z, domZ, E, domE, incE, incdomE)
        n = lib().wh_seq_table_dev(self._h, residues_t.data_ptr(), offsets_t.data_ptr(), nq, residues_t.numel(), int(max_len),
                                   flags_t.data_ptr(), detail_t.data_ptr(), C.byref(o), out.data_ptr(), cap, self._stream())
        check(min(n, 0), "wh_seq_table_dev")
        return out[:n]

    def domains_dev(self, residues_t, offsets_t, max_len: int, flags_t, detail_t):
        """domains() on torch tensors resident on the device (wh_domain_counts_dev, wh_domains_dev on torch's current
        stream): detail_t is a uint8 tensor holding the nq * H wh_pair_detail records of wh_score_dev.  Returns (records as
        a uint8 tensor [n, 56] - view it on the host with numpy's DOMAIN_FIELDS dtype -, dom_off int64 [nq * H + 1],
        n_unlisted int32 [nq, H])."""
        import torch
        nq = offsets_t.numel() - 1
        dev = residues_t.device
        counts = torch.empty((nq, self.H), dtype=torch.int32, device=dev)
        unl = torch.empty((nq, self.H), dtype=torch.int32, device=dev)
        dom_off = torch.zeros(nq * self.H + 1, dtype=torch.int64, device=dev)
        if nq:
            check(lib().wh_domain_counts_dev(self._h, flags_t.data_ptr(), detail_t.data_ptr(), nq, counts.data_ptr(),
                                             unl.data_ptr(), self._stream()), "wh_domain_counts_dev")
            dom_off[1:] = torch.cumsum(counts.reshape(-1), 0)
        n = int(dom_off[-1].item())
        out = torch.zeros((n, np.dtype(DOMAIN_FIELDS).itemsize), dtype=torch.uint8, device=dev)
        if nq:
            check(lib().wh_domains_dev(self._h, residues_t.data_ptr(), offsets_t.data_ptr(), nq, residues_t.numel(),
                                       int(max_len), flags_t.data_ptr(), detail_t.data_ptr(), dom_off.data_ptr(),
                                       out.data_ptr(), self._stream()), "wh_domains_dev")
        return out, dom_off, unl

    def consensus_t(self, offsets_t, max_len: int, qpair_off_t, pair_h_t, pair_w_t, col_offsets_t, cols_t,
                    ret_off_t, retained_t, nongaps_t, backbone_length: int, max_pairs_per_query: int):
        """Weighted consensus DP on device-resident inputs (wh_consensus_dev): per residue the backbone
        column or -1 - (column before which the insertion sits), and (min, max) touched column per query."""
        import torch
        nq = offsets_t.numel() - 1
        dev = offsets_t.device
        out = torch.empty(int(cols_t.numel() and offsets_t[-1].item()), dtype=torch.int32, device=dev)
        mm = torch.empty((nq, 2), dtype=torch.int32, device=dev)
        check(lib().wh_consensus_dev(self._h, offsets_t.data_ptr(), nq, int(max_len), qpair_off_t.data_ptr(),
                                     pair_h_t.data_ptr(), pair_w_t.data_ptr(), col_offsets_t.data_ptr(),
                                     cols_t.data_ptr(), ret_off_t.data_ptr(), retained_t.data_ptr(),
                                     nongaps_t.data_ptr(), int(backbone_length), int(max_pairs_per_query),
                                     out.data_ptr(), mm.data_ptr(), self._stream()), "wh_consensus_dev")
        return out, mm
