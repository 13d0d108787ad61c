"""Resident GPU server behind the level-0 hmmsearch / hmmalign executables (see __init__.py).

    python -m witch_amd.shim.server --socket /tmp/witch_hip.sock [--device 0] [--daemonize]

Protocol (one request per connection): the client sends  tool \\0 cwd \\0 arg \\0 arg ... and shuts
its write side; the server answers "<exit status>\\n<message>".  Requests are served by one
thread per connection; GPU work is serialised, and hmmalign requests that arrive together (WITCH
issues them from up to num_cpus workers at once) are batched into ONE wh_align launch.
"""
import argparse
import os
import socket
import sys
import threading
import time

import numpy as np

from . import formats


def default_socket_path():
    """$WITCH_HIP_SOCKET, else a socket inside a directory only this user can enter
    ($XDG_RUNTIME_DIR/witch_hip or /tmp/witch_hip_<uid>, mode 0700; client.c uses the same rule)."""
    if os.environ.get("WITCH_HIP_SOCKET"):
        return os.environ["WITCH_HIP_SOCKET"]
    base = os.environ.get("XDG_RUNTIME_DIR")
    d = os.path.join(base, "witch_hip") if base else "/tmp/witch_hip_%d" % os.getuid()
    return os.path.join(d, "server.sock")


def private_socket_dir(sock_path):
    """Create the socket's directory 0700 and refuse one that somebody else owns or can write to."""
    d = os.path.dirname(os.path.abspath(sock_path))
    os.makedirs(d, mode=0o700, exist_ok=True)
    st = os.stat(d)
    if d.startswith("/tmp/witch_hip_") or d.endswith("/witch_hip"):
        if st.st_uid != os.getuid() or (st.st_mode & 0o077):
            raise PermissionError("socket directory %s is not private to uid %d" % (d, os.getuid()))
    return d


class ArgError(Exception):
    pass


def parse_hmmsearch_argv(argv):
    """The options WITCH passes (algorithm.py:526-532) plus the ones that take a value in HMMER,
    so that positional arguments are found; unknown flags are ignored like a no-op."""
    takes_value = {"-o", "-A", "-E", "-T", "-Z", "--cpu", "--tblout", "--domtblout", "--pfamtblout", "--domE", "--domT",
                   "--incE", "--incT", "--incdomE", "--incdomT", "--F1", "--F2", "--F3", "--domZ", "--seed", "--tformat",
                   "--textw"}
    opts, pos, i = {}, [], 0
    while i < len(argv):
        a = argv[i]
        if a in takes_value:
            if i + 1 >= len(argv):
                raise ArgError("option %s needs a value" % a)
            opts[a] = argv[i + 1]
            i += 2
        elif a.startswith("-") and a != "-":
            opts[a] = True
            i += 1
        else:
            pos.append(a)
            i += 1
    if len(pos) != 2:
        raise ArgError("Incorrect number of command line arguments.\nUsage: hmmsearch [options] <hmmfile> <seqdb>")
    return opts, pos[0], pos[1]


HMMER_F = (0.02, 1e-3, 1e-5)      # hmmsearch's default --F1 --F2 --F3


def filter_thresholds(opts):
    """None for a search with --max (--F1 --F2 --F3 --nobias are then ignored, as in HMMER), else (F1, F2, F3)."""
    if "--max" in opts:
        return None
    F = []
    for o, d in zip(("--F1", "--F2", "--F3"), HMMER_F):
        try:
            F.append(float(opts.get(o, d)))
        except ValueError:
            raise ArgError("witch-hip hmmsearch shim: bad value for %s" % o)
        if not F[-1] >= 0:
            raise ArgError("witch-hip hmmsearch shim: bad value for %s" % o)
    return tuple(F)


def bias_filter_enabled():
    """WITCH_HIP_BIAS_FILTER=1 in the server's environment: HMMER's bias filter runs for a filtered search without
    --nobias (WITCH's own filtered command line).  An opt-in for now; it becomes the default later."""
    return os.environ.get("WITCH_HIP_BIAS_FILTER", "") == "1"


def alidisplay_enabled():
    """WITCH_HIP_ALIDISPLAY=1 in the server's environment: a line without --noali gets hmmsearch's alignment display (the
    four lines under "== domain N" of every reported domain, rendered on the GPU: wh_domain_display).  An opt-in for now, as
    the bias filter is; it becomes the default later.  Unset, every line is answered as with --noali."""
    return os.environ.get("WITCH_HIP_ALIDISPLAY", "") == "1"


def domain_seqlen_enabled():
    """WITCH_HIP_DOMAIN_SEQLEN=1 in the server's environment: the domain stage aligns every envelope under the length model of
    its whole sequence, as hmmsearch does (EHMM.set_domain_length_model("sequence")): --domtblout, the domain tables, -A and
    the alignment display then show hmmsearch's own alignment, and the display needs no second alignment launch for its PP
    line.  An opt-in for now, as the bias filter and the display are.  Unset, every output is what it was."""
    return os.environ.get("WITCH_HIP_DOMAIN_SEQLEN", "") == "1"


def display_textw(opts):
    """The text width of the alignment display: --textw N (HMMER refuses N < 120, so does this), --notextw: None (one
    block), else 120."""
    if "--notextw" in opts:
        return None
    if "--textw" not in opts:
        return 120
    try:
        w = int(opts["--textw"])
    except ValueError:
        raise ArgError("Failed to parse command line: option --textw takes integer arg; got %s" % opts["--textw"])
    if w < 120:
        raise ArgError("Failed to parse command line: option --textw takes integer arg in range n>=120; got %s on cmdline" % opts["--textw"])
    return w


def check_hmmsearch_options(opts):
    """The GPU path computes what WITCH's own command lines ask for (algorithm.py:526-532): a reporting threshold that
    lets every hit through, and either `--max` (no filters) or the filtered search of WITCH's `filters` switch - the MSV,
    Viterbi and Forward stages at --F1 --F2 --F3 (HMMER's defaults 0.02, 1e-3, 1e-5; wh_score_filtered).  ONE gap remains:
    the bias filter is not implemented, so a filtered search must say --nobias; plain filtered search (no --max, no
    --nobias) is refused with a message that says exactly this - unless the server's environment has
    WITCH_HIP_BIAS_FILTER=1: the bias filter then runs (bias_filter_enabled).  With --max the four options are ignored, as in HMMER.
    Anything else that would change the reported set in HMMER (a real E-value / score cut-off, no null2) is refused
    with exit status 1 instead of being silently ignored.
    --domtblout FILE is written (per-domain records of wh_domains; --domE, -Z and --domZ apply to it and to the
    domain tables of the main output, whose '!' / '?' marks follow --incE and --incdomE; without --domtblout none of
    these five is read - -Z and --domZ are then not even checked, as before).
    -A FILE is written too: the alignment of every domain that satisfies the inclusion thresholds (wh_hits_msa: --incE,
    --incdomE, -Z and --domZ are read and checked for it as for --domtblout; --notextw: one block), and the main output
    says so behind "//"; a backend without search_hits refuses the option by name.
    --tblout FILE is written as well: the per-sequence table of wh_seq_table, alone or together with --domtblout and -A
    (-Z, --domZ, -E, --domE, --incE and --incdomE are read and checked for it as for --domtblout); a backend without
    search_table refuses the option by name.
    The alignment display - what hmmsearch prints by default under every domain table - is written where the server's
    environment has WITCH_HIP_ALIDISPLAY=1 and the line has no --noali (alidisplay_enabled; --textw N and --notextw apply,
    --domE, -Z and --domZ are read and checked for it as for --domtblout; a backend without search_display refuses such a
    line by name; a model with "RF yes", "CS yes" or without "CONS yes" is refused by the library).  Without the variable the
    display stays a no-op: the output is that of --noali, as before."""
    if "--max" not in opts and "--nobias" not in opts and not bias_filter_enabled():
        raise ArgError("witch-hip hmmsearch shim: the filtered search is implemented without HMMER's bias filter only: "
                       "pass --nobias (MSV, Viterbi and Forward filters at --F1 --F2 --F3), or --max (no filters; "
                       "WITCH passes --max unless its filters are switched on)")
    filter_thresholds(opts)
    for o in ("-T", "--incT", "--domT", "--incdomT", "--nonull2", "--cut_ga", "--cut_nc", "--cut_tc"):
        if o in opts:
            raise ArgError("witch-hip hmmsearch shim: option %s is not supported" % o)
    for o in ("-E", "--incE", "--domE", "--incdomE"):
        if o in opts:
            try:
                v = float(opts[o])
            except ValueError:
                raise ArgError("witch-hip hmmsearch shim: bad value for %s" % o)
            if o == "--domE" and not v >= 0:
                raise ArgError("witch-hip hmmsearch shim: bad value for %s" % o)
            if o in ("--incE", "--incdomE") and ("-A" in opts or "--tblout" in opts) and not v >= 0:
                raise ArgError("witch-hip hmmsearch shim: bad value for %s" % o)
            if o == "-E" and v < 1e6:
                raise ArgError("witch-hip hmmsearch shim: -E %s would drop hits; only E >= 1e6 (WITCH: 99999999) "
                               "is supported, every sequence with a domain is reported" % opts[o])
    shown = alidisplay_enabled() and "--noali" not in opts
    if shown:
        display_textw(opts)
    for o in (("-Z", "--domZ") if "--domtblout" in opts or "-A" in opts or "--tblout" in opts or shown else ()):      # (read only for the per-domain output, -A and --tblout; else ignored as before)
        if o in opts:
            try:
                ok = float(opts[o]) > 0
            except ValueError:
                ok = False
            if not ok:
                raise ArgError("witch-hip hmmsearch shim: bad value for %s" % o)


class MapaliMismatch(Exception):
    """The --mapali alignment is not the one the model was built from (its checksum is not the model's CKSUM)."""


def parse_hmmalign_argv(argv):
    takes_value = {"-o", "--mapali", "--informat", "--outformat"}
    opts, pos, i = {}, [], 0
    while i < len(argv):
        a = argv[i]
        if a in takes_value:
            if i + 1 >= len(argv):
                raise ArgError("option %s needs a value" % a)
            opts[a] = argv[i + 1]
            i += 2
        elif a.startswith("-") and a != "-":
            opts[a] = True
            i += 1
        else:
            pos.append(a)
            i += 1
    if len(pos) != 2:
        raise ArgError("Incorrect number of command line arguments.\nUsage: hmmalign [-options] <hmmfile> <seqfile>")
    return opts, pos[0], pos[1]


class GpuBackend:
    """The only place that touches libwitch_hip.so.  One single-model EHMM per HMM file
    (hmmsearch works one model at a time; hmmalign batches are grouped by model)."""

    def __init__(self, device=0, max_models=None):
        import collections
        self.device = device
        # realpath -> (mtime, EHMM, header), least recently used first.  Every handle owns device
        # workspace (hundreds of MB once it has scored a chunk) and a WITCH ensemble has hundreds of
        # models, so the cache is bounded and evicted handles are closed.
        self.cache = collections.OrderedDict()
        self.max_models = max_models or int(os.environ.get("WITCH_HIP_MAX_MODELS", "32"))
        self.lock = threading.Lock()
        self.seqlen = domain_seqlen_enabled()      # read once, like the handles' own environment
        self.calls = []                            # the EHMM stages of the last search, in call order (tests)

    def model(self, path):
        from witch_amd.ehmm import EHMM
        rp = os.path.realpath(path)
        mt = os.stat(rp).st_mtime
        hit = self.cache.get(rp)
        if hit is None or hit[0] != mt:
            if hit is not None:
                hit[1].close()
                del self.cache[rp]
            while len(self.cache) >= self.max_models:
                _, (_, old, _) = self.cache.popitem(last=False)
                old.close()
            hit = (mt, EHMM([rp], device=self.device), formats.hmm_header(rp))
            if self.seqlen:
                hit[1].set_domain_length_model("sequence")
            self.cache[rp] = hit
        else:
            self.cache.move_to_end(rp)
        return hit[1], hit[2]

    def search(self, hmm_path, records, want_domains=False, filters=None, bias=False):
        """records: [(name, text)] -> (header, [(name, bits, bias_bits, n_domains)] of reported sequences); with
        want_domains also {name: [domain records]}: the fields of wh_domain (EHMM.domains) and the envelope's envsc.
        The domains cost an alignment per envelope: only a caller that prints them asks for them.
        filters=(F1, F2, F3): behind hmmsearch's acceleration filters (without the bias filter: --nobias); the stage
        counts of the search are then in self.last_passed (n MSV, n bias, n Vit, n Fwd).  bias=True: with the bias filter."""
        hdr, rows, domains = self._search(hmm_path, records, want_domains, filters, None, bias)[:3]
        return (hdr, rows, domains) if want_domains else (hdr, rows)

    def search_hits(self, hmm_path, records, inc, want_domains=False, filters=None, bias=False):
        """search() for hmmsearch -A: (header, rows, domains or None, hits) - hits is EHMM.hits_msa's dict, the alignment of
        every domain that satisfies the inclusion thresholds, its rows in HMMER's hit order (formats.hit_order) and domain
        order.  inc: {"incE", "incdomE", "Z", "domZ"} (Z / domZ None: the number of targets / of reported sequences).  The
        rows carry the unrounded score as the tables of --domtblout do.  With want_domains the domain records come from the
        same alignment of the envelopes (wh_hits_msa hands them back): one domain stage serves --domtblout and -A."""
        return self._search(hmm_path, records, want_domains, filters, inc, bias)[:4]

    def search_table(self, hmm_path, records, table, want_domains=False, filters=None, bias=False, inc=None):
        """search() for hmmsearch --tblout: (header, rows, domains or None, hits or None, table rows) from ONE scoring call.
        table: {"Z", "domZ", "E", "domE", "incE", "incdomE"} (Z / domZ None: the number of targets / of reported sequences);
        the table rows are EHMM.seq_table's records (wh_seq_table).  inc: as for search_hits, when -A is asked for as well.
        The rows carry the unrounded score, as for --domtblout."""
        return self._search(hmm_path, records, want_domains, filters, inc, bias, table)

    def search_display(self, hmm_path, records, display, inc=None, table=None, filters=None, bias=False):
        """search() for a line that shows the alignments: (header, rows, domains, hits or None, table rows or None, lines).
        display: {"domE", "domZ"} (domZ None: the number of reported sequences); lines: {name: {domain index: (model, match
        line, target, PP)}} of the reportable domains (EHMM.display_lines).  inc / table: as for search_hits / search_table,
        when -A / --tblout are asked for on the same line.  There is ONE domain stage (wh_domain_paths_dev): the domain
        records, the display and the rows of -A all come from that one domain stage."""
        return self._search(hmm_path, records, True, filters, inc, bias, table, display)

    def _search(self, hmm_path, records, want_domains, filters, inc, bias=False, table=None, display=None):
        from witch_amd.ehmm import pack_queries
        domains, hits, tbl, lines = {}, None, None, None
        with self.lock:
            e, hdr = self.model(hmm_path)
            seqs = [e.digitize(t.upper()) for _, t in records]     # alignment_tools.py:730-731 upper-cases
            res, offs = pack_queries(seqs)
            if filters is None:
                deci, flags, det = e.score(res, offs, want_detail=True)
            else:
                deci, flags, det = e.score(res, offs, want_detail=True, filters=filters, nobias=not bias, bias=bias)
                c = e.last_filter_counts()
                self.last_passed = (c["msv"], c["bias"], c["vit"], c["fwd"])
            exact = want_domains or inc is not None or table is not None
            rows = []
            for i, (name, _) in enumerate(records):
                if flags[i, 0] & 1:
                    d = det[i]
                    bias = max(0.0, float(d.pre_score) - float(d.seq_score))
                    rows.append((name, deci[i, 0] / 10.0, bias, int(d.nenv)) + ((float(d.seq_score),) if exact else ()))
            recs = dom_off = None
            if display is not None:
                recs, dom_off, hits, lines = self._shared_domain_stage(e, hdr, records, res, offs, flags, det, rows, inc, display)
            elif inc is not None:
                at = {name: i for i, (name, _) in enumerate(records)}
                first = [at[r[0]] for r in formats.hit_order(rows, hdr)]
                order = first + sorted(set(range(len(records))) - set(first))
                hits = e.hits_msa(res, offs, "".join(t for _, t in records), flags, det,
                                  Z=len(records) if inc.get("Z") is None else inc["Z"],
                                  domZ=max(len(rows), 1) if inc.get("domZ") is None else inc["domZ"],
                                  incE=inc.get("incE", 0.01), incdomE=inc.get("incdomE", 0.01), order=order, want_domains=True)
                recs, dom_off = hits.pop("domains"), hits.pop("dom_off")
            elif want_domains:
                recs, dom_off = e.domains(res, offs, flags, det)
            if want_domains:
                for i, (name, _) in enumerate(records):
                    lst = []
                    for r in recs[dom_off[i]:dom_off[i + 1]]:
                        d = {k: r[k].item() for k in recs.dtype.names}
                        d["envsc"] = float(det[i].envsc[d["index"]])
                        lst.append(d)
                    if lst:
                        domains[name] = lst
            if table is not None:
                tbl = e.seq_table(res, offs, flags, det, **table)
        return (hdr, rows, (domains if want_domains else None), hits, tbl) + (() if display is None else (lines,))

    def _shared_domain_stage(self, e, hdr, records, res, offs, flags, det, rows, inc, display):
        """ONE domain stage (EHMM.domain_paths), then the stages that read its records, columns and posteriors on the device:
        the display, and the hit selection of -A where it is asked for.  The display's PP line takes hmmsearch's own
        posteriors, decoded under the whole sequence's length model (EHMM.sequence_model_posteriors: one more alignment
        launch over the envelopes that are shorter than their sequence); the domain records and -A keep the stage's.  With
        WITCH_HIP_DOMAIN_SEQLEN=1 the stage itself aligns under that model: all three read the stage's, one alignment launch.
        Returns (domain records, dom_off, hits or None, display lines)."""
        import torch
        dev = torch.device("cuda", self.device)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
        nq = len(records)
        recs, dom_off, env_off, cols, pp = e.domain_paths(res, offs, flags, det)
        self.calls = ["domain_paths"]
        if self.seqlen:                # (the stage's path and posteriors are hmmsearch's already: no padded-envelope pass)
            pp_seq = pp
        else:
            pp_seq = e.sequence_model_posteriors(res, offs, recs, env_off, cols, pp, h=0)
            self.calls.append("sequence_model_posteriors")
        with torch.cuda.device(dev):
            res_t, offs_t, flags_t = up(res), up(offs), up(np.asarray(flags).reshape(-1))
            dom_t, dom_off_t = up(recs.view(np.uint8).reshape(len(recs), -1)), up(dom_off)
            env_t, cols_t = up(env_off), up(cols)
            domZ = max(len(rows), 1) if display.get("domZ") is None else display["domZ"]
            disp = e.domain_display_t(res_t, offs_t, flags_t, dom_off_t, dom_t, env_t, cols_t, up(pp_seq), domE=display.get("domE", 10.0),
                                      domZ=domZ, h=0)
            hits = None
            if inc is not None:
                at = {name: i for i, (name, _) in enumerate(records)}
                first = [at[r[0]] for r in formats.hit_order(rows, hdr)]
                order = first + sorted(set(range(nq)) - set(first))
                text_t = up(np.frombuffer("".join(t for _, t in records).encode(), dtype=np.uint8).copy())
                det_t = up(np.frombuffer(bytes(det), dtype=np.uint8).copy())
                hits = e.hits_msa_t(text_t, offs_t, flags_t, det_t, dom_off_t, dom_t, env_t, cols_t, up(pp),
                                    Z=nq if inc.get("Z") is None else inc["Z"], domZ=max(len(rows), 1) if inc.get("domZ") is None else inc["domZ"],
                                    incE=inc.get("incE", 0.01), incdomE=inc.get("incdomE", 0.01), h=0, order_t=up(np.array(order, dtype=np.int32)))
        return recs, dom_off, hits, e.display_lines(disp, [n for n, _ in records])

    def align(self, jobs):
        """jobs: [(hmm_path, name, text)] -> [(M, cols, pp)]; one launch per distinct model.  pp: the posterior
        probability of each residue's state on the path (wh_align_pp), hmmalign's PP line."""
        from witch_amd.ehmm import pack_queries
        out = [None] * len(jobs)
        by_model = {}
        for j, (hp, _, _) in enumerate(jobs):
            by_model.setdefault(os.path.realpath(hp), []).append(j)
        with self.lock:
            for hp, idxs in by_model.items():
                e, hdr = self.model(hp)
                seqs = [e.digitize(jobs[j][2].upper()) for j in idxs]
                res, offs = pack_queries(seqs)
                cols, co, pp = e.align(res, offs, np.arange(len(idxs)), np.zeros(len(idxs), dtype=np.int32), want_pp=True)
                for n, j in enumerate(idxs):
                    out[j] = (int(e.M[0]), cols[co[n]:co[n + 1]].copy(), pp[co[n]:co[n + 1]].copy())
        return out

    def align_msa(self, hmm_path, records, trim=False, mapali=None):
        """records: [(name, text)] -> EHMM.msa's dict: hmmalign's ONE alignment of all the sequences to the model, aligned
        and assembled on the device (wh_msa).  The rows carry the records' own characters, match residues upper case and
        inserts lower case.  mapali=(names, rows): hmmalign --mapali, the rows of the model's own alignment in front
        (wh_msa_mapali); MapaliMismatch where the alignment is not the one the model came from."""
        from witch_amd.ehmm import alignment_checksum
        with self.lock:
            e, hdr = self.model(hmm_path)
            res, offs = e.digitize_many([t.upper() for _, t in records])
            if mapali is None:
                return e.msa(res, offs, "".join(t for _, t in records), h=0, trim=trim)
            want = e.cksum(0)
            if want is not None and alignment_checksum({2: "amino", 1: "rna"}.get(e.alphabet, "dna"), mapali[1]) != want:
                raise MapaliMismatch()
            return e.msa(res, offs, "".join(t for _, t in records), h=0, trim=trim, mapali=mapali)


class AlignBatcher:
    """Collects hmmalign jobs that arrive within a short window and runs them together."""

    def __init__(self, backend, window_s=0.0005, max_batch=4096):
        self.backend, self.window, self.max_batch = backend, window_s, max_batch
        self.cv = threading.Condition()
        self.queue = []
        self.thread = threading.Thread(target=self._run, daemon=True)
        self.thread.start()

    def submit(self, job):
        slot = {"job": job, "done": threading.Event(), "result": None, "error": None}
        with self.cv:
            self.queue.append(slot)
            self.cv.notify()
        slot["done"].wait()
        if slot["error"] is not None:
            raise slot["error"]
        return slot["result"]

    def _run(self):
        while True:
            with self.cv:
                while not self.queue:
                    self.cv.wait()
            time.sleep(self.window)                       # let the other workers' requests arrive
            with self.cv:
                batch, self.queue = self.queue[:self.max_batch], self.queue[self.max_batch:]
            try:
                res = self.backend.align([s["job"] for s in batch])
                for s, r in zip(batch, res):
                    s["result"] = r
            except Exception as ex:                       # one bad job fails alone on the retry
                for s in batch:
                    try:
                        s["result"] = self.backend.align([s["job"]])[0]
                    except Exception as ex1:
                        s["error"] = ex1
                del ex
            for s in batch:
                s["done"].set()


class Server:
    def __init__(self, backend, sock_path):
        self.backend = backend
        self.batcher = AlignBatcher(backend)
        self.sock_path = sock_path
        self.stats = {"hmmsearch": 0, "hmmalign": 0}

    # ---------------------------------------------------------------- the two tools
    def run_hmmsearch(self, argv, cwd):
        opts, hmm, fa = parse_hmmsearch_argv(argv)
        hmm, fa = os.path.join(cwd, hmm), os.path.join(cwd, fa)
        if not os.path.exists(hmm):
            raise ArgError("Error: File existence/permissions problem in trying to open HMM file %s." % hmm)
        if not os.path.exists(fa):
            raise ArgError("Error: Failed to open sequence file %s for reading" % fa)
        check_hmmsearch_options(opts)
        F = filter_thresholds(opts)
        fkw = {} if F is None else {"filters": F}           # (a search with --max calls the backend as ever)
        if F is not None and "--nobias" not in opts:        # (accepted above only where the bias filter is switched on)
            fkw["bias"] = True
        passed = lambda: None if F is None else (self.backend.last_passed, F)
        if alidisplay_enabled() and "--noali" not in opts:
            return self.run_hmmsearch_display(opts, hmm, fa, cwd, fkw, passed, argv)
        if "--tblout" in opts:
            return self.run_hmmsearch_table(opts, hmm, fa, cwd, fkw, passed, argv)
        if "-A" in opts:
            return self.run_hmmsearch_hits(opts, hmm, fa, cwd, fkw, passed)
        records = formats.read_fasta(fa)
        if "--domtblout" in opts:
            hdr, rows, domains = self.backend.search(hmm, records, want_domains=True, **fkw)
            lengths = {n: len(t) for n, t in records}
            kw = {"Z": float(opts["-Z"]) if "-Z" in opts else None, "domZ": float(opts["--domZ"]) if "--domZ" in opts else None,
                  "domE": float(opts.get("--domE", 10.0))}
            inc = {"incE": float(opts.get("--incE", 0.01)), "incdomE": float(opts.get("--incdomE", 0.01))}
            text = formats.format_hmmsearch(hmm, fa, hdr, rows, len(records), domains=domains, lengths=lengths, passed=passed(), **kw, **inc)
            with open(os.path.join(cwd, opts["--domtblout"]), "w") as f:
                f.write(formats.format_domtblout(hmm, fa, hdr, rows, lengths, domains, len(records), **kw))
        else:
            hdr, rows = self.backend.search(hmm, records, **fkw)
            text = formats.format_hmmsearch(hmm, fa, hdr, rows, len(records), passed=passed())
        if "-o" in opts:
            with open(os.path.join(cwd, opts["-o"]), "w") as f:
                f.write(text)
            return ""
        return text

    def run_hmmsearch_display(self, opts, hmm, fa, cwd, fkw, passed, argv):
        """A line without --noali where the display is switched on (alidisplay_enabled): the main output carries hmmsearch's
        "(and alignments)" section - every domain table followed by the alignment of its reportable domains, wrapped to
        --textw N (default 120; --notextw: one block).  --domtblout, -A and --tblout on the same line are written as they are
        without the display, and share its one alignment of the envelopes."""
        if not hasattr(self.backend, "search_display"):
            raise ArgError("witch-hip hmmsearch shim: the alignment display (WITCH_HIP_ALIDISPLAY=1, no --noali) needs a backend "
                           "that renders the domain alignments (search_display); this one does not, and the request is not ignored: "
                           "pass --noali")
        textw = display_textw(opts)
        keys = formats.hmm_display_keys(hmm)
        for k, want, why in (("CONS", True, "has no consensus line to print"), ("RF", False, "has a reference line, which HMMER prints above the alignment"),
                             ("CS", False, "has a consensus structure line, which HMMER prints above the alignment")):
            if keys[k] != want:
                raise ArgError("witch-hip hmmsearch shim: the alignment display is implemented for models with CONS yes, RF no and CS no; "
                               "%s says %s %s (it %s): pass --noali" % (hmm, k, "yes" if keys[k] else "no", why))
        desc = {}
        records = formats.read_fasta(fa, descriptions=desc)
        kw = {"Z": float(opts["-Z"]) if "-Z" in opts else None, "domZ": float(opts["--domZ"]) if "--domZ" in opts else None}
        inc = {"incE": float(opts.get("--incE", 0.01)), "incdomE": float(opts.get("--incdomE", 0.01))}
        domE = float(opts.get("--domE", 10.0))
        table = dict(kw, E=float(opts.get("-E", 10.0)), domE=domE, **inc) if "--tblout" in opts else None
        hdr, rows, domains, hits, tbl, lines = self.backend.search_display(hmm, records, {"domE": domE, "domZ": kw["domZ"]},
                                                                           inc=dict(inc, **kw) if "-A" in opts else None, table=table, **fkw)
        trailer = formats.hits_msa_trailer(len(hits["row_recs"]), opts["-A"]) if "-A" in opts else None
        lengths = {n: len(t) for n, t in records}
        kw["domE"] = domE
        text = formats.format_hmmsearch(hmm, fa, hdr, rows, len(records), domains=domains, lengths=lengths, passed=passed(),
                                        trailer=trailer, display={"lines": lines, "textw": textw}, **kw, **inc)
        if "--domtblout" in opts:
            with open(os.path.join(cwd, opts["--domtblout"]), "w") as f:
                f.write(formats.format_domtblout(hmm, fa, hdr, rows, lengths, domains, len(records), **kw))
        if "-A" in opts:
            with open(os.path.join(cwd, opts["-A"]), "w") as f:
                f.write(formats.format_hits_msa([n for n, _ in records], hits["row_recs"], hits["rows"], hits["pp_rows"], hits["pp_cons"],
                                                None if formats.hmm_has_rf(hmm) else hits["rf"], descriptions=desc,
                                                notextw="--notextw" in opts))
        if "--tblout" in opts:
            entries = formats.seq_table_entries(hdr, [n for n, _ in records], tbl, len(records), Z=table["Z"], descriptions=desc)
            with open(os.path.join(cwd, opts["--tblout"]), "w") as f:
                f.write(formats.format_tblout(hmm, fa, hdr, entries, option_settings="hmmsearch " + " ".join(argv), cwd=cwd,
                                              date=time.ctime()))
        if "-o" in opts:
            with open(os.path.join(cwd, opts["-o"]), "w") as f:
                f.write(text)
            return ""
        return text

    def run_hmmsearch_hits(self, opts, hmm, fa, cwd, fkw, passed):
        """hmmsearch -A FILE: the search with the alignment of all included domains written to FILE (Stockholm in blocks of
        200 columns; --notextw: one block), with or without --domtblout in the same call.  The main output gets HMMER's line
        about the file behind "//"; its tables are those of a call without -A."""
        if not hasattr(self.backend, "search_hits"):
            raise ArgError("witch-hip hmmsearch shim: -A needs a backend that aligns the included hits (search_hits); "
                           "this one does not, and the option is not ignored")
        desc = {}
        records = formats.read_fasta(fa, descriptions=desc)
        want = "--domtblout" in opts
        kw = {"Z": float(opts["-Z"]) if "-Z" in opts else None, "domZ": float(opts["--domZ"]) if "--domZ" in opts else None}
        inc = {"incE": float(opts.get("--incE", 0.01)), "incdomE": float(opts.get("--incdomE", 0.01))}
        hdr, rows, domains, hits = self.backend.search_hits(hmm, records, dict(inc, **kw), want_domains=want, **fkw)
        n_rows = len(hits["row_recs"])
        trailer = formats.hits_msa_trailer(n_rows, opts["-A"])
        if want:
            lengths = {n: len(t) for n, t in records}
            kw["domE"] = float(opts.get("--domE", 10.0))
            text = formats.format_hmmsearch(hmm, fa, hdr, rows, len(records), domains=domains, lengths=lengths, passed=passed(),
                                            trailer=trailer, **kw, **inc)
            with open(os.path.join(cwd, opts["--domtblout"]), "w") as f:
                f.write(formats.format_domtblout(hmm, fa, hdr, rows, lengths, domains, len(records), **kw))
        else:
            text = formats.format_hmmsearch(hmm, fa, hdr, [r[:4] for r in rows], len(records), passed=passed(), trailer=trailer)
        with open(os.path.join(cwd, opts["-A"]), "w") as f:
            f.write(formats.format_hits_msa([n for n, _ in records], hits["row_recs"], hits["rows"], hits["pp_rows"], hits["pp_cons"],
                                            None if formats.hmm_has_rf(hmm) else hits["rf"], descriptions=desc,
                                            notextw="--notextw" in opts))
        if "-o" in opts:
            with open(os.path.join(cwd, opts["-o"]), "w") as f:
                f.write(text)
            return ""
        return text

    def run_hmmsearch_table(self, opts, hmm, fa, cwd, fkw, passed, argv):
        """hmmsearch --tblout FILE: the search with the per-sequence table written to FILE, alone or together with
        --domtblout and -A, from one scoring call.  The main output and the other files are those of the same call
        without --tblout."""
        if not hasattr(self.backend, "search_table"):
            raise ArgError("witch-hip hmmsearch shim: --tblout needs a backend that assembles the per-sequence table "
                           "(search_table); this one does not, and the option is not ignored")
        if "-A" in opts and not hasattr(self.backend, "search_hits"):
            raise ArgError("witch-hip hmmsearch shim: -A needs a backend that aligns the included hits (search_hits); "
                           "this one does not, and the option is not ignored")
        desc = {}
        records = formats.read_fasta(fa, descriptions=desc)
        want = "--domtblout" in opts
        kw = {"Z": float(opts["-Z"]) if "-Z" in opts else None, "domZ": float(opts["--domZ"]) if "--domZ" in opts else None}
        inc = {"incE": float(opts.get("--incE", 0.01)), "incdomE": float(opts.get("--incdomE", 0.01))}
        table = dict(kw, E=float(opts.get("-E", 10.0)), domE=float(opts.get("--domE", 10.0)), **inc)
        hdr, rows, domains, hits, tbl = self.backend.search_table(hmm, records, table, want_domains=want,
                                                                  inc=dict(inc, **kw) if "-A" in opts else None, **fkw)
        trailer = formats.hits_msa_trailer(len(hits["row_recs"]), opts["-A"]) if "-A" in opts else None
        if want:
            lengths = {n: len(t) for n, t in records}
            kw["domE"] = float(opts.get("--domE", 10.0))
            text = formats.format_hmmsearch(hmm, fa, hdr, rows, len(records), domains=domains, lengths=lengths, passed=passed(),
                                            trailer=trailer, **kw, **inc)
            with open(os.path.join(cwd, opts["--domtblout"]), "w") as f:
                f.write(formats.format_domtblout(hmm, fa, hdr, rows, lengths, domains, len(records), **kw))
        else:
            text = formats.format_hmmsearch(hmm, fa, hdr, [r[:4] for r in rows], len(records), passed=passed(), trailer=trailer)
        if "-A" in opts:
            with open(os.path.join(cwd, opts["-A"]), "w") as f:
                f.write(formats.format_hits_msa([n for n, _ in records], hits["row_recs"], hits["rows"], hits["pp_rows"], hits["pp_cons"],
                                                None if formats.hmm_has_rf(hmm) else hits["rf"], descriptions=desc,
                                                notextw="--notextw" in opts))
        entries = formats.seq_table_entries(hdr, [n for n, _ in records], tbl, len(records), Z=table["Z"], descriptions=desc)
        with open(os.path.join(cwd, opts["--tblout"]), "w") as f:
            f.write(formats.format_tblout(hmm, fa, hdr, entries, option_settings="hmmsearch " + " ".join(argv), cwd=cwd,
                                          date=time.ctime()))
        if "-o" in opts:
            with open(os.path.join(cwd, opts["-o"]), "w") as f:
                f.write(text)
            return ""
        return text

    def run_hmmalign(self, argv, cwd):
        opts, hmm, fa = parse_hmmalign_argv(argv)
        hmm, fa = os.path.join(cwd, hmm), os.path.join(cwd, fa)
        if not os.path.exists(hmm):
            raise ArgError("Error: File existence/permissions problem in trying to open HMM file %s." % hmm)
        if not os.path.exists(fa):
            raise ArgError("Error: Failed to open sequence file %s for reading" % fa)
        records = formats.read_fasta(fa)
        if "--mapali" in opts:
            # the rows of the model's alignment come with every call, also one for a single sequence
            if not hasattr(self.backend, "align_msa"):
                raise ArgError("witch-hip hmmalign shim: --mapali needs a backend that assembles alignments (align_msa); "
                               "this one does not, and the option is not ignored")
            return self.run_hmmalign_msa(opts, hmm, fa, records, cwd)
        if len(records) != 1 and hasattr(self.backend, "align_msa"):
            return self.run_hmmalign_msa(opts, hmm, fa, records, cwd)
        if len(records) != 1:
            # WITCH aligns one query per call (aligner.py:90-100); a multi-sequence alignment
            # needs the shared insert columns hmmalign computes, which this backend does not emit
            raise ArgError("witch-hip hmmalign shim: exactly one sequence per call (got %d)" % len(records))
        name, text = records[0]
        res = self.batcher.submit((hmm, name, text))
        if len(res) > 2 and res[2] is not None:
            # hmmalign's own layout: PP, PP_cons and RF lines, the C flank behind the model's last column
            M, cols, pp = res[:3]
            sto = formats.format_stockholm(name, formats.stockholm_row(text, cols, M, flank_at_end=True), pp=pp,
                                           rf=not formats.hmm_has_rf(hmm))
        else:                                             # a backend without posteriors: the sequence line alone
            M, cols = res[:2]
            sto = formats.format_stockholm(name, formats.stockholm_row(text, cols, M))
        if "-o" in opts:
            with open(os.path.join(cwd, opts["-o"]), "w") as f:
                f.write(sto)
            return ""
        return sto

    def run_hmmalign_msa(self, opts, hmm, fa, records, cwd):
        """A file of several sequences: hmmalign's one alignment of all of them (the reference's bundled MAGUS, SEPP and UPP
        call it so), honouring --trim, --outformat Stockholm | Pfam | afa and -o."""
        if not records:
            raise ArgError("Error: Sequence file %s is empty or misformatted" % fa)
        outformat = opts.get("--outformat", "Stockholm")
        if str(outformat).lower() not in formats.MSA_FORMATS:
            raise ArgError("ERROR: %s is not a recognized output MSA file format (witch-hip hmmalign shim: Stockholm, Pfam, afa)" % outformat)
        names, pp_rows, desc = [n for n, _ in records], None, None
        if "--mapali" in opts:
            ali_path = os.path.join(cwd, opts["--mapali"])
            if not os.path.exists(ali_path):
                raise ArgError("Error: Failed to open --mapali alignment file %s for reading" % ali_path)
            try:
                ali = formats.read_msa(ali_path)
            except ValueError as ex:
                raise ArgError("Error: %s" % ex)
            try:
                m = self.backend.align_msa(hmm, records, trim="--trim" in opts, mapali=(ali["names"], ali["rows"]))
            except MapaliMismatch:
                # HMMER's own words and its exit status 1
                raise ArgError("--mapali MSA %s isn't same as the one HMM came from (checksum mismatch)" % opts["--mapali"])
            names, desc = ali["names"] + names, ali["desc"]
            pp_rows = [None] * len(ali["names"]) + list(m["pp_rows"])
        else:
            m = self.backend.align_msa(hmm, records, trim="--trim" in opts)
            pp_rows = m["pp_rows"]
        text = formats.format_msa(names, m["rows"], pp_rows, m["pp_cons"], None if formats.hmm_has_rf(hmm) else m["rf"], outformat,
                                  **({"desc": desc} if desc else {}))
        if "-o" in opts:
            with open(os.path.join(cwd, opts["-o"]), "w") as f:
                f.write(text)
            return ""
        return text

    # ---------------------------------------------------------------- plumbing
    def handle(self, conn):
        try:
            buf = b""
            while True:
                chunk = conn.recv(65536)
                if not chunk:
                    break
                buf += chunk
            parts = buf.split(b"\0")
            if parts and parts[-1] == b"":
                parts.pop()
            if len(parts) < 2:
                raise ArgError("malformed request")
            tool, cwd, argv = parts[0].decode(), parts[1].decode(), [p.decode() for p in parts[2:]]
            if tool == "hmmsearch":
                out = self.run_hmmsearch(argv, cwd)
            elif tool == "hmmalign":
                out = self.run_hmmalign(argv, cwd)
            elif tool == "shutdown":
                conn.sendall(b"0\nbye\n")
                conn.close()
                os._exit(0)
            elif tool == "ping":
                out = "pong %d %d\n" % (self.stats["hmmsearch"], self.stats["hmmalign"])
            else:
                raise ArgError("unknown tool %r" % tool)
            if tool in self.stats:
                self.stats[tool] += 1
            conn.sendall(b"0\n" + out.encode())
        except ArgError as ex:
            conn.sendall(b"1\n" + str(ex).encode() + b"\n")
        except Exception as ex:                           # HMMER exits 1 with a message; so do we
            conn.sendall(b"1\nError: " + ("%s: %s" % (type(ex).__name__, ex)).encode() + b"\n")
        finally:
            try:
                conn.close()
            except OSError:
                pass

    def serve_forever(self, ready=None, idle_timeout=None):
        """One server per socket: an exclusive flock on <socket>.lock is taken BEFORE the socket is
        touched (and before any GPU call), so of the many clients WITCH starts at once - each of which
        launches a server when it cannot connect - exactly one server survives; the others exit 0 and
        their clients connect to the survivor.  The server leaves after <idle_timeout> seconds without
        a request ($WITCH_HIP_IDLE_TIMEOUT, default 3600; 0 = never)."""
        import fcntl
        private_socket_dir(self.sock_path)
        self._lockf = open(self.sock_path + ".lock", "w")
        for attempt in range(100):
            try:
                fcntl.flock(self._lockf, fcntl.LOCK_EX | fcntl.LOCK_NB)
                break
            except OSError:
                # another server owns this socket - unless it is just leaving (idle shutdown: path already
                # unlinked, lock released a moment later): then wait for the lock instead of giving up
                if os.path.exists(self.sock_path) or attempt == 99:
                    return False
                time.sleep(0.05)
        if os.path.exists(self.sock_path):
            os.unlink(self.sock_path)
        old_umask = os.umask(0o077)
        try:
            srv = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
            srv.bind(self.sock_path)
        finally:
            os.umask(old_umask)
        srv.listen(512)
        if idle_timeout is None:
            idle_timeout = float(os.environ.get("WITCH_HIP_IDLE_TIMEOUT", "3600"))
        srv.settimeout(idle_timeout if idle_timeout > 0 else None)
        if ready is not None:
            ready.set()
        while True:
            try:
                conn, _ = srv.accept()
            except socket.timeout:
                if threading.active_count() > 2:          # requests still running: keep going
                    continue
                # Leave without dropping anyone: unlink the path FIRST (a client arriving from now on finds no
                # socket and starts a fresh server, which waits on the flock until this one is gone), then serve
                # whatever is already in the listen backlog before closing.
                try:
                    os.unlink(self.sock_path)
                except OSError:
                    pass
                fcntl.flock(self._lockf, fcntl.LOCK_UN)    # a successor may bind a new socket while the backlog drains
                srv.setblocking(False)
                late = []
                while True:
                    try:
                        conn, _ = srv.accept()
                    except (BlockingIOError, OSError):
                        break
                    conn.settimeout(None)
                    t = threading.Thread(target=self.handle, args=(conn,), daemon=True)
                    t.start()
                    late.append(t)
                for t in late:
                    t.join()
                srv.close()
                return True
            conn.settimeout(None)
            threading.Thread(target=self.handle, args=(conn,), daemon=True).start()


def request(sock_path, tool, argv, cwd=None):
    """Python twin of client.c (tests and tooling): returns (status, text)."""
    s = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
    s.connect(sock_path)
    s.sendall(b"\0".join([tool.encode(), (cwd or os.getcwd()).encode()] + [a.encode() for a in argv]) + b"\0")
    s.shutdown(socket.SHUT_WR)
    buf = b""
    while True:
        chunk = s.recv(65536)
        if not chunk:
            break
        buf += chunk
    s.close()
    head, _, body = buf.partition(b"\n")
    return int(head or b"1"), body.decode()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--socket", default=default_socket_path())
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--daemonize", action="store_true", help="detach (the clients start the server this way)")
    args = ap.parse_args()
    if args.daemonize:
        # fork BEFORE anything touches HIP
        if os.fork() > 0:
            return
        os.setsid()
        if os.fork() > 0:
            os._exit(0)
        private_socket_dir(args.socket)
        log = open(args.socket + ".log", "a")
        os.dup2(log.fileno(), 1)
        os.dup2(log.fileno(), 2)
        sys.stdin.close()
    private_socket_dir(args.socket)
    Server(GpuBackend(args.device), args.socket).serve_forever()


if __name__ == "__main__":
    main()
