"""Text formats of the level-0 shim: FASTA in, hmmsearch per-sequence table, single-sequence
Stockholm and hmmalign's multi-sequence alignment (Stockholm, Pfam, afa) out.  Pure Python, no GPU."""
import math


def read_fasta(path, descriptions=None):
    """[(name, sequence)] - name is the first word of the header, like HMMER's sqio.  descriptions: a dict that receives
    {name: the rest of the header line} for the records that have one (the "DE" text of hmmsearch -A)."""
    out, name, chunks = [], None, []
    with open(path) as f:
        for line in f:
            line = line.rstrip("\n")
            if line.startswith(">"):
                if name is not None:
                    out.append((name, "".join(chunks)))
                words = line[1:].split(None, 1)
                name = words[0] if words else ""
                if descriptions is not None and len(words) > 1 and words[1].strip():
                    descriptions[name] = words[1].strip()
                chunks = []
            elif name is not None:
                chunks.append(line.strip())
    if name is not None:
        out.append((name, "".join(chunks)))
    return out


def hmm_header(path):
    """NAME, LENG and the Forward E-value parameters (tau, lambda) of a HMMER3/f file."""
    info = {"name": "unnamed", "M": 0, "ftau": None, "flambda": None}
    opener = open
    if str(path).endswith(".gz"):
        import gzip
        opener = gzip.open
    with opener(path, "rt") as f:
        for line in f:
            w = line.split()
            if not w:
                continue
            if w[0] == "NAME":
                info["name"] = w[1]
            elif w[0] == "LENG":
                info["M"] = int(w[1])
            elif w[0] == "STATS" and len(w) >= 5 and w[2] == "FORWARD":
                info["ftau"], info["flambda"] = float(w[3]), float(w[4])
            elif w[0] == "HMM":
                break
    return info


def forward_evalue(bits, n_targets, ftau, flambda):
    """E = Z * P(score >= s) with the exponential tail HMMER fits for Forward scores
    (P = exp(-lambda (s - tau)) for s >= tau, else 1).  WITCH never reads it (loader.py:293)."""
    if ftau is None or flambda is None:
        return 0.0
    x = bits - ftau
    p = 1.0 if x < 0 else math.exp(max(-745.0, -flambda * x))
    return p * n_targets


def _g(x):
    return "%9.2g" % x


def _hmmsearch_head(hmm_path, fasta_path, hdr, rows):
    """(lines up to the per-sequence table's rule, width of its name column): shared by both forms of the main output."""
    namew = max([8] + [len(r[0]) for r in rows])
    out = []
    out.append("# hmmsearch :: search profile(s) against a sequence database")
    out.append("# witch-hip level-0 shim (MI355X); table layout of HMMER 3.1b2")
    out.append("# - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - -")
    out.append("# query HMM file:                  %s" % hmm_path)
    out.append("# target sequence database:        %s" % fasta_path)
    out.append("# - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - - -")
    out.append("")
    out.append("Query:       %s  [M=%d]" % (hdr["name"], hdr["M"]))
    out.append("Scores for complete sequences (score includes all domains):")
    out.append("   --- full sequence ---   --- best 1 domain ---    -#dom-")
    out.append("    E-value  score  bias    E-value  score  bias    exp  N  %-*s Description" % (namew, "Sequence"))
    out.append("    ------- ------ -----    ------- ------ -----   ---- --  %s -----------" % ("-" * namew))
    if not rows:
        out.append("")
        out.append("   [No hits detected that satisfy reporting thresholds]")
    return out, namew


def _hmmsearch_tail(out, hdr, n_targets, passed=None, trailer=None):
    """The pipeline summary that ends the main output; returns the text.  passed: None (a search with --max, as ever), or
    ((n MSV, n bias, n Vit, n Fwd), (F1, F2, F3)) of a filtered search: HMMER's four "Passed ... filter:" lines.
    trailer: a line behind "//" (hits_msa_trailer: what hmmsearch -A says about its file)."""
    out.append("")
    out.append("")
    out.append("Internal pipeline statistics summary:")
    out.append("-------------------------------------")
    out.append("Query model(s):                            1  (%d nodes)" % hdr["M"])
    out.append("Target sequences:                   %8d" % n_targets)
    if passed is not None:
        (n1, nb, n2, n3), (F1, F2, F3) = passed
        nt = float(max(n_targets, 1))
        for label, n, F in (("MSV", n1, F1), ("bias", nb, F1), ("Vit", n2, F2), ("Fwd", n3, F3)):
            out.append("%-28s%15d  (%.6g); expected %.1f (%.6g)" % ("Passed %s filter:" % label, n, n / nt, F * n_targets, F))
    out.append("//")
    if trailer is not None:
        out.append(trailer)
    out.append("[ok]")
    return "\n".join(out) + "\n"


def format_hmmsearch(hmm_path, fasta_path, hdr, rows, n_targets, domains=None, lengths=None, Z=None, domZ=None, domE=10.0,
                     incE=0.01, incdomE=0.01, passed=None, trailer=None, display=None):
    """rows: [(name, bits, bias_bits, n_domains)] of the REPORTED sequences.  The table is what
    evalHMMSearchOutput reads: a line starting with 'E-value', then >= 9 whitespace-separated
    fields per row (E-value, score, bias, best-domain E-value/score/bias, exp, N, name), a blank
    line to end.  Without <domains> the best-domain columns repeat the full-sequence values (not computed).
    With <domains> ({name: [domain records]}, see domain_entries; lengths: {name: residues}; a row may carry the
    unrounded score as a fifth element, for the E-values) they hold the
    i-Evalue, score and bias of the pair's best domain (the highest envelope score), N is the number of reportable
    domains (incE / incdomE decide the '!' marks), and HMMER's "Domain annotation for each sequence" section (its ">> name" tables, as under --noali) follows.
    passed: the stage counts and thresholds of a filtered search (_hmmsearch_tail); None under --max.  trailer: see there.
    display (with <domains> only): the alignment display, see _format_hmmsearch_domains; None: the output of --noali."""
    if domains is not None:
        return _format_hmmsearch_domains(hmm_path, fasta_path, hdr, rows, n_targets, domains, lengths, Z, domZ, domE, incE, incdomE, passed, trailer,
                                         display)
    out, namew = _hmmsearch_head(hmm_path, fasta_path, hdr, rows)
    for name, bits, bias, ndom in sorted(rows, key=lambda r: -r[1]):
        ev = forward_evalue(bits, n_targets, hdr["ftau"], hdr["flambda"])
        out.append("  %s %6.1f %5.1f  %s %6.1f %5.1f  %5.1f %2d  %-*s " %
                   (_g(ev), bits, bias, _g(ev), bits, bias, float(max(ndom, 1)), max(ndom, 1), namew, name))
    return _hmmsearch_tail(out, hdr, n_targets, passed, trailer)


# ------------------------------------------------------------------------------------------------ per-domain output
DOMTBL_COLUMNS = ["target", "tacc", "tlen", "query", "qacc", "qlen", "evalue", "score", "bias", "num", "of", "c_evalue",
                  "i_evalue", "dom_score", "dom_bias", "hmm_from", "hmm_to", "ali_from", "ali_to", "env_from", "env_to", "acc"]


def ln_survival(bits, ftau, flambda):
    """ln P(score >= bits) under HMMER's exponential tail for Forward scores: min(0, -lambda (bits - tau))."""
    return 0.0 if bits < ftau else -flambda * (bits - ftau)


def _exact(row):
    """A row's score for E-values and ordering: its fifth element (the unrounded float32 score) when it has one, else the
    printed one."""
    return row[4] if len(row) > 4 else row[1]


def hit_order(rows, hdr):
    """The reported sequences in HMMER's order: by E-value, ties (all the scores below tau have P = 1) by name."""
    if hdr.get("ftau") is None or hdr.get("flambda") is None:
        return sorted(rows, key=lambda r: (-_exact(r), r[0]))
    return sorted(rows, key=lambda r: (ln_survival(_exact(r), hdr["ftau"], hdr["flambda"]), r[0]))


def domain_entries(hdr, rows, lengths, domains, n_targets, Z=None, domZ=None, domE=10.0, incE=0.01, incdomE=0.01):
    """One dict per domain of every reported sequence, in HMMER's output order, with the 22 columns of a --domtblout
    line as numbers (DOMTBL_COLUMNS) plus "c_evalue_ftz" (the c-Evalue as the reference's binary evaluates it, a P-value below
    the smallest normal double flushed to 0: _pvalue; the alignment display's header prints it), "reportable" (c-Evalue <= domE) and "included" (the '!' of a domain table: the
    sequence's E-value <= incE and the domain's c-Evalue <= incdomE, hmmsearch's --incE / --incdomE, default 0.01).
    domains: {name: [records]}, a record having index, of, env_i, env_j, ali_i, ali_j, hmm_i, hmm_j, bits, bias_bits, oasc,
    lnP (the fields of wh_domain).  Z defaults to the number of targets, domZ to the number of reported sequences; "#" and
    "of" count all the pair's domains."""
    Z = float(n_targets if Z is None else Z)
    domZ = float(len(rows) if domZ is None else domZ)
    out = []
    for row in hit_order(rows, hdr):
        name, bits, bias = row[:3]
        ev = forward_evalue(_exact(row), Z, hdr["ftau"], hdr["flambda"])
        for d in domains.get(name, []):
            p = math.exp(max(-745.0, float(d["lnP"]))) if d["lnP"] == d["lnP"] else 0.0
            Ld = int(d["env_j"]) - int(d["env_i"]) + 1
            out.append({"target": name, "tacc": "-", "tlen": int(lengths[name]), "query": hdr["name"], "qacc": "-",
                        "qlen": int(hdr["M"]), "evalue": ev, "score": float(bits), "bias": float(bias),
                        "num": int(d["index"]) + 1, "of": int(d["of"]), "c_evalue": p * domZ, "i_evalue": p * Z,
                        "dom_score": float(d["bits"]), "dom_bias": float(d["bias_bits"]),
                        "hmm_from": int(d["hmm_i"]), "hmm_to": int(d["hmm_j"]), "ali_from": int(d["ali_i"]),
                        "ali_to": int(d["ali_j"]), "env_from": int(d["env_i"]), "env_to": int(d["env_j"]),
                        "acc": float(d["oasc"]) / Ld, "c_evalue_ftz": _pvalue(float(d["lnP"])) * domZ, "reportable": p * domZ <= domE,
                        "included": ev <= incE and p * domZ <= incdomE})
    return out


def _domtbl_widths(entries):
    return (max([20] + [len(e["target"]) for e in entries]), max([20] + [len(e["query"]) for e in entries]),
            max([10] + [len(e["tacc"]) for e in entries]), max([10] + [len(e["qacc"]) for e in entries]))


def format_domtblout_lines(entries, widths=None):
    """HMMER 3.1b2's --domtblout line for each entry (DOMTBL_COLUMNS as numbers; description "-")."""
    tw, qw, taw, qaw = widths or _domtbl_widths(entries)
    return ["%-*s %-*s %5d %-*s %-*s %5d %9.2g %6.1f %5.1f %3d %3d %9.2g %9.2g %6.1f %5.1f %5d %5d %5d %5d %5d %5d %4.2f %s" %
            (tw, e["target"], taw, e["tacc"], e["tlen"], qw, e["query"], qaw, e["qacc"], e["qlen"], e["evalue"], e["score"],
             e["bias"], e["num"], e["of"], e["c_evalue"], e["i_evalue"], e["dom_score"], e["dom_bias"], e["hmm_from"],
             e["hmm_to"], e["ali_from"], e["ali_to"], e["env_from"], e["env_to"], e["acc"], "-") for e in entries]


def format_domtblout_header(widths):
    tw, qw, taw, qaw = widths
    return ["#%*s %22s %40s %11s %11s %11s" % (tw + qw - 1 + 15 + taw + qaw, "", "--- full sequence ---",
                                                  "-------------- this domain -------------", "hmm coord", "ali coord", "env coord"),
            "#%-*s %-*s %5s %-*s %-*s %5s %9s %6s %5s %3s %3s %9s %9s %6s %5s %5s %5s %5s %5s %5s %5s %4s %s" %
            (tw - 1, " target name", taw, "accession", "tlen", qw, "query name", qaw, "accession", "qlen", "E-value", "score",
             "bias", "#", "of", "c-Evalue", "i-Evalue", "score", "bias", "from", "to", "from", "to", "from", "to", "acc",
             "description of target"),
            "#%s %s %s %s %s %s %s %s %s %s %s %s %s %s %s %s %s %s %s %s %s %s %s" %
            ("-" * (tw - 1), "-" * taw, "-----", "-" * qw, "-" * qaw, "-----", "---------", "------", "-----", "---", "---",
             "---------", "---------", "------", "-----", "-----", "-----", "-----", "-----", "-----", "-----", "----",
             "---------------------")]


def format_domtblout(hmm_path, fasta_path, hdr, rows, lengths, domains, n_targets, Z=None, domZ=None, domE=10.0):
    """The --domtblout file in HMMER 3.1b2's layout: three header lines, one line per reportable domain, the trailer's
    comment lines (program, version, pipeline mode, the two files, [ok])."""
    entries = [e for e in domain_entries(hdr, rows, lengths, domains, n_targets, Z, domZ, domE) if e["reportable"]]
    widths = _domtbl_widths(entries) if entries else (20, max(20, len(hdr["name"])), 10, 10)
    out = format_domtblout_header(widths) + format_domtblout_lines(entries, widths)
    out += ["#", "# Program:         hmmsearch", "# Version:         3.1b2 (February 2015)", "# Pipeline mode:   SEARCH",
            "# Query file:      %s" % hmm_path, "# Target file:     %s" % fasta_path, "# [ok]"]
    return "\n".join(out) + "\n"


# ------------------------------------------------------------------------------------------------ per-sequence table
TBL_COLUMNS = ["target", "tacc", "query", "qacc", "evalue", "score", "bias", "best_evalue", "best_score", "best_bias", "exp", "reg",
               "clu", "ov", "env", "dom", "rep", "inc", "desc"]


def _pvalue(lnp):
    """exp(lnP) as the reference's hmmsearch binary evaluates it: its SSE build runs with flush-to-zero and
    denormals-are-zero set, so a P-value below the smallest NORMAL double (2.2e-308) prints as 0.  NaN (no STATS line): 0."""
    if lnp != lnp:
        return 0.0
    p = math.exp(lnp)
    return p if p >= 2.2250738585072014e-308 else 0.0


def seq_table_entries(hdr, names, table, n_targets, H=1, Z=None, descriptions=None):
    """One dict per row of EHMM.seq_table (TBL_COLUMNS as numbers, plus "capped"), in HMMER's hit order.  names: the
    searched records' names by query number; Z defaults to the number of targets.  A model without STATS lines has no
    E-values: 0, as in the main output."""
    Z = float(n_targets if Z is None else Z)
    descriptions = descriptions or {}
    rows = {}
    for r in table:
        name = names[int(r["pair"]) // H]
        lnp, blnp = float(r["seq_lnP"]), float(r["best_lnP"])
        rows[name] = {"target": name, "tacc": "-", "query": hdr["name"], "qacc": "-",
                      "evalue": _pvalue(lnp) * Z, "score": float(r["seq_bits"]),
                      "bias": float(r["seq_bias_bits"]), "best_evalue": _pvalue(blnp) * Z,
                      "best_score": float(r["best_bits"]), "best_bias": float(r["best_bias_bits"]), "exp": float(r["exp"]),
                      "reg": int(r["reg"]), "clu": int(r["clu"]), "ov": int(r["ov"]), "env": int(r["env"]), "dom": int(r["dom"]),
                      "rep": int(r["rep"]), "inc": int(r["inc"]), "desc": descriptions.get(name, "-"), "capped": bool(r["capped"])}
    order = hit_order([(n, e["score"], e["bias"], e["dom"], e["score"]) for n, e in rows.items()], hdr)
    return [rows[o[0]] for o in order]


def _tbl_widths(entries):
    return (max([20] + [len(e["target"]) for e in entries]), max([20] + [len(e["query"]) for e in entries]),
            max([10] + [len(e["tacc"]) for e in entries]), max([10] + [len(e["qacc"]) for e in entries]))


def format_tblout_header(widths=(20, 20, 10, 10)):
    """The three comment lines in front of HMMER 3.1b2's --tblout rows; the name columns grow with the longest name."""
    tw, qw, taw, qaw = widths
    return ["#%*s %22s %22s %33s" % (tw + qw + taw + qaw + 2, "", "--- full sequence ----", "--- best 1 domain ----",
                                     "--- domain number estimation ----"),
            "#%-*s %-*s %-*s %-*s %9s %6s %5s %9s %6s %5s %5s %3s %3s %3s %3s %3s %3s %3s %s" %
            (tw - 1, " target name", taw, "accession", qw, "query name", qaw, "accession", "  E-value", " score", " bias",
             "  E-value", " score", " bias", "exp", "reg", "clu", " ov", "env", "dom", "rep", "inc", "description of target"),
            "#%s %s %s %s %s %s %s %s %s %s %s %s %s %s %s %s %s %s %s" %
            ("-" * (tw - 1), "-" * taw, "-" * qw, "-" * qaw, "---------", "------", "-----", "---------", "------", "-----",
             "  ---", "---", "---", "---", "---", "---", "---", "---", "---------------------")]


def format_tblout_lines(entries, widths=None):
    """HMMER 3.1b2's --tblout line for each entry (TBL_COLUMNS as numbers)."""
    tw, qw, taw, qaw = widths or _tbl_widths(entries)
    return ["%-*s %-*s %-*s %-*s %9.2g %6.1f %5.1f %9.2g %6.1f %5.1f %5.1f %3d %3d %3d %3d %3d %3d %3d %s" %
            (tw, e["target"], taw, e["tacc"], qw, e["query"], qaw, e["qacc"], e["evalue"], e["score"], e["bias"], e["best_evalue"],
             e["best_score"], e["best_bias"], e["exp"], e["reg"], e["clu"], e["ov"], e["env"], e["dom"], e["rep"], e["inc"],
             e.get("desc") or "-") for e in entries]


def format_tblout(hmm_path, fasta_path, hdr, entries, option_settings=None, cwd=None, date=None):
    """The --tblout file in HMMER 3.1b2's layout: three header lines, one line per reported sequence in hit order, the
    trailer's comment lines (program, version, pipeline mode, the two files; the command line, the directory and the date -
    date: time.ctime()'s text, as HMMER writes it - where the caller gives them; [ok]).  A row whose record is capped
    (EHMM.seq_table: more envelopes than a detail record lists) is written as it is, and one extra comment line in front of
    the trailer names those sequences: their env, dom, ov, rep, inc and best domain are lower bounds."""
    widths = _tbl_widths(entries) if entries else (20, max(20, len(hdr["name"])), 10, 10)
    out = format_tblout_header(widths) + format_tblout_lines(entries, widths)
    capped = [e["target"] for e in entries if e.get("capped")]
    if capped:
        out.append("# witch-hip: env, dom, ov, rep, inc and the best domain are lower bounds (more envelopes than are listed) for: %s" %
                   " ".join(capped))
    out += ["#", "# Program:         hmmsearch", "# Version:         3.1b2 (February 2015)", "# Pipeline mode:   SEARCH",
            "# Query file:      %s" % hmm_path, "# Target file:     %s" % fasta_path]
    if option_settings is not None:
        out.append("# Option settings: %s" % option_settings)
    if cwd is not None:
        out.append("# Current dir:     %s" % cwd)
    if date is not None:
        out.append("# Date:            %s" % date)
    out.append("# [ok]")
    return "\n".join(out) + "\n"


def format_domain_table(name, entries, M, L):
    """HMMER's ">> name" section of one reported sequence (as printed under --noali): its reportable domains."""
    out = [">> %s  " % name]
    shown = [e for e in entries if e["reportable"]]
    if not shown:
        out.append("   [No individual domains that satisfy reporting thresholds (although complete target did)]")
        out.append("")
        return out
    out.append(" %3s   %6s %5s %9s %9s %7s %7s %2s %7s %7s %2s %7s %7s %2s %4s" %
               ("#", "score", "bias", "c-Evalue", "i-Evalue", "hmmfrom", "hmm to", "  ", "alifrom", "ali to", "  ", "envfrom", "env to",
                "  ", "acc"))
    out.append(" %3s   %6s %5s %9s %9s %7s %7s %2s %7s %7s %2s %7s %7s %2s %4s" %
               ("---", "------", "-----", "---------", "---------", "-------", "-------", "  ", "-------", "-------", "  ", "-------",
                "-------", "  ", "----"))
    for e in shown:
        out.append(" %3d %c %6.1f %5.1f %9.2g %9.2g %7d %7d %c%c %7d %7d %c%c %7d %7d %c%c %4.2f" %
                   (e["num"], "!" if e["included"] else "?", e["dom_score"], e["dom_bias"], e["c_evalue"], e["i_evalue"],
                    e["hmm_from"], e["hmm_to"], "[" if e["hmm_from"] == 1 else ".", "]" if e["hmm_to"] == M else ".",
                    e["ali_from"], e["ali_to"], "[" if e["ali_from"] == 1 else ".", "]" if e["ali_to"] == L else ".",
                    e["env_from"], e["env_to"], "[" if e["env_from"] == 1 else ".", "]" if e["env_to"] == L else ".", e["acc"]))
    out.append("")
    return out


def format_alidisplay(hmm_name, seq_name, hmm_from, ali_from, model, mline, aseq, ppline, textw=120):
    """The lines of one domain's alignment under its "== domain" header, as HMMER 3.1b2's p7_alidisplay_Print lays them out.
    model, mline, aseq, ppline: the four lines of EHMM.domain_display, one character per column (str, bytes or uint8 arrays).
    Names are right-aligned to the longer of the two; the start coordinates are right-aligned and the end coordinates
    left-aligned to the widest of the domain's four coordinates.  The columns are wrapped into blocks of
    textw - name width - 2 x coordinate width - 5 columns (at least 40 where that does not hold the whole alignment), a blank
    line between two blocks, each block with the coordinates of its own first and last node and residue; textw None
    (--notextw): one block.  A block whose target line holds no residue has "-" for both target coordinates."""
    model, mline, aseq, ppline = _text(model), _text(mline), _text(aseq), _text(ppline)
    N = len(model)
    hmm_to = hmm_from + sum(1 for c in model if c != ".") - 1
    ali_to = ali_from + sum(1 for c in aseq if c != "-") - 1
    namew = max(len(hmm_name), len(seq_name))
    cw = max(len(str(v)) for v in (hmm_from, hmm_to, ali_from, ali_to))
    aliw = N if textw is None else textw - namew - 2 * cw - 5
    if aliw < N and aliw < 40:
        aliw = 40
    out, k1, i1 = [], hmm_from, ali_from
    for pos in range(0, N, max(aliw, 1)):
        if pos:
            out.append("")
        mo, aq = model[pos:pos + aliw], aseq[pos:pos + aliw]
        nk, ni = sum(1 for c in mo if c != "."), sum(1 for c in aq if c != "-")
        out.append("  %*s %*d %s %-*d" % (namew, hmm_name, cw, k1, mo, cw, k1 + nk - 1))
        out.append("  %*s %*s %s" % (namew, " ", cw, " ", mline[pos:pos + aliw]))
        if ni > 0:
            out.append("  %*s %*d %s %-*d" % (namew, seq_name, cw, i1, aq, cw, i1 + ni - 1))
        else:
            out.append("  %*s %*s %s %*s" % (namew, seq_name, cw, "-", aq, cw, "-"))
        out.append("  %*s %*s %s PP" % (namew, "", cw, "", ppline[pos:pos + aliw]))
        k1 += nk
        i1 += ni
    return out


def format_domain_alignments(hmm_name, seq_name, entries, lines, textw=120):
    """The "Alignments for each domain:" part behind one sequence's domain table: per reportable domain its header (its
    number among the sequence's REPORTABLE domains, as HMMER counts them; "%.1f" score, "%.2g" conditional E-value),
    format_alidisplay's lines and a blank line.  entries: the
    sequence's domain_entries; lines: {domain number - 1: (model, mline, aseq, ppline)}.  A sequence without a reportable
    domain gets nothing (its table says so already).  A reportable domain without lines - one the alignment gave no path -
    keeps its header and says so in brackets."""
    shown = [e for e in entries if e["reportable"]]
    if not shown:
        return []
    out = ["  Alignments for each domain:"]
    for nd, e in enumerate(shown, 1):
        out.append("  == domain %d  score: %.1f bits;  conditional E-value: %.2g" % (nd, e["dom_score"], e.get("c_evalue_ftz", e["c_evalue"])))
        four = lines.get(e["num"] - 1)
        if four is None:
            out.append("   [No alignment is displayed for this domain: it has no path]")
        else:
            out.extend(format_alidisplay(hmm_name, seq_name, e["hmm_from"], e["ali_from"], *four, textw=textw))
        out.append("")
    return out


def _format_hmmsearch_domains(hmm_path, fasta_path, hdr, rows, n_targets, domains, lengths, Z, domZ, domE, incE, incdomE, passed=None,
                              trailer=None, display=None):
    """display: None (the output of --noali), or {"lines": {name: {domain index: (model, mline, aseq, ppline)}}, "textw":
    the text width or None}: the section's title says "(and alignments)" and every domain table is followed by
    format_domain_alignments."""
    entries = domain_entries(hdr, rows, lengths, domains, n_targets, Z, domZ, domE, incE, incdomE)
    by_name = {}
    for e in entries:
        by_name.setdefault(e["target"], []).append(e)
    order = hit_order(rows, hdr)
    out, namew = _hmmsearch_head(hmm_path, fasta_path, hdr, rows)
    for row in order:
        name, bits, bias, ndom = row[:4]
        ev = forward_evalue(_exact(row), float(n_targets if Z is None else Z), hdr["ftau"], hdr["flambda"])
        doms = by_name.get(name, [])
        nrep = sum(1 for e in doms if e["reportable"])
        if doms:
            recs = domains[name]
            best = doms[max(range(len(doms)), key=lambda t: float(recs[t]["envsc"]) if "envsc" in recs[t] else doms[t]["dom_score"])]
            bev, bsc, bbias = best["i_evalue"], best["dom_score"], best["dom_bias"]
        else:
            bev, bsc, bbias = ev, bits, bias
        out.append("  %s %6.1f %5.1f  %s %6.1f %5.1f  %5.1f %2d  %-*s " %
                   (_g(ev), bits, bias, _g(bev), bsc, bbias, float(max(ndom, 1)), nrep, namew, name))
    out.append("")
    out.append("")
    out.append("Domain annotation for each sequence:" if display is None else "Domain annotation for each sequence (and alignments):")
    for row in order:
        out.extend(format_domain_table(row[0], by_name.get(row[0], []), hdr["M"], lengths[row[0]]))
        if display is not None:
            out.extend(format_domain_alignments(hdr["name"], row[0], by_name.get(row[0], []), display["lines"].get(row[0], {}),
                                                display.get("textw", 120)))
    return _hmmsearch_tail(out, hdr, n_targets, passed, trailer)


def stockholm_row(seq_text, cols, M, flank_at_end=False):
    """One hmmalign row: match columns 0..M-1 in order (uppercase residue or '-'), residues that
    are not in a match column (cols == -1: flanks and inserts) lowercase where they occur.  With
    flank_at_end the residues behind the last match state (the C flank) follow the model's last column,
    where hmmalign itself writes them; the decoded columns are the same either way."""
    parts, c = [], 0
    cols = [int(x) for x in cols]
    last = max([i for i, col in enumerate(cols) if col >= 0], default=len(cols) - 1) if flank_at_end else len(cols) - 1
    for ch, col in zip(seq_text[:last + 1], cols[:last + 1]):
        if col >= 0:
            if col > c:
                parts.append("-" * (col - c))
            parts.append(ch.upper())
            c = col + 1
        else:
            parts.append(ch.lower())
    if M > c:
        parts.append("-" * (M - c))
    if flank_at_end:
        parts.append(seq_text[last + 1:len(cols)].lower())
    return "".join(parts)


def pp_char(p):
    """hmmalign's character for a posterior probability (HMMER's p7_alidisplay_EncodePostProb): '0'..'9' for
    p + 0.05 in [0.0, 0.1) .. [0.9, 1.0), '*' from 0.95 up."""
    p = float(p) + 0.05
    return "*" if p >= 1.0 else chr(ord("0") + int(p * 10.0))


def hmm_has_rf(path):
    """True when the model file's header says "RF yes" (hmmalign then copies the model's own reference line)."""
    opener = open
    if str(path).endswith(".gz"):
        import gzip
        opener = gzip.open
    with opener(path, "rt") as f:
        for line in f:
            w = line.split()
            if w and w[0] == "RF":
                return len(w) > 1 and w[1].lower() == "yes"
            if w and w[0] == "HMM":
                break
    return False


def hmm_display_keys(path):
    """{"CONS", "RF", "CS": bool} of a model file's header: what decides whether its alignments can be displayed."""
    keys = {"CONS": False, "RF": False, "CS": False}
    opener = open
    if str(path).endswith(".gz"):
        import gzip
        opener = gzip.open
    with opener(path, "rt") as f:
        for line in f:
            w = line.split()
            if w and w[0] in keys:
                keys[w[0]] = len(w) > 1 and w[1].lower() == "yes"
            if w and w[0] == "HMM":
                break
    return keys


def stockholm_pp_lines(row, pp, rf=True):
    """The annotation lines of one hmmalign row (stockholm_row) from the per-residue posteriors <pp> (or their
    characters): (PP, PP_cons, RF).  PP: the residue's character, '.' in a gap.  PP_cons of a single sequence: the same
    character in match columns that hold a residue, '.' elsewhere.  RF: 'x' at match columns, '.' at insert columns
    (models without a reference line of their own); None with rf=False."""
    gr, cons, rfl, r = [], [], [], 0
    for ch in row:
        if ch == "-":
            gr.append("."); cons.append("."); rfl.append("x")
        else:
            d = pp[r] if isinstance(pp[r], str) else pp_char(pp[r])
            r += 1
            gr.append(d)
            cons.append(d if ch.isupper() else ".")
            rfl.append("x" if ch.isupper() else ".")
    return "".join(gr), "".join(cons), "".join(rfl) if rf else None


def format_stockholm(name, row, width=200, pp=None, rf=True):
    """Interleaved Stockholm blocks of <width> columns like hmmalign writes.  With <pp> (one posterior probability, or
    its character, per residue of the row) also hmmalign's "#=GR <name> PP", "#=GC PP_cons" and (rf) "#=GC RF" lines,
    the sequence name padded to the longest tag; without it the sequence lines alone."""
    out = ["# STOCKHOLM 1.0", ""]
    if pp is None:
        namew = max(len(name), 1)
        for a in range(0, max(len(row), 1), width):
            out.append("%-*s %s" % (namew, name, row[a:a + width]))
            out.append("")
        out.append("//")
        return "\n".join(out) + "\n"
    gr, cons, rfl = stockholm_pp_lines(row, pp, rf)
    tagw = len("#=GR %s PP" % name)
    blocks = list(range(0, max(len(row), 1), width))
    for a in blocks:
        out.append("%-*s %s" % (tagw, name, row[a:a + width]))
        out.append("%-*s %s" % (tagw, "#=GR %s PP" % name, gr[a:a + width]))
        out.append("%-*s %s" % (tagw, "#=GC PP_cons", cons[a:a + width]))
        if rfl is not None:
            out.append("%-*s %s" % (tagw, "#=GC RF", rfl[a:a + width]))
        if a != blocks[-1]:
            out.append("")
    out.append("//")
    return "\n".join(out) + "\n"


class FormatError(ValueError):
    """An output format format_msa does not write (the server reports it as hmmalign does)."""


MSA_FORMATS = ("stockholm", "pfam", "afa")


def _text(x):
    """A row as str: str, bytes or a uint8 array."""
    if isinstance(x, str):
        return x
    return (x if isinstance(x, (bytes, bytearray)) else bytes(bytearray(x))).decode("ascii")


def read_msa(path):
    """An alignment file, aligned FASTA or Stockholm (told apart by the "# STOCKHOLM" line; Pfam's one block or interleaved
    blocks): {"names", "rows" (one length, the characters as given), "desc": {name: text of its "#=GS name DE" line}}.  Other
    Stockholm annotation is skipped.  ValueError for rows of different lengths, a repeated FASTA name or an empty file."""
    with open(path) as f:
        lines = f.read().splitlines()
    first = next((ln for ln in lines if ln.strip()), "")
    names, rows, desc = [], {}, {}
    if first.startswith("# STOCKHOLM"):
        for ln in lines:
            if ln.startswith("//"):
                break
            w = ln.split(None, 3)
            if ln.startswith("#=GS") and len(w) >= 3 and w[2] == "DE":
                desc[w[1]] = w[3].strip() if len(w) > 3 else ""
            elif ln.strip() and not ln.startswith("#"):
                n, t = ln.split()[:2]
                if n not in rows:
                    names.append(n)
                    rows[n] = []
                rows[n].append(t)
    else:
        for n, t in read_fasta(path):
            if n in rows:
                raise ValueError("alignment file %s: the name %s is repeated" % (path, n))
            names.append(n)
            rows[n] = [t]
    out = ["".join(rows[n]) for n in names]
    if not out or len(set(len(r) for r in out)) != 1 or not out[0]:
        raise ValueError("alignment file %s is empty, or its rows differ in length" % path)
    return {"names": names, "rows": out, "desc": desc}


def format_msa(names, rows, pp_rows, pp_cons, rf, outformat="Stockholm", width=200, desc=None):
    """hmmalign's output for an alignment of several sequences (EHMM.msa: rows, pp_rows [nq][W], pp_cons, rf [W]; str,
    bytes or uint8 arrays; rf None: no "#=GC RF" line, as for a model with a reference line of its own), byte for byte
    HMMER 3.1b2's: "Stockholm" in blocks of <width> columns, every block with its "#=GR PP" and "#=GC" lines; "Pfam" in
    one block; "afa" the rows alone, 60 characters per line.  The format's name is matched without case, as Easel does;
    any other format raises FormatError.  An entry of pp_rows may be None: a row without posteriors (a row of the --mapali
    alignment) gets no "#=GR PP" line.  desc: {name: text}, hmmalign's "#=GS name DE text" block in front of the rows (in
    afa: behind the name)."""
    fmt = str(outformat).lower()
    if fmt not in MSA_FORMATS:
        raise FormatError("%s is not a recognized output MSA file format" % outformat)
    names = list(names)
    rows = [_text(r) for r in rows]
    if fmt == "afa":
        out = []
        for n, r in zip(names, rows):
            out.append(">" + n + (" " + desc[n] if desc and n in desc else ""))
            out.extend(r[a:a + 60] for a in range(0, len(r), 60))
        return "\n".join(out) + "\n" if out else ""
    pps = [None if r is None else _text(r) for r in pp_rows]
    cons = _text(pp_cons)
    rfl = None if rf is None else _text(rf)
    W = len(cons)
    namew = max([len(n) for n in names] + [1])
    margin = max(namew + 1, len("#=GC PP_cons "))                                 # Easel: the widest of the line tags, plus a space
    if any(p is not None for p in pps) or not pps:
        margin = max(margin, namew + len("#=GR  PP "))
    if rfl is not None:
        margin = max(margin, len("#=GC RF "))
    step = W if fmt == "pfam" or W == 0 else width
    out = ["# STOCKHOLM 1.0", ""]
    if desc and any(n in desc for n in names):
        out.extend("#=GS %-*s DE %s" % (namew, n, desc[n]) for n in names if n in desc)
        out.append("")
    starts = list(range(0, max(W, 1), max(step, 1)))
    for a in starts:
        for n, r, p in zip(names, rows, pps):
            out.append("%-*s%s" % (margin, n, r[a:a + step]))
            if p is not None:
                out.append("%-*s%s" % (margin, "#=GR %-*s PP" % (namew, n), p[a:a + step]))
        out.append("%-*s%s" % (margin, "#=GC PP_cons", cons[a:a + step]))
        if rfl is not None:
            out.append("%-*s%s" % (margin, "#=GC RF", rfl[a:a + step]))
        if a != starts[-1]:
            out.append("")
    out.append("//")
    return "\n".join(out) + "\n"


def format_hits_msa(names, row_recs, rows, pp_rows, pp_cons, rf, descriptions=None, notextw=False):
    """The file of hmmsearch -A: the alignment of the included domains (EHMM.hits_msa) as HMMER 3.1b2 writes it.  names: the
    searched records' names by query number; row_recs: per row (query, index, ali_i, ali_j).  A row is named
    "name/ali_i-ali_j" and carries "#=GS <row> DE [subseq from] <the record's description, or its name>"; Stockholm in
    blocks of 200 columns, with --notextw (notextw) in one block.  No rows: HMMER creates the file empty."""
    if len(row_recs) == 0:
        return ""
    descriptions = descriptions or {}
    rnames, desc = [], {}
    for q, _, ai, aj in ((int(r[0]), int(r[1]), int(r[2]), int(r[3])) for r in row_recs):
        rnames.append("%s/%d-%d" % (names[q], ai, aj))
        desc[rnames[-1]] = "[subseq from] %s" % descriptions.get(names[q], names[q])
    return format_msa(rnames, rows, pp_rows, pp_cons, rf, "Pfam" if notextw else "Stockholm", desc=desc)


def hits_msa_trailer(n_rows, path):
    """What hmmsearch says behind "//" about its -A file (path: as given on the command line)."""
    if n_rows == 0:
        return "# No hits satisfy inclusion thresholds; no alignment saved"
    return "# Alignment of %d hits satisfying inclusion thresholds saved to: %s" % (n_rows, path)


def decode_stockholm_row(row):
    """aligner.py:126-142: per residue the 0-based match column or -1."""
    cols, regular = [], 0
    for ch in row:
        if ch == '-':
            regular += 1
        elif ch == '.':
            continue
        elif ch.islower():
            cols.append(-1)
        else:
            cols.append(regular)
            regular += 1
    return cols
