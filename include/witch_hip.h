/*
 * witch_hip.h - C ABI of libwitch_hip.so: MI355X-native query-vs-eHMM scoring,
 * weighting/top-k and optimal-accuracy alignment for WITCH.
 *
 * Every entry point replaces a piece of the reference's HMMER-subprocess path
 * (paths relative to the c5shen/WITCH checkout):
 *
 *   wh_ehmm_load   <- HMMSubset.__init__ reading NSEQ + the HMM text files that
 *                     hmmsearch/hmmalign parse      witch_msa/gcmm/loader.py:17-65
 *   wh_score*      <- SearchAlgorithm.search / subset_frag_chunk_hmmsearch running
 *                     "hmmsearch --cpu 1 --noali -E 99999999 --max" per (HMM, chunk)
 *                     and evalHMMSearchOutput        witch_msa/gcmm/algorithm.py:273-336,482-544,579-605
 *   wh_topk*       <- readAndRankBitscoreMP + calculateWeights/writeWeights
 *                                                    witch_msa/gcmm/loader.py:299-332, weighting.py:58-74,121-169
 *                     and the 0.999 cumulative-weight cut   witch_msa/gcmm/aligner.py:58-63
 *   wh_align*      <- getBackbones running "hmmalign -o OUT HMM QUERY" per chosen HMM
 *                     and decoding the Stockholm row witch_msa/gcmm/aligner.py:96-142
 *   wh_domains*    <- hmmsearch's "Domain annotation for each sequence" section and its --domtblout file; NO reference
 *                     code reads either (evalHMMSearchOutput parses the per-sequence table only): they are here for the
 *                     users of the hmmsearch program the library replaces
 *   wh_hits_msa*   <- "hmmsearch -A FILE": the alignment of all domains that satisfy the inclusion thresholds (HMMER's
 *                     p7_tophits_Alignment); no reference code asks for it either
 *   wh_seq_table*  <- "hmmsearch --tblout FILE": the per-sequence table (HMMER's p7_tophits_TabularTargets), its exp, reg and
 *                     clu columns from wh_seq_expect*; no reference code asks for it either
 *   wh_domain_display* <- hmmsearch's default output, the alignment of every reported domain (HMMER's p7_alidisplay_Create);
 *                     no reference code asks for it either
 *
 * Conventions: plain pointers and sizes; the caller owns every input and output
 * buffer; the library owns wh_ehmm handles and its device workspace.  Functions
 * return 0 on success or a negative WH_E* code; wh_last_error() gives the message of
 * the calling thread's last failure.  Calls on one handle must not overlap.
 * "*_dev" variants take DEVICE pointers and a hipStream_t (passed as void*) and only
 * enqueue work; the plain variants take HOST pointers and block.
 *
 * Data contract:
 *   decibits  int32  [nq x H]  bit-score x 10 exactly as hmmsearch's "%6.1f" prints it
 *   flags     uint8  [nq x H]  WH_FLAG_* (REPORTED = the pair is listed by hmmsearch)
 *   top-k     int32 idx[nq x k] (the caller's hmm_index values, -1 padded),
 *             double w[nq x k] (0 padded), n_kept[nq], n_used[nq] (0.999 prefix length)
 *             ordered by (-weight, -decibits, +hmm_index)
 *   cols      int32, CSR over the residues of each pair: 0-based match column or -1
 */
#ifndef WITCH_HIP_H
#define WITCH_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WH_OK          0
#define WH_EINVAL     -1   /* bad argument                                   */
#define WH_EIO        -2   /* cannot open / parse an HMM file                */
#define WH_ENODEV     -3   /* no usable HIP device                           */
#define WH_EHIP       -4   /* a HIP runtime call failed                      */
#define WH_ERANGE     -5   /* too many pairs in one call (2^31 or more; models and queries: any length.  A query too long for a
                              kernel's LDS plan only under the development knobs WH_NO_LONG_SCORE / WH_NO_RESOLVE)          */
#define WH_ENOMEM     -6   /* device memory: also a call whose workspace for ONE workgroup does not fit (wh_last_error: the figures) */

#define WH_ALPH_DNA    0
#define WH_ALPH_RNA    1
#define WH_ALPH_AMINO  2

#define WH_FLAG_REPORTED  1   /* pair appears in hmmsearch's per-sequence table          */
#define WH_FLAG_MULTI     2   /* a region was multidomain (HMMER's stochastic class)     */
#define WH_FLAG_OVERRIDE  4   /* reconstruction score overrode the Forward score         */
#define WH_FLAG_TRUNC     8   /* part of the pair was left out of its score (never for a well-formed call: see below) */
#define WH_FLAG_EXACT    16   /* an envelope failed the sparse-spill certificate and was redone dense */
#define WH_FLAG_FILTERED 32   /* wh_score_filtered only: an acceleration filter rejected the pair (never with REPORTED) */

/* Envelopes a wh_pair_detail record LISTS.  The SCORE of a pair has no such limit (hmmsearch has none: SURVEY A.4, called at
 * witch_msa/gcmm/algorithm.py:526-532): a pair with more regions than the scoring kernels' list holds is scored a second
 * time inside the same call by the long-list pass (float64 front end with the region list in HBM + a resolver launch of
 * its own; wh_last_score_counters out8[7] counts such pairs), every region and every envelope enters its score, and it
 * comes back WITHOUT WH_FLAG_TRUNC; its detail record lists the first WH_MAX_ENVELOPES envelopes, nregions is the full
 * count.  Nor is there a limit INSIDE a multidomain region: the resolver keeps 32 domains of a sampled trace, 8 192
 * sampled segments and 64 significant clusters of a region in fixed lists; a region that needs more (a tandem repeat of
 * more than 32 copies) is counted to the end, and its pair is scored again inside the same call by the big-region pass -
 * the same resolver with those lists in HBM, sized from the counts (wh_last_region_overflow).  Nor does the resolver limit
 * the QUERY length: its per-wave LDS block holds the query and a state per residue, and a call whose longest query does
 * not fit (beyond ~52 000 residues; ~31 000 with a model of more than 32 767 nodes) sizes its main launches for the
 * lengths that keep their occupancy and resolves the pairs of longer queries in the long-query pass, the same resolver
 * with those two arrays in HBM (wh_last_long_query_pairs).  Nor do the SCORING and ALIGNMENT kernels: their launches keep the
 * query in LDS, and a call whose longest query a size class cannot plan (wh_ehmm_max_query_len: 15 788 - 142 368 residues
 * by model class) sizes them for the lengths every class accepts and hands the pairs of longer queries to the long-query
 * scoring / alignment pass - the any-size float64 kernels, one wavefront per pair, with the residues in HBM beyond ~163 000
 * residues (wh_last_long_score_pairs, wh_last_long_align_pairs).  What remains is the device's memory: one wave's float64 slab
 * grows with query length x model length, and a call whose slab does not fit is refused with WH_ENOMEM before anything is
 * launched.  What can still set WH_FLAG_TRUNC: a malformed record in the resolver's queue (an internal error; a region
 * outside its sequence), more than four million pairs for the long-list pass in one call, or the development knobs
 * WH_NO_LONG_LIST / WH_NO_BIG_REGION / WH_NO_RESOLVE (WH_NO_LONG_QUERY sets no flag: the call runs without the resolver,
 * multidomain regions stay one envelope).  The value stays 8 for binary compatibility. */
#define WH_MAX_ENVELOPES 16

/* Which code path a pair took through the scoring kernels: an optional per-pair record, 16 bits (wh_set_path_buffer16)
 * or the low byte alone (wh_set_path_buffer).  A pair's result does not depend on the path except in the last bits of
 * the float32 null2 correction (window vs full width): the tests draw their oracle samples per path. */
#define WH_PATH_P2_WIN     1   /* regions from the multihit Backward sweep on a node window (certified)  */
#define WH_PATH_P2_FULL    2   /* ... from the full-width sweep (no window fitted, or a decision in doubt) */
#define WH_PATH_P4_W256    4   /* an envelope's Backward sweep kept from a 256-node window                */
#define WH_PATH_P4_W512    8   /* ... from a 512-node window                                              */
#define WH_PATH_P4_WFAIL  16   /* a window failed the mass certificate and was redone at full width       */
#define WH_PATH_P4_FULL   32   /* an envelope's Backward sweep at full width                              */
#define WH_PATH_DENSE     64   /* an envelope redone with every Forward row stored (WH_FLAG_EXACT)        */
#define WH_PATH_MULTI    128   /* finished by the multidomain resolver                                    */
/* ... and what was stored of an envelope's Forward rows (16-bit record only; the three attempts: envelope_attempts,
 * wh_score7.hip): */
#define WH_PATH_BAND_KEPT 256  /* an envelope accepted from the banded store (lane blocks around P1's dominant path) */
#define WH_PATH_BAND_FAIL 512  /* an envelope's band failed its mass certificate and the rows were stored again
                                  unbanded - whether that store was then accepted or the dense one followed (then
                                  WH_PATH_DENSE is set as well).  An envelope without a band sets neither bit.       */

typedef struct wh_ehmm wh_ehmm;

/* Optional per-pair diagnostics (tests compare them with the oracle stage by stage). */
typedef struct wh_pair_detail {
  float   fwd_bits;        /* (Forward - null1) / ln 2, multihit local               */
  float   seq_score;       /* final float32 score before the deci-bit print          */
  float   pre_score;       /* score before the null2 correction                      */
  float   seqbias_nats;
  int32_t nregions;
  int32_t nenv;
  int32_t env_i[WH_MAX_ENVELOPES];
  int32_t env_j[WH_MAX_ENVELOPES];
  float   envsc[WH_MAX_ENVELOPES];      /* nats */
  float   domcorr[WH_MAX_ENVELOPES];    /* nats */
} wh_pair_detail;

const char *wh_version(void);
const char *wh_last_error(void);

/* Select the HIP device for the calling process (one process per GPU). */
int wh_init(int device);
int wh_device_info(char *name, int name_len, int *cu_count, int64_t *hbm_bytes);

/* Digitise text residues with HMMER/Easel's alphabet rules (case-insensitive, U->T,
 * X->N for nucleic acids).  Codes >= K are degenerate; 255 marks an illegal character. */
int wh_digitize(int alphabet, const char *text, int64_t n, uint8_t *out);

/* Parse n HMMER3/f text models, configure the local profiles and upload them.
 * hmm_index[i] is the caller's label for model i (WITCH's A_0_<idx>); nseq may be NULL
 * (then NSEQ from each file header is used, as loader.py:48-53 does). */
wh_ehmm *wh_ehmm_load(const char *const *hmm_paths, const int32_t *hmm_index, const int32_t *nseq, int n);
void     wh_ehmm_free(wh_ehmm *e);
int      wh_ehmm_count(const wh_ehmm *e);
int      wh_ehmm_alphabet(const wh_ehmm *e);
int      wh_ehmm_info(const wh_ehmm *e, int32_t *M, int32_t *nseq, int32_t *hmm_index);
/* MAP annotation of model h: alignment column (1-based) of match state k=1..M, 0 if absent. */
int      wh_ehmm_map(const wh_ehmm *e, int h, int32_t *map_cols);
/* The length up to which the queries of a call stay on the float32 kernels, in scoring and in alignment: the largest
 * length every launch of the handle's size classes can plan (phase-call, pass-synchronous and several-waves-per-pair
 * kernels alike).  A call with a longer query is served all the same - the pairs of the longer queries by the long-query
 * passes (float64, one wavefront per pair: correct, not fast) - so this is a performance figure, not a limit.
 * wh_query_len_cap gives the same figure (default knobs) from the node counts alone, without a handle or a device. */
int      wh_ehmm_max_query_len(const wh_ehmm *e);
int      wh_query_len_cap(int alphabet, const int32_t *model_nodes, int n);

/* All-vs-all scoring: nq queries (digital residues, CSR offsets[nq+1]) x H models.  One call serves fewer than 2^31
 * pairs (WH_ERANGE beyond: feed the queries in chunks, as the reference feeds hmmsearch 20 000 sequences at a time,
 * witch_msa/gcmm/algorithm.py:209,280-284; witch_amd.gcmm.QueryAlignmentEngine.run does). */
int wh_score(wh_ehmm *e, const uint8_t *residues, const int64_t *offsets, int64_t nq,
             int32_t *decibits, uint8_t *flags, float *fwd_bits, wh_pair_detail *detail);
int wh_score_dev(wh_ehmm *e, const uint8_t *d_residues, const int64_t *d_offsets, int64_t nq,
                 int64_t total_residues, int32_t max_len,
                 int32_t *d_decibits, uint8_t *d_flags, float *d_fwd_bits, wh_pair_detail *d_detail,
                 void *stream);

/* Weights over the reported models of each query, deterministic top-k and 0.999 prefix. */
int wh_topk(wh_ehmm *e, const int32_t *decibits, const uint8_t *flags, int64_t nq, int k,
            int32_t *idx, double *w, int32_t *n_kept, int32_t *n_used);
int wh_topk_dev(wh_ehmm *e, const int32_t *d_decibits, const uint8_t *d_flags, int64_t nq, int k,
                int32_t *d_idx, double *d_w, int32_t *d_n_kept, int32_t *d_n_used, void *stream);

/* Optimal-accuracy alignment of query pair_q[p] against model position pair_h[p]
 * (0..H-1, the position in the load order, not the hmm_index label).
 * cols is CSR: pair p writes cols[col_offsets[p] .. col_offsets[p] + len(query)). */
int wh_align(wh_ehmm *e, const uint8_t *residues, const int64_t *offsets, int64_t nq,
             const int64_t *pair_q, const int32_t *pair_h, int64_t npairs,
             const int64_t *col_offsets, int32_t *cols);
int wh_align_dev(wh_ehmm *e, const uint8_t *d_residues, const int64_t *d_offsets, int64_t nq,
                 int64_t total_residues, int32_t max_len,
                 const int64_t *d_pair_q, const int32_t *d_pair_h, int64_t npairs,
                 const int64_t *d_col_offsets, int32_t *d_cols, void *stream);

/* The same alignment with hmmalign's per-residue confidence (its "#=GR <name> PP" line): pp is CSR by the same
 * col_offsets as cols, one float per residue - the posterior probability that residue i was emitted by the state the
 * returned path puts it in: M_k where cols >= 0, else I_k (an insert) or N / C (a flank residue; J cannot occur, the
 * alignment profile is unihit).  pp == NULL is wh_align / wh_align_dev: same columns, same launches, same workspace.
 * Nothing outside the pairs' ranges is written.  A pair returned without a path (all columns -1) gets 0 for every
 * residue; a pair that a later pass of the call aligns again (several-waves -> any-size hand-over, long-query pass)
 * carries that pass's values.
 * Precision, by the kernel that aligned the pair:
 *  - register kernels (models of up to 3 072 nodes) and the several-waves kernel: float32 Forward x Backward / Z, within
 *    2e-4 + 3e-6 L of a float64 evaluation (measured: 3e-6).  A pair aligned on a node window (wh_last_align_paths)
 *    carries LOWER BOUNDS: the mass certificate lets a window drop 3e-6 * L (kAlnWinTol * L) of posterior mass in total
 *    over the pair, so no value is more than that below the full-width one.
 *  - a pair that leaves float32 range (n_logspace of wh_last_align_status; typically several copies of a long family in
 *    one query): with pp == NULL it is redone by the float32 log-space pass, whose posteriors - differences of
 *    logarithms of thousands of nats - are good to a few percent only; they are NOT returned.  A call with pp hands such
 *    a pair to the float64 any-size kernel instead, like every pair that kernel serves anyway (models beyond 3 072
 *    nodes, the long-query pass): float64 throughout, in log space where needed, within 5e-16 L^2 of exact (1e-9 for
 *    the pairs in probability space), rounded to float once at the store: 2^-25 = 3e-8 below 1.  The columns are
 *    hmmalign's from either kernel.
 * witch_amd.shim.formats.pp_char turns a value into hmmalign's character. */
int wh_align_pp(wh_ehmm *e, const uint8_t *residues, const int64_t *offsets, int64_t nq,
                const int64_t *pair_q, const int32_t *pair_h, int64_t npairs,
                const int64_t *col_offsets, int32_t *cols, float *pp);
int wh_align_pp_dev(wh_ehmm *e, const uint8_t *d_residues, const int64_t *d_offsets, int64_t nq,
                    int64_t total_residues, int32_t max_len,
                    const int64_t *d_pair_q, const int32_t *d_pair_h, int64_t npairs,
                    const int64_t *d_col_offsets, int32_t *d_cols, float *d_pp, void *stream);
/* The same with pp as doubles.  What the float32 kernels return is their float32 value widened; the any-size float64
 * kernel (models beyond 3 072 nodes, the long-query pass, pairs handed over by the several-waves kernel) returns its
 * float64 posterior unrounded - a float holds a value below 1 only to 2^-25 = 3e-8. */
int wh_align_pp64(wh_ehmm *e, const uint8_t *residues, const int64_t *offsets, int64_t nq,
                  const int64_t *pair_q, const int32_t *pair_h, int64_t npairs,
                  const int64_t *col_offsets, int32_t *cols, double *pp);
int wh_align_pp64_dev(wh_ehmm *e, const uint8_t *d_residues, const int64_t *d_offsets, int64_t nq,
                      int64_t total_residues, int32_t max_len,
                      const int64_t *d_pair_q, const int32_t *d_pair_h, int64_t npairs,
                      const int64_t *d_col_offsets, int32_t *d_cols, double *d_pp, void *stream);
/* wh_align_pp[_dev] under a length model of the caller's choice: cfg_len[nq] (int32, >= 1) is, per query, the number of
 * residues the unihit length model of its pairs is configured for - the N and C loops are cfg_len / (cfg_len + 2) where
 * wh_align_pp takes the query's own length.  That is how hmmsearch aligns an envelope: as Ld residues under the length model
 * of the whole sequence of L (cfg_len = L), which equals aligning the envelope followed by L - Ld residues that every state
 * emits with odds 1.  Only the length configuration changes: rows, workspace, launch planning, node windows and the
 * hand-overs follow the residues given, and the precision is wh_align_pp's.  cfg_len == NULL is wh_align_pp[_dev] itself,
 * bit for bit.  The host-pointer variant refuses an entry < 1 (WH_EINVAL, wh_last_error names the query); the _dev variant
 * does not read the array on the host, and its kernels take an entry < 1 as 1. */
int wh_align_pp_len(wh_ehmm *e, const uint8_t *residues, const int64_t *offsets, int64_t nq,
                    const int64_t *pair_q, const int32_t *pair_h, int64_t npairs,
                    const int64_t *col_offsets, int32_t *cols, float *pp, const int32_t *cfg_len);
int wh_align_pp_len_dev(wh_ehmm *e, const uint8_t *d_residues, const int64_t *d_offsets, int64_t nq,
                        int64_t total_residues, int32_t max_len,
                        const int64_t *d_pair_q, const int32_t *d_pair_h, int64_t npairs,
                        const int64_t *d_col_offsets, int32_t *d_cols, float *d_pp, const int32_t *d_cfg_len, void *stream);

/* ---- per-domain results (hmmsearch's "Domain annotation for each sequence" section and --domtblout; no reference code
 * calls either - witch_msa reads the per-sequence table alone) -------------------------------------------------------
 * A DOMAIN is an envelope of a reported pair, as wh_score lists it in the pair's wh_pair_detail record.  Its ALIGNMENT is
 * wh_align_pp's alignment of the envelope's residues env_i..env_j against the pair's model - hmmalign's optimal-accuracy
 * alignment under the unihit length model of Ld = env_j - env_i + 1 residues.  On domains that HMMER prints with an
 * accuracy of 0.95 or more that is hmmsearch's own alignment, coordinate for coordinate; on weaker ones hmmsearch usually
 * prints the same alignment with columns trimmed at an end (the agreement per stratum).
 * That is the default, WH_LENMODEL_ENVELOPE.  Under wh_set_domain_length_model(e, WH_LENMODEL_SEQUENCE) the envelope is aligned
 * under the length model of its whole sequence of L residues (wh_align_pp_len with cfg_len = L), as hmmsearch does it: ali_*,
 * hmm_*, oasc, the columns and the posteriors are then hmmsearch's on the weak domains too; env_*, bits, bias_bits and lnP do
 * not depend on the alignment and are the same bits under either setting.
 * bits, bias_bits and lnP follow HMMER's float32 arithmetic (L: the query's length):
 *   bits = (envsc + (L - Ld) ln(L / (L + 3)) - nullsc - dombias) / ln 2,  nullsc = L ln(L / (L + 1)) + ln(1 / (L + 1)),
 *   dombias = logsum(0, ln(1 / 256) + domcorr),  bias_bits = dombias / ln 2,  lnP = min(0, -lambda (bits - tau))
 * with tau, lambda from the model's STATS LOCAL FORWARD line (wh_ehmm_evparams).  The E-values are the caller's:
 * i-Evalue = exp(lnP) Z (Z: number of targets), c-Evalue = exp(lnP) domZ (domZ: number of reported targets). */
typedef struct wh_domain {
  int64_t pair;            /* q * H + h                                                        */
  int32_t index, of;       /* 0-based among the pair's envelopes; the pair's envelope count as far as the detail record tells
                              it (HMMER's "#" - 1 and "of"): see wh_domain_counts for its two limits                       */
  int32_t env_i, env_j;    /* 1-based, as in wh_pair_detail                                     */
  int32_t ali_i, ali_j;    /* first / last residue of the query in a match state; 0, 0: no path */
  int32_t hmm_i, hmm_j;    /* their nodes, 1-based                                              */
  float   bits, bias_bits; /* HMMER's per-domain score and bias                                 */
  float   oasc;            /* sum of the path's posteriors over the envelope; acc = oasc / Ld   */
  float   lnP;             /* min(0, -lambda (bits - tau)); NaN for a model without a STATS LOCAL FORWARD line */
} wh_domain;

/* Domains per pair, from the flags and detail records of a wh_score call over nq queries: counts[nq x H] =
 * min(nenv, WH_MAX_ENVELOPES) for a pair with WH_FLAG_REPORTED, else 0.  The caller turns the counts into the CSR
 * dom_off[nq x H + 1].  n_unlisted[nq x H] (optional) and a record's "of" say what the detail record lets them say about the
 * envelopes beyond its list, which entered the pair's score and which no domain record describes.  The scoring kernels cap
 * nenv at WH_MAX_ENVELOPES and export the full count of REGIONS only (nregions), so there are two limits:
 *  - a pair of the long-list pass (nregions > WH_MAX_ENVELOPES): of = nregions, n_unlisted = nregions - WH_MAX_ENVELOPES -
 *    regions, not envelopes: exact when each region of the pair is one envelope, a lower bound otherwise;
 *  - a pair with at most WH_MAX_ENVELOPES regions but more envelopes than that (one multidomain region that the resolver
 *    splits many times, such as a tandem repeat of 17 or more copies): of = WH_MAX_ENVELOPES and n_unlisted = 0 although
 *    envelopes are missing from the list - the records cannot tell such a pair from one with exactly 16 envelopes.
 * Every other pair: of = nenv, n_unlisted = 0. */
int wh_domain_counts(wh_ehmm *e, const uint8_t *flags, const wh_pair_detail *detail, int64_t nq,
                     int32_t *counts, int32_t *n_unlisted);
int wh_domain_counts_dev(wh_ehmm *e, const uint8_t *d_flags, const wh_pair_detail *d_detail, int64_t nq,
                         int32_t *d_counts, int32_t *d_n_unlisted, void *stream);
/* The domain records of a scoring call: the same residues / offsets / nq, its flags and detail records, and dom_off
 * [nq x H + 1], the exclusive prefix sums of wh_domain_counts' counts (checked against the records: WH_EINVAL otherwise, as
 * for an envelope outside its query).  out[dom_off[nq x H]]: the domains of pair p at dom_off[p] .. dom_off[p + 1], in envelope
 * order.  Three kernels around one wh_align_pp_dev call on the packed envelopes (envelopes of one pair may overlap, so they are
 * copied): the launch planning, node windows, log-space and any-size hand-overs of that call serve as they are, and
 * wh_last_align_status / _paths / wh_last_kernel_ms(2) then describe the domains' alignments.  The _dev variant reads
 * dom_off's last entry and the envelope lengths back (it waits for the stream twice before the alignment, which waits itself,
 * as wh_align_dev does); max_len: the longest query, which no envelope may exceed (WH_EINVAL); total_residues is not read. */
int wh_domains(wh_ehmm *e, const uint8_t *residues, const int64_t *offsets, int64_t nq,
               const uint8_t *flags, const wh_pair_detail *detail, const int64_t *dom_off, wh_domain *out);
int wh_domains_dev(wh_ehmm *e, const uint8_t *d_residues, const int64_t *d_offsets, int64_t nq,
                   int64_t total_residues, int32_t max_len,
                   const uint8_t *d_flags, const wh_pair_detail *d_detail, const int64_t *d_dom_off, wh_domain *d_out,
                   void *stream);
/* The length model the domain stage aligns an envelope under - handle state, for production use (no development knob):
 * WH_LENMODEL_ENVELOPE (the default): the envelope's own Ld residues, hmmalign's alignment of the envelope;
 * WH_LENMODEL_SEQUENCE: the L residues of the envelope's sequence, hmmsearch's own alignment.  Under the latter the stage's
 * list kernel also writes each domain's sequence length, and the stage's one alignment call passes that array as d_cfg_len.
 * Everything behind that call follows: wh_domains*, wh_domain_paths*, wh_hits_msa and wh_domain_display.  Any other value:
 * WH_EINVAL.  wh_get_domain_length_model returns the setting (WH_EINVAL for a null handle).  Neither needs the device. */
#define WH_LENMODEL_ENVELOPE 0
#define WH_LENMODEL_SEQUENCE 1
int wh_set_domain_length_model(wh_ehmm *e, int model);
int wh_get_domain_length_model(const wh_ehmm *e);
/* The Forward E-value parameters of every model, from its "STATS LOCAL FORWARD tau lambda" line (hmmbuild writes it, as
 * does wh_hmmbuild2 / wh_hmmbuild_batch with WH_BUILD_STATS): tau[H], lambda[H], present[H] (each optional); a model without
 * the line loads as before and has present = 0, tau = lambda = NaN.  Needs no device. */
int wh_ehmm_evparams(const wh_ehmm *e, float *tau, float *lambda, int32_t *present);
/* The same for one model file, through the same parser, without a handle (wh_ehmm_load needs a device, this does not). */
int wh_hmm_evparams(const char *hmm_path, float *tau, float *lambda, int32_t *present);

/* ---- hmmsearch's acceleration filters (hmmsearch WITHOUT --max: MSV filter -> bias filter -> Viterbi filter -> Forward) ----
 * Per (query of length L, model), as HMMER 3.1b2's pipeline decides, with null1 = L ln(L / (L + 1)) + ln(1 / (L + 1)):
 *   1. MSV      P = gumbel_surv((usc - null1) / ln 2; mu_MSV, lambda)        rejected where P > F1; a filter overflow passes
 *   2. bias     OPT-IN (nobias = WH_BIAS_FILTER_ON).  filtersc = the float32 scaled Forward score of the query on a two-state
 *               HMM (background; the model's composition, its COMPO line, staying L1 = M / 8 residues on average) plus the
 *               length terms of null1, as p7_bg_FilterScore computes it;  P = gumbel_surv((usc - filtersc) / ln 2; mu_MSV,
 *               lambda), rejected where P > F1.  With nobias = 1 the pipeline runs as "hmmsearch --nobias" does:
 *               filtersc = null1 and the stage passes with stage 1.  nobias = 0 is STILL REFUSED with WH_EINVAL: a later
 *               change makes 0 mean WH_BIAS_FILTER_ON (HMMER's default) and retires the refusal.
 *   3. Viterbi  only where the last P > F2:  P = gumbel_surv((vfsc - filtersc) / ln 2; mu_VIT, lambda), rejected where P > F2
 *   4. Forward  P = exp_surv((fwdsc - filtersc) / ln 2; tau, lambda), rejected where P > F3 (wh_score_filtered only)
 * mu, tau, lambda: the model's three "STATS LOCAL" lines; a model without them cannot be filtered (WH_EINVAL, the message
 * names it).  The two filters are integer dynamic programmes (8-bit, 16-bit): the device's raw scores are the host's and
 * HMMER's to the bit, and every decision is a comparison of float32 scores that both sides compute with correctly
 * rounded operations alone - wh_filter and wh_filter_host agree bit for bit.
 * With the bias filter on, device and host also agree bit for bit on filtersc: one float32 recurrence without fused
 * operations, its logarithms from + - x / on float64 alone (no libm on either side).
 * opts == NULL: HMMER's defaults, F1 = 0.02, F2 = 1e-3, F3 = 1e-5, nobias = 0 (so: refused until the bias filter is the
 * default; pass nobias = 1 or WH_BIAS_FILTER_ON; any other value is WH_EINVAL).  F >= 1 switches a stage off.
 * stage[nq x H], in the scoring calls' pair order: bit 0 passed MSV, 1 passed bias, 2 passed Viterbi (also set where the
 * sweep was skipped because the pair was below F2 already), 3 the Viterbi sweep ran, 4 passed Forward (wh_score_filtered
 * only).  An empty query fails every stage.  filter_bias_nats (optional) = filtersc - null1: 0 with nobias = 1, and where
 * the bias filter did not run (a pair rejected by the MSV stage).
 * msv_raw / vit_raw (optional): the filters' raw integer results - MSV xJ (-1: overflow), Viterbi xC (32768: overflow,
 * -32768: no path, -32769: the sweep did not run). */
#define WH_BIAS_FILTER_ON 2   /* wh_filter_opts.nobias: run the bias filter (1: hmmsearch --nobias; 0: refused for now) */
typedef struct wh_filter_opts { double F1, F2, F3; int32_t nobias; } wh_filter_opts;
int wh_filter(wh_ehmm *e, const uint8_t *residues, const int64_t *offsets, int64_t nq, const wh_filter_opts *opts,
              uint8_t *stage, float *filter_bias_nats, int32_t *msv_raw, int32_t *vit_raw);
/* max_len: the longest query (a longer one gets stage 128 and nothing else); total_residues is not read */
int wh_filter_dev(wh_ehmm *e, const uint8_t *d_residues, const int64_t *d_offsets, int64_t nq, int64_t total_residues, int32_t max_len,
                  const wh_filter_opts *opts, uint8_t *d_stage, float *d_filter_bias_nats, int32_t *d_msv_raw, int32_t *d_vit_raw,
                  void *stream);
/* The same pipeline as plain scalar code over the n model files: no handle (wh_ehmm_load needs a device) and no HIP call - the
 * reference of the kernels, for a build without a GPU.  counts4 (optional): pairs, passed MSV, passed bias, passed Viterbi. */
int wh_filter_host(const char *const *hmm_paths, int n, const uint8_t *residues, const int64_t *offsets, int64_t nq,
                   const wh_filter_opts *opts, uint8_t *stage, float *filter_bias_nats, int32_t *msv_raw, int32_t *vit_raw,
                   int64_t *counts4);
/* wh_score behind the filters: the filters run on every pair, the queries with at least one pair past stage 3 are compacted
 * on the device and scored by the EXISTING scoring path (all H models of such a query: correct, partial savings; with one
 * model only survivors are scored), the results are scattered back and stage 4 is applied from fwd_bits.  A pair past all
 * four stages carries exactly wh_score's decibits, flags, fwd_bits and detail.  A pair that a stage rejected: flags =
 * WH_FLAG_FILTERED alone, decibits = 0, detail zeroed (fwd_bits: its value where the pair was scored, else 0).  stage is
 * optional.  The _dev variant waits for the stream once (it reads the surviving queries back), then as wh_score_dev does. */
int wh_score_filtered(wh_ehmm *e, const uint8_t *residues, const int64_t *offsets, int64_t nq, const wh_filter_opts *opts,
                      int32_t *decibits, uint8_t *flags, float *fwd_bits, wh_pair_detail *detail, uint8_t *stage);
int wh_score_filtered_dev(wh_ehmm *e, const uint8_t *d_residues, const int64_t *d_offsets, int64_t nq, int64_t total_residues,
                          int32_t max_len, const wh_filter_opts *opts, int32_t *d_decibits, uint8_t *d_flags, float *d_fwd_bits,
                          wh_pair_detail *d_detail, uint8_t *d_stage, void *stream);
/* The last wh_filter / wh_score_filtered call on the handle: out[0] = pairs, [1] passed MSV, [2] passed bias, [3] passed
 * Viterbi, [4] passed Forward, [5] pairs handed to the scoring kernels ([4], [5]: 0 after wh_filter).  Waits for the device. */
int wh_last_filter_counts(wh_ehmm *e, int64_t out[6]);
/* Test hook of the bias filter's logarithm (float64 arithmetic alone, the same code on host and device): the number of
 * float32 bit patterns in [first, last] on which it differs from (float) log((double) x) of the host's libm. */
int64_t wh_filter_log_differences(uint32_t first, uint32_t last);

/* Outcome classes of the last wh_align / wh_align_dev call on this handle (the call itself returns WH_OK for
 * them): n_logspace = pairs that left the float range and were redone in log space (same columns as hmmalign's
 * own log-space fallback); n_unaligned = pairs returned with ALL columns -1 where hmmalign (aligner.py:96-142) would
 * have produced an alignment: always 0 since round 5 (a pair on a model of more than 3072 nodes whose log-space Forward
 * and Backward scores disagree used to be dropped; it is now aligned from the Forward-normalised posteriors, as hmmalign
 * does, counted in n_logspace and noted on stderr).  The argument stays for binary compatibility; unaligned_pairs is
 * not written. */
int wh_last_align_status(wh_ehmm *e, int64_t *n_logspace, int64_t *n_unaligned, int64_t *unaligned_pairs, int64_t cap);

/* Which sweeps the register-kernel pairs (models of up to 3072 nodes) of the last wh_align / wh_align_dev call went
 * through - same columns either way, the split only prices the call (bench.py):
 * paths4[0] = Backward / posteriors / OA / traceback on a 256-node window around the dominant path, [3] = on a
 * 512-node window, [1] = window result not accepted (mass certificate) and redone at full width, [2] = full width
 * from the start (query too long for a window, no dominant path, models of fewer than 8 nodes per lane). */
int wh_last_align_paths(wh_ehmm *e, int64_t *paths4);

/* How the Backward sweeps of the last wh_score call ran, counted on the device by the one-wavefront-per-pair scoring
 * kernels (models of up to 24 cells per lane; the pass-synchronous, several-waves-per-pair and any-size kernels have no
 * window and are not counted).  Envelope sweeps (unihit Backward + posterior accumulation -> null2):
 * paths6[0] = envelopes whose sweep ran on a 256-node window around the dominant alignment and passed the mass
 * certificate, [1] = the same on a 512-node window, [2] = windows that failed the certificate (each then ran again at
 * full width), [3] = full-width sweeps (no window tried, a failed window, or the dense redo of a sparse spill).
 * Multihit sweeps (Backward + domain decoding): [4] = pairs whose regions come from a sweep on a node
 * window (every threshold decision of the region scan beyond the window's slack), [5] = pairs whose window left a
 * decision in doubt and whose sweep ran again at full width (pairs that never tried a window are in neither).
 * Waits for the device.  (What a window is: DESIGN.md section 4.1; WH_NO_WINDOW switches both off.) */
int wh_last_score_paths(wh_ehmm *e, int64_t *paths6);
/* The same six counters and, in out8[6], the BYTES of Forward rows the envelope sweeps of the last scoring call stored to
 * their slabs (lane blocks kept by the sparse spill x 8 bytes per cell: what the kernels ASKED the memory system to write,
 * counted on the device with one scalar add per row; the Backward sweeps read about three quarters of it back).  bench.py
 * reports it live beside the HBM-level traffic of the stamped profile: a regression of the spill shows in the driver's own
 * line (one-wavefront-per-pair kernels only).  out8[7] = pairs of the last call that went through the long-list pass
 * (more regions than WH_MAX_ENVELOPES; see there). */
int wh_last_score_counters(wh_ehmm *e, int64_t *out8);
/* The big-region pass of the last scoring call: out4[0] = pairs it scored again because one multidomain region needed
 * longer lists than the resolver's fixed ones (see WH_MAX_ENVELOPES), out4[1] = the most domains in one sampled trace,
 * [2] = the most sampled segments and [3] = the most significant clusters of such a region (0 where that list was long
 * enough).  All 0: no pair went through the pass, which then cost nothing beyond four ints in the call's one read-back. */
int wh_last_region_overflow(wh_ehmm *e, int64_t *out4);
/* The long-query pass of the last scoring call: out[0] = pairs it resolved because their query is longer than the length
 * cap of the resolver's main launches (only in a call whose longest query does not fit the resolver's LDS block), out[1] =
 * the longest query among them.  Both 0: no pair went through the pass (two more ints in the call's one read-back). */
int wh_last_long_query_pairs(wh_ehmm *e, int64_t out[2]);
/* The long-query scoring pass of the last scoring call: out[0] = pairs it scored because their query is longer than the
 * length cap of the call's scoring launches (every model of every such query; only in a call whose longest query a size
 * class cannot plan, or under the development knob WH_SCORE_LMAIN), out[1] = the longest query among them.  Both 0: no
 * pair went through the pass, and the call made no launch and no read-back for it.  wh_last_long_align_pairs: the same
 * for the last wh_align call (pairs on models of up to 3 072 nodes handed to the any-size float64 alignment kernel). */
int wh_last_long_score_pairs(wh_ehmm *e, int64_t out[2]);
int wh_last_long_align_pairs(wh_ehmm *e, int64_t out[2]);

/* Optional per-PAIR record of the same, 8 bits: a device array of nq x H bytes that the scoring calls made after this one
 * fill with the low eight WH_PATH_* bits (NULL switches it off again).  Written by the staged launches only
 * (WH_SCORE_KERNEL=10 / 11; pairs of the other kernels keep whatever the array held; under 10 the envelopes run fused
 * and the record carries the P2 and resolver bits alone).  The buffer belongs to the caller and must stay valid for as
 * many pairs as the calls score.  tests/test_gpu_parity.py draws its headline-size oracle samples per path from it. */
int wh_set_path_buffer(wh_ehmm *e, uint8_t *d_paths);
/* The 16-bit record: a device array of nq x H uint16_t that every scoring kernel of a call fills, the default fused kernel
 * included - one store per pair beside the pair's flags, so no pair keeps what the array held (NULL switches it off again;
 * the kernels then take a wave-uniform branch around the record).  The low byte has the bits above, bits 8 and 9 are
 * WH_PATH_BAND_KEPT / WH_PATH_BAND_FAIL.  An empty or unscored pair gets 0.
 *  - score_kernel7 (the default for models of up to 24 cells per lane) derives the bits from what it counts anyway: a path
 *    counter that moved while the pair was scored is a bit;
 *  - the staged launches (WH_SCORE_KERNEL=10 / 11) record each sweep where it runs; the low byte is what wh_set_path_buffer
 *    gets in the same call;
 *  - the kernels without windows or bands (pass-synchronous, several waves per pair, the any-size float64 front end with
 *    its long-list and long-query scoring passes): WH_PATH_P2_FULL | WH_PATH_P4_FULL for a pair with an envelope,
 *    WH_PATH_DENSE with WH_FLAG_EXACT, WH_PATH_MULTI for a pair they queue for the resolver (the any-size front end queues
 *    every pair with a region).  A pair that a later pass of the same call scores again carries that pass's record.
 * Not written by the opt-in schedules WH_SCORE_KERNEL=9 and 12 (two queries per wave, four envelopes per sweep): their
 * pairs keep what the array held.  Both buffers may be set; each is filled by its own rule. */
int wh_set_path_buffer16(wh_ehmm *e, uint16_t *d_paths);

/* Scoring passes the last wh_score call REPEATED (0 to 2: the loop in wh_score_dev allows two repeats, and a pass repeated
 * because a staged batch ran out of envelope units - WH_SCORE_KERNEL=10 / 11 - counts as well).  The queue that hands pairs with a multidomain region to the
 * resolver stage is sized by estimate (5 % of the pairs, or 1.25 x the largest share an earlier call on the handle
 * queued); a call that needs more slots counts them, grows the queue and scores once more - same results, about twice
 * the scoring time of that one call.  Negative: error. */
int wh_last_queue_reruns(wh_ehmm *e);

/* Weighted consensus of each query's per-HMM alignments (witch-ng merge DP; replaces the Python
 * loops of alignSubQueriesNew, witch_msa/gcmm/aligner.py:376-473).  Pairs are grouped by
 * query in top-k order: query q owns pairs qpair_off[q] .. qpair_off[q+1]; pair p aligned
 * the query to model pair_h[p] (position 0..H-1) with weight pair_w[p] and per-residue match
 * columns cols[col_offsets[p] ..] as produced by wh_align.  retained / nongaps are the
 * reference's subset_to_retained_columns / subset_to_nongaps_per_column
 * (witch_msa/gcmm/algorithm.py:423-429), CSR over models by ret_off[H+1].
 * out (CSR by <offsets>, one int per residue): backbone column >= 0 for a match, -1 - nc for
 * an insertion placed before backbone column nc.  minmax[2q], minmax[2q+1]: first/last
 * backbone column touched (max < 0: nothing aligned). */
int wh_consensus(wh_ehmm *e, const int64_t *offsets, int64_t nq, const int64_t *qpair_off,
                 const int32_t *pair_h, const double *pair_w, const int64_t *col_offsets, const int32_t *cols,
                 const int64_t *ret_off, const int32_t *retained, const int32_t *nongaps,
                 int32_t backbone_length, int32_t *out, int32_t *minmax);
int wh_consensus_dev(wh_ehmm *e, const int64_t *d_offsets, int64_t nq, int32_t max_len, const int64_t *d_qpair_off,
                     const int32_t *d_pair_h, const double *d_pair_w, const int64_t *d_col_offsets,
                     const int32_t *d_cols, const int64_t *d_ret_off, const int32_t *d_retained,
                     const int32_t *d_nongaps, int32_t backbone_length, int32_t max_pairs_per_query,
                     int32_t *d_out, int32_t *d_minmax, void *stream);

/* Duration (ms) and launch count of the kernels of the last *_dev/plain call, measured
 * with HIP events on the stream the kernels ran on: which = 0 scoring kernels, 1 topk, 2 align, 3 consensus,
 * 4 multidomain resolver (the second part of wh_score: stage time of scoring = 0 + 4), 5 the domain stage (wh_domains: its
 * gather and summary kernels and the alignment launches between them; which = 2 then holds the alignment launches alone),
 * 6 the alignment assembly (wh_msa_dev: widths, layout, render and PP_cons kernels, and the host's one wait between them),
 * 7 the --mapali mapping (wh_msa_mapali_dev: count and map kernels, and the host's one wait between them),
 * 8 the hit selection of hmmsearch -A (wh_hits_msa_dev: mark, scan, place and slice kernels, and the host's one wait between them),
 * 9 the alignment display (wh_domain_display_dev: count, scan and render kernels, and the host's one wait between count and render). */
int wh_last_kernel_ms(wh_ehmm *e, int which, double *ms, int *launches);
/* Timing mode only: the scoring launches of the last wh_score[_dev] call, in launch order - the cells-per-lane class of the
 * launch's models (16 = models of 961..1024 nodes ...), the kernel family (0 phase-call wh::k7::score_kernel7, 1
 * pass-synchronous wh::score_big_kernel, 2 any-size wh::generic_front_kernel, 3 several-waves-per-pair wh::wide::score_wide_kernel with
 * cells_per_lane = (cells per virtual lane: 12, 16, 24 or 48) x waves) and its HIP-event duration.  Returns the number
 * of launches (the first <cap> are written); bench.py names the measured dominant kernel from it. */
int wh_last_score_launches(wh_ehmm *e, int32_t *cells_per_lane, int32_t *kind, double *ms, int cap);
/* The launch shape of the one-wavefront-per-pair scoring launches (models of up to 24 cells per lane) of the last scoring
 * pass, in launch order, timing mode or not: the cells-per-lane class, the waves per workgroup (16 = four per SIMD, the
 * 1 024-thread object wh::k7w::score_kernel7; 12 or fewer = wh::k7::score_kernel7 and the other families) and how the
 * multihit Backward sweep tries its node window: 0 not at all, 1 with three more rows per wave in LDS, 2 in place with the
 * Forward sweep's rows backed up in HBM (DESIGN.md sections 4.1 and 9.12).  Returns the number of launches (the first <cap>
 * are written; any of the arrays may be NULL).  Does not wait for the device. */
int wh_last_score_shapes(wh_ehmm *e, int32_t *cells_per_lane, int32_t *waves, int32_t *p2win, int cap);
/* When enabled, every kernel launch is bracketed by HIP events (bench/roofline use). */
int wh_set_timing(wh_ehmm *e, int enabled);
/* Development knobs (WH_SCORE_KERNEL, WH_KEEP_LOG2, WH_MAX_WAVES, WH_FORCE_SPECG,
 * WH_NO_LOGSPACE, WH_STATS, WH_TRACE, WH_DBG; WH_SCORE_LMAIN=<n> caps the main length of scoring and alignment calls at n
 * residues, WH_NO_LONG_SCORE switches the long-query scoring / alignment passes off, WH_LONGQ_FORCE runs them with the
 * residues in HBM whatever the length).  The environment is read ONCE, in wh_ehmm_load; this call
 * changes a knob on a live handle (A/B harness tools/ab_score.py).  Production needs none of them. */
int wh_set_option(wh_ehmm *e, const char *name, const char *value);

/* ---- final transitive merge ---------------------------------------------------
 * Replaces mergeAlignmentsCollapsed -> ExtendedAlignment.merge_in per query (witch_msa/gcmm/merger.py:40-131,
 * helpers/alignment_tools.py:1183-1316) and the masked writer (alignment_tools.py:1140-1156, merger.py:100-103),
 * fed directly with wh_consensus' per-residue codes (code >= 0 backbone column; -1 - g insertion in front of
 * column g).  q_text: the queries' characters as given (case is normalised as the reference does: aligned
 * residues upper, insertions lower); q_row[q]: >= 0 the query gets a row (rows follow the backbone rows in query
 * order), -1 its insertions widen the gaps but it gets no row (its name exists already), -2 no alignment.
 * backbone: nb rows of B characters (already upper-cased).  Returns two malloc'ed row-major byte matrices
 * (release with wh_free_text): the full alignment rows x width and the masked one rows x B.  Needs no model
 * handle: device = the HIP device to run on. */
int wh_merge(int device, const uint8_t *q_text, const int64_t *q_off, int64_t nq, const int32_t *codes, const int32_t *q_row,
             const uint8_t *backbone, int32_t nb, int32_t B, uint8_t **out_full, uint8_t **out_masked, int64_t *out_rows,
             int64_t *out_width);
/* One process per GPU (queries sharded): the width of a gap is the MAX over all ranks' queries - the merge's one
 * exchange step.  Call once with widths_local != NULL and out_full == NULL (fills widths_local[B+1] from this
 * rank's queries, renders nothing; backbone may be NULL), all-reduce MAX over the ranks (RCCL), call again with
 * widths_global: this rank's rows (nb backbone rows first; pass nb = 0 on the ranks that do not write them) are
 * rendered in the global layout. */
int wh_merge_sharded(int device, const uint8_t *q_text, const int64_t *q_off, int64_t nq, const int32_t *codes, const int32_t *q_row,
                     const uint8_t *backbone, int32_t nb, int32_t B, int32_t *widths_local, const int32_t *widths_global,
                     uint8_t **out_full, uint8_t **out_masked, int64_t *out_rows, int64_t *out_width);

/* ---- hmmalign for a FILE of sequences: one alignment of all of them to one model ------------------------------------
 * What `hmmalign [--trim] HMM SEQFILE` computes (HMMER 3.1b2: p7_tracealign_Seqs; the reference's bundled MAGUS, SEPP and
 * UPP call it with whole fragment files), assembled on the device from wh_align_pp_dev's per-residue columns and posteriors
 * for the pairs (q, h), q = 0..nq-1 (CSR by the sequences' offsets), and the sequences' characters as given (text, as
 * wh_merge's q_text: match residues come out upper case, inserts lower case).  Layout: every node 1..M is a column; between
 * the columns of nodes k and k + 1 lies insert block k, as wide as the longest insert run any sequence has there (block 0:
 * the N flank, right-justified; block M: the C flank, left-justified; an internal run of n residues puts its first n / 2
 * flush left and the rest flush right); a deleted node is '-', an unused insert cell '.'.  Returned, each malloc'ed (release
 * with wh_free_text; on failure nothing is left allocated):
 *   W                 the alignment's width
 *   rows[nq x W]      the sequences' rows           pp_rows[nq x W]  their "#=GR PP" rows ('.' where the row has no residue)
 *   pp_cons[W]        "#=GC PP_cons": on a match column the character of the MEAN posterior over the sequences with a residue
 *                     there (float32 sum in sequence order - no floating-point atomics - divided by the count), '.' elsewhere
 *   rf[W]             "#=GC RF" of a model without a reference line of its own: 'x' on match columns, '.' on insert columns
 *   matmap[M]         0-based alignment column of node k + 1
 *   pathless          sequences that came back from the alignment without a match state: they render as gaps only
 * flags: WH_MSA_TRIM = hmmalign --trim: the residues of both flanks are dropped (blocks 0 and M stay empty).
 * nq == 0: WH_OK, W = M.  h out of range or a NULL handle: WH_EINVAL, wh_last_error names the entry point.
 * wh_msa_dev is the assembly alone, on device arrays (total_residues = d_offsets[nq]; it waits for the stream once, to read
 * W, and once at the end); wh_msa takes host pointers and runs wh_align_pp_dev first.  wh_last_kernel_ms(6): the assembly's
 * kernels; (2): the alignment launches of wh_msa. */
#define WH_MSA_TRIM   1
#define WH_MSA_NO_LDS 2   /* test hook: the rows are rendered in global memory whatever the width */
#define WH_MSA_CONS_HMMER 4   /* wh_msa_dev only: PP_cons in HMMER's own arithmetic - the float posteriors summed in a double
                               * in row order, divided by (float) n, the quotient rounded to float and encoded as (int)(p * 10.0 +
                               * 0.5).  wh_hits_msa_dev sets it (the arithmetic reproduces the binary's -A files); wh_msa's
                               * float32 sums stay as they are */
int wh_msa(wh_ehmm *e, const uint8_t *residues, const int64_t *offsets, const uint8_t *text, int64_t nq, int32_t h,
           int32_t flags, int64_t *out_W, uint8_t **out_rows, uint8_t **out_pp_rows, uint8_t **out_pp_cons, uint8_t **out_rf,
           int32_t **out_matmap, int64_t *out_pathless);
int wh_msa_dev(wh_ehmm *e, const int32_t *d_cols, const float *d_pp, const uint8_t *d_text, const int64_t *d_offsets,
               int64_t nq, int64_t total_residues, int32_t h, int32_t flags, int64_t *out_W, uint8_t **out_rows,
               uint8_t **out_pp_rows, uint8_t **out_pp_cons, uint8_t **out_rf, int32_t **out_matmap, int64_t *out_pathless,
               void *stream);

/* ---- hmmalign --mapali ALN HMM SEQS: the alignment model h was built from as rows of the output, in front of the new
 * sequences (HMMER's way to add sequences to an existing alignment: what UPP and SEPP call the extended alignment of a
 * subset).  map_rows: the n_map rows of that alignment, alen characters each, no terminator (a letter is a residue, any
 * other character of the alphabet a gap).  A residue of such a row goes by its alignment COLUMN, through the model's MAP
 * annotation (wh_ehmm_map): in the column of node k it is node k's, upper case; in a column between those of nodes k and
 * k + 1 it is an insert of block k, lower case (before node 1's column: block 0, behind node M's: block M) - also where the
 * row has no residue in node k's column, or none in any node's column before it.  Inside a block the alignment's own columns
 * are not kept: the residues a row has there form one run, laid out like a new sequence's (above); block widths are the
 * maximum over rows and new sequences together; WH_MSA_TRIM drops the rows' residues of blocks 0 and M too.
 * Outputs as wh_msa's, with these differences: rows holds n_map + nq rows, the alignment's first; pp_rows holds nq rows (a
 * row of the alignment has no posteriors, hmmalign writes no "#=GR PP" line for it); pp_cons is the mean over the new
 * sequences alone; pathless counts new sequences only.  n_map == 0: wh_msa's result.  nq == 0 with n_map > 0: the rows alone.
 * WH_EINVAL, wh_last_error naming the entry point: a model without "MAP yes" or without a CKSUM line, or whose MAP columns do
 * not increase; alen short of the last MAP column; bad pointers; and, wh_msa_mapali only, a character outside the alphabet or
 * an alignment whose checksum (wh_alignment_checksum) is not the model's CKSUM - hmmalign's "checksum mismatch".
 * wh_msa_mapali_dev takes the rows and the new sequences' alignment on the device and does NOT verify the checksum (its caller
 * has the rows on the host, or has none); it waits for the stream three times (the rows' residue counts, the uploads, W) and
 * at the end.  wh_last_kernel_ms(7): the count and map kernels with the host's wait between them; (6): the assembly. */
int wh_msa_mapali(wh_ehmm *e, const uint8_t *residues, const int64_t *offsets, const uint8_t *text, int64_t nq, int32_t h,
                  int32_t flags, const uint8_t *map_rows, int64_t n_map, int64_t alen, int64_t *out_W, uint8_t **out_rows,
                  uint8_t **out_pp_rows, uint8_t **out_pp_cons, uint8_t **out_rf, int32_t **out_matmap, int64_t *out_pathless);
int wh_msa_mapali_dev(wh_ehmm *e, const int32_t *d_cols, const float *d_pp, const uint8_t *d_text, const int64_t *d_offsets,
                      int64_t nq, int64_t total_residues, int32_t h, int32_t flags, const uint8_t *d_map_rows, int64_t n_map,
                      int64_t alen, int64_t *out_W, uint8_t **out_rows, uint8_t **out_pp_rows, uint8_t **out_pp_cons,
                      uint8_t **out_rf, int32_t **out_matmap, int64_t *out_pathless, void *stream);
/* hmmbuild's CKSUM of an alignment (nseq rows of alen characters, flat): Jenkins' one-at-a-time hash over the digital
 * residues; case and the gap character ('-' '.' '_') do not enter it.  Host code, no GPU needed.  molecule as wh_hmmbuild. */
int wh_alignment_checksum(const char *molecule, const char *rows, int32_t nseq, int64_t alen, uint32_t *out_cksum);
/* The CKSUM line of model h: *present = 0 where the file has none. */
int wh_ehmm_cksum(const wh_ehmm *e, int h, uint32_t *cksum, int32_t *present);

/* ---- hmmsearch -A FILE: the alignment of all hits that satisfy the inclusion thresholds ---------------------------------
 * wh_domain_paths[_dev] replaces nothing of its own: it is wh_domains[_dev] - the same steps through the same code, the
 * records bit for bit - that also hands back what it computes on the way, the alignment of every envelope: env_off
 * [ndom + 1], the CSR of the envelopes in record order, and per envelope residue its 0-based node (-1: none) and the float32
 * posterior of its state (wh_align_pp's values).
 *  - _dev: *d_env_off, *d_cols, *d_pp point into the handle's workspace on the device and stay valid until the next
 *    wh_domains*, wh_domain_paths* or wh_hits_msa call on the handle; *total_env = env_off[ndom].  Waits as wh_domains_dev.
 *  - host: env_off is the caller's [ndom + 1]; *out_cols and *out_pp are malloc'ed (release with wh_free_text; NULL where
 *    there is no domain).
 * wh_hits_msa[_dev] replaces HMMER 3.1b2's p7_tophits_Alignment behind `hmmsearch -A`: every domain of model h that passes
 * the inclusion thresholds becomes one row of hmmalign's alignment (wh_msa's layout and outputs).  A domain is included where
 * its pair is WH_FLAG_REPORTED, it has a path (ali_i != 0), the sequence's E-value exp(lnP_seq) Z <= incE with lnP_seq =
 * min(0, -lambda (seq_score - tau)) in double from the float32 fields, and its own conditional E-value exp(lnP) domZ <=
 * incdomE; both are decided as lnP <= ln(threshold / Z), the logarithms taken once on the host (a model without a STATS
 * line has no E-values: every reported sequence and every domain with a path is included, as in the level-0 tables).  Pairs of
 * other models than h are ignored.  Rows: the queries in order[0..nq-1] (a permutation of 0..nq-1; NULL: query order), the
 * domains of a query in domain order.  A row is the residues ali_i..ali_j of the sequence (text: the characters as given)
 * with the domain's own path on that range - no re-alignment - and with posteriors as HMMER keeps them for such a row: the
 * displayed PP character decoded again ('*' where p + 0.05 >= 1.0 -> 1.0, else d = (int)(p * 10.0 + 0.5) -> (float)d / 10), so
 * the "#=GR PP" rows are the characters of the real posteriors and "#=GC PP_cons" is the character of the mean of the decoded
 * tenths, in HMMER's own arithmetic (WH_MSA_CONS_HMMER).
 * Outputs: *out_nrows and rows_rec[*out_nrows] (malloc'ed, wh_free_text: per row the query, the domain's index within its
 * pair, ali_i, ali_j - the caller forms the name "name/ali_i-ali_j" from them), then wh_msa's W, rows, pp_rows, pp_cons, rf,
 * matmap.  No included domain: WH_OK, 0 rows, W = M.  msa_flags: 0 or WH_MSA_NO_LDS.
 * WH_EINVAL, wh_last_error naming the entry point: NULL handle, h out of range, opts NULL or Z <= 0 or domZ <= 0 or a
 * negative or NaN threshold, records that do not fit dom_off / their envelopes / their queries, an order[] that names a query
 * outside 0..nq-1 or yields more rows than there are domains (a query named twice: the caller's error, never a write out of
 * bounds).
 * wh_hits_msa_dev is the stage alone, on device arrays (it reads dom_off's last entry back, then the row and residue totals -
 * two waits before wh_msa_dev's own).  wh_hits_msa takes host pointers and runs wh_domain_paths_dev then wh_hits_msa_dev;
 * out_dom (optional, [dom_off[nq x H]]) receives the wh_domain records, so that a caller who wants the domain tables and the
 * alignment pays for one alignment of the envelopes.  wh_last_kernel_ms(8): the mark, scan, place and slice kernels with the
 * host's wait between them; (6): the assembly; (5): the domain stage of wh_hits_msa. */
typedef struct wh_hits_opts { double Z, domZ, incE, incdomE; } wh_hits_opts;
typedef struct wh_hit_row { int32_t query, index, ali_i, ali_j; } wh_hit_row;
int wh_domain_paths(wh_ehmm *e, const uint8_t *residues, const int64_t *offsets, int64_t nq, const uint8_t *flags,
                    const wh_pair_detail *detail, const int64_t *dom_off, wh_domain *out, int64_t *env_off,
                    int32_t **out_cols, float **out_pp);
int wh_domain_paths_dev(wh_ehmm *e, const uint8_t *d_residues, const int64_t *d_offsets, int64_t nq, int64_t total_residues,
                        int32_t max_len, const uint8_t *d_flags, const wh_pair_detail *d_detail, const int64_t *d_dom_off,
                        wh_domain *d_out, const int64_t **d_env_off, const int32_t **d_cols, const float **d_pp,
                        int64_t *total_env, void *stream);
int wh_hits_msa(wh_ehmm *e, const uint8_t *residues, const int64_t *offsets, const uint8_t *text, int64_t nq,
                const uint8_t *flags, const wh_pair_detail *detail, const int64_t *dom_off, int32_t h, const int32_t *order,
                const wh_hits_opts *opts, int32_t msa_flags, wh_domain *out_dom, int64_t *out_nrows, wh_hit_row **out_rows_rec,
                int64_t *out_W, uint8_t **out_rows, uint8_t **out_pp_rows, uint8_t **out_pp_cons, uint8_t **out_rf,
                int32_t **out_matmap);
int wh_hits_msa_dev(wh_ehmm *e, const uint8_t *d_text, const int64_t *d_offsets, int64_t nq, const uint8_t *d_flags,
                    const wh_pair_detail *d_detail, const int64_t *d_dom_off, const wh_domain *d_dom, const int64_t *d_env_off,
                    const int32_t *d_cols, const float *d_pp, int32_t h, const int32_t *d_order, const wh_hits_opts *opts,
                    int32_t msa_flags, int64_t *out_nrows, wh_hit_row **out_rows_rec, int64_t *out_W, uint8_t **out_rows,
                    uint8_t **out_pp_rows, uint8_t **out_pp_cons, uint8_t **out_rf, int32_t **out_matmap, void *stream);

/* ---- hmmsearch's alignment display: the four lines under "== domain N" -------------------------------------------------
 * wh_domain_display[_dev] replaces what HMMER 3.1b2's p7_alidisplay_Create writes for every reported domain: the model's
 * consensus line, the match line, the target line and the posterior (PP) line, one character per alignment column from the
 * domain's first match state (ali_i / hmm_i) to its last (ali_j / hmm_j).  The caller wraps them into blocks and adds names
 * and coordinates (witch_amd/shim/formats.py: format_alidisplay).  Per column:
 *   match state   model: the node's consensus letter as the model file prints it; target: the alphabet's symbol of the
 *                 residue's digital code, upper case; match line: the consensus letter where the residue's code equals the
 *                 letter's code, else '+' where the float32 match odds of that residue at that node exceed 1.0, else ' '
 *   insert state  model '.', match line ' ', target: the symbol in lower case
 *   delete state  (a node between two consecutive match states of the path) model: its consensus letter, match line ' ',
 *                 target '-', PP '.'
 *   PP            match and insert: HMMER's p7_alidisplay_EncodePostProb of the float32 posterior, in double:
 *                 '*' where p + 0.05 >= 1.0, else '0' + (int)((p + 0.05) * 10.0)
 * A domain is SELECTED where its pair is WH_FLAG_REPORTED and of model h, it has a path (ali_i != 0) and is reportable:
 * lnP <= ln(domE / domZ), the logarithm taken once on the host (domE = 0 selects nothing; lnP NaN - a model without a STATS
 * line - selects every domain with a path).  The selected domains keep record order.
 * The model needs "CONS yes" in its header and neither "RF yes" nor "CS yes" (HMMER prints extra lines for those): any
 * other model is refused with WH_EINVAL, wh_last_error naming the entry point and the header key.  The model's display table
 * (float32 match odds per node and residue code, degenerate codes included, from the values the scoring tables are built
 * from; the consensus letters and their codes) is built and uploaded at the first display call of that model, not at load.
 * Inputs: residues / offsets / nq / flags of the scoring call, dom_off, and the records, env_off, cols, pp of
 * wh_domain_paths_dev.  Outputs of _dev, the CALLER's device arrays: d_disp_off[ndom + 1] (the first nsel + 1 entries are
 * written), d_recs[ndom] (nsel written: the query and the domain's index within its pair), and four byte arrays of cap
 * bytes each, of which the first disp_off[nsel] are written, each exactly once; nothing beyond is touched.  cap >= the sum
 * over all domains of (M + envelope length) always suffices.  *out_nsel, *out_total = disp_off[nsel]; WH_ERANGE (nothing
 * rendered, *out_total set) where total > cap.  The records are checked against dom_off, their envelopes, their queries and
 * their own paths (nodes rising from hmm_i to hmm_j): WH_EINVAL otherwise.  Three kernels - count (one wavefront per domain),
 * a two-level scan, render (one wavefront per domain) - and one wait of the host between count and render, after a first
 * one for dom_off's last entry.  wh_last_kernel_ms(9): these kernels with that wait.
 * The PP line encodes the posteriors it is given.  Under WH_LENMODEL_ENVELOPE (the default) wh_domain_paths_dev's are
 * hmmalign's, under the length model of the envelope, where hmmsearch decodes an envelope under the length model of its whole
 * sequence (the level-0 server then passes those from a second alignment launch: DESIGN.md section 4.15).  Under
 * WH_LENMODEL_SEQUENCE the stage's path and posteriors are hmmsearch's already.
 * wh_domain_display takes host pointers and runs wh_domain_paths_dev first (wh_last_kernel_ms(5): that domain stage);
 * out_dom (optional, [dom_off[nq x H]]) receives the wh_domain records; *out_disp_off, *out_recs and the four lines are
 * malloc'ed (release with wh_free_text; NULL where nothing is selected).
 * wh_ehmm_consensus: the consensus letters of model h as its file prints them (the CONS column of the match lines), M
 * characters without a terminator; *present = 0 and nothing written where the header does not say "CONS yes". */
typedef struct wh_display_rec { int32_t query, index; } wh_display_rec;
int wh_ehmm_consensus(const wh_ehmm *e, int h, char *out /* [M] */, int32_t *present);
/* The same for one model file, through the same parser, without a handle (wh_ehmm_load needs a device, this does not): the
 * first min(cap, M) letters, *out_M = M (optional), *present = 1 (CONS yes) | 2 (RF yes) | 4 (CS yes). */
int wh_hmm_consensus(const char *hmm_path, char *out, int32_t cap, int32_t *out_M, int32_t *present);
int wh_domain_display(wh_ehmm *e, const uint8_t *residues, const int64_t *offsets, int64_t nq, const uint8_t *flags,
                      const wh_pair_detail *detail, const int64_t *dom_off, int32_t h, double domE, double domZ,
                      wh_domain *out_dom, int64_t *out_nsel, int64_t **out_disp_off, wh_display_rec **out_recs,
                      uint8_t **out_model, uint8_t **out_match, uint8_t **out_target, uint8_t **out_pp);
int wh_domain_display_dev(wh_ehmm *e, const uint8_t *d_residues, const int64_t *d_offsets, int64_t nq, const uint8_t *d_flags,
                          const int64_t *d_dom_off, const wh_domain *d_dom, const int64_t *d_env_off, const int32_t *d_cols,
                          const float *d_pp, int32_t h, double domE, double domZ, int64_t cap, int64_t *d_disp_off,
                          wh_display_rec *d_recs, uint8_t *d_model, uint8_t *d_match, uint8_t *d_target, uint8_t *d_ppline,
                          int64_t *out_nsel, int64_t *out_total, void *stream);

/* ---- hmmsearch --tblout: the per-sequence table -------------------------------------------------------------------------
 * Three of its columns are counts of HMMER's domain definition that the scoring kernels do not export: exp, the expected
 * number of domains (the B state's posterior occupancy summed over the sequence, btot[L]); reg, the regions of the
 * rt1 = 0.25 / rt2 = 0.10 scan; clu, how many of them met the multidomain test (rt3 = 0.20) and went to stochastic clustering.
 * wh_seq_expect[_dev] recomputes the two full-width multihit sweeps they come from for the pairs of pair_list alone
 * (pair_list[t] = q * H + h, any order, a pair may repeat): out[t] = { exp, reg, clu }.  One wavefront per pair, float32 in
 * HMMER's arithmetic for models of up to 3 072 nodes (the DP row in registers, the special states of every row in a
 * per-wave HBM workspace sized from max_len: no limit on the query length); longer models: float64, the row in HBM.  A pair
 * whose Forward score is not finite, or an empty query: { 0, 0, 0 }.  The _dev variant reads the pair list back (it waits
 * for the stream once) to order the work by model.  wh_seq_expect_host: the same sweeps in float64 as plain scalar code
 * over the n model files - no handle, no HIP call; thresholds and profile construction are the kernels'. */
typedef struct wh_seq_expect_rec { float exp; int32_t reg, clu; } wh_seq_expect_rec;
int wh_seq_expect(wh_ehmm *e, const uint8_t *residues, const int64_t *offsets, int64_t nq, const int64_t *pair_list,
                  int64_t n_pairs, wh_seq_expect_rec *out);
int wh_seq_expect_dev(wh_ehmm *e, const uint8_t *d_residues, const int64_t *d_offsets, int64_t nq, int64_t total_residues,
                      int32_t max_len, const int64_t *d_pair_list, int64_t n_pairs, wh_seq_expect_rec *d_out, void *stream);
int wh_seq_expect_host(const char *const *hmm_paths, int n, const uint8_t *residues, const int64_t *offsets, int64_t nq,
                       const int64_t *pair_list, int64_t n_pairs, wh_seq_expect_rec *out);
/* One row per pair with WH_FLAG_REPORTED, in pair order, from the flags and detail records of a scoring call over the same
 * queries.  Z <= 0: nq; domZ <= 0: the number of reported pairs (as HMMER sets them).  Returns the number of rows (>= 0) or a
 * negative WH_E* code; WH_ERANGE: more rows than <cap> (nothing is written).
 *   seq_bits, seq_bias_bits   the sequence's score and bias: detail.seq_score, max(0, pre_score - seq_score)
 *   seq_lnP                   min(0, -lambda (seq_score - tau)) in double from the float32 fields; NaN without a STATS line
 *   exp, clu                  from the sweep (wh_seq_expect)
 *   reg                       detail.nregions, the count the score was built from (the sweep's own count is compared:
 *                             wh_last_seq_table_status)
 *   env, dom                  the envelopes the detail record lists (min(nenv, WH_MAX_ENVELOPES))
 *   ov                        listed envelopes d >= 1 with env_i[d] <= env_j[d - 1]
 *   best ...                  the listed envelope with the largest bits (a tie: the first), its bits, bias and lnP by the
 *                             formula above wh_domain
 *   rep, inc                  listed domains with exp(lnP) domZ <= domE on a sequence with E-value <= E; ... <= incdomE on
 *                             a sequence with E-value <= incE (a model without STATS lines: every listed domain)
 *   capped                    1 where nenv == WH_MAX_ENVELOPES or nregions > WH_MAX_ENVELOPES: env, dom, ov, rep, inc and
 *                             the best domain are then lower bounds (see wh_domain_counts)
 * Two small kernels around wh_seq_expect_dev: the first compacts the reported pairs into the pair list, the second fills
 * one record per lane.  The _dev variant waits for the stream twice (the row count, the pair list). */
typedef struct wh_seq_table_opts { double Z, domZ, E, domE, incE, incdomE; } wh_seq_table_opts;
typedef struct wh_seq_row {
  int64_t pair;
  double  seq_lnP;
  float   seq_bits, seq_bias_bits;
  float   exp;
  int32_t reg, clu, ov, env, dom, rep, inc;
  int32_t best;
  float   best_bits, best_bias_bits, best_lnP;
  int32_t capped;
  int32_t reserved;        /* 0 (the record is 80 bytes) */
} wh_seq_row;
int wh_seq_table(wh_ehmm *e, const uint8_t *residues, const int64_t *offsets, int64_t nq, const uint8_t *flags,
                 const wh_pair_detail *detail, const wh_seq_table_opts *opts, wh_seq_row *out, int64_t cap);
int wh_seq_table_dev(wh_ehmm *e, const uint8_t *d_residues, const int64_t *d_offsets, int64_t nq, int64_t total_residues,
                     int32_t max_len, const uint8_t *d_flags, const wh_pair_detail *d_detail, const wh_seq_table_opts *opts,
                     wh_seq_row *d_out, int64_t cap, void *stream);
/* The assembly alone on host arrays, without a handle or a device (the same inline code the kernel runs): rows from the
 * records and the sweep's results expect[t] of the reported pairs in pair order (t-th reported pair); tau / lambda [H] as
 * wh_ehmm_evparams gives them.  lengths[nq]: the queries' lengths.  Returns the row count or WH_ERANGE. */
int wh_seq_table_host(int H, const float *tau, const float *lambda, const int64_t *lengths, int64_t nq, const uint8_t *flags,
                      const wh_pair_detail *detail, const wh_seq_expect_rec *expect, const wh_seq_table_opts *opts,
                      wh_seq_row *out, int64_t cap);
/* The last wh_seq_table[_dev] call: out[0] = rows, [1] = rows with capped set, [2] = rows whose sweep counted other regions
 * than detail.nregions, [3] = pairs the sweep served on the any-size float64 path. */
int wh_last_seq_table_status(wh_ehmm *e, int64_t out[4]);

/* ---- eHMM construction (host code, no GPU needed) -------------------------------
 * Replaces the reference's per-subset call
 *     hmmbuild --cpu 1 --<molecule> --ere 0.59 --symfrac 0.0 --informat afa -o /dev/null MODEL SUBSET.fasta
 * (witch_msa/gcmm/algorithm.py:463-470).  rows: nseq aligned sequences of alen characters each (aligned
 * FASTA text, '-' '.' '_' gaps; no terminator needed), molecule "dna" | "rna" | "amino".  Writes the model as
 * HMMER3/f text (same probability fields, MAP / CONS annotation, COMPO, NSEQ / EFFN / CKSUM as hmmbuild
 * 3.1b2, MAXL included for nucleotide models; no STATS lines - see wh_hmmbuild2) into a malloc'ed buffer the caller releases with wh_free_text.  out_M /
 * out_neff (optional): model length and effective sequence number. */
int  wh_hmmbuild(const char *molecule, int32_t nseq, int64_t alen, const char *const *rows, const char *name,
                 double ere, double symfrac, double fragthresh, char **out_text, int64_t *out_len,
                 int32_t *out_M, double *out_neff);
/* Same, with options.  flags: WH_BUILD_STATS adds hmmbuild's three "STATS LOCAL MSV / VITERBI / FORWARD" lines
 * (E-value calibration on 3 x 200 random sequences, generator seeded with 42 as hmmbuild does: the MSV and Viterbi
 * and Forward locations come out in hmmbuild's printed digits on all 47 golden model files; the reference's bundled
 * hmmsearch then prints the same report, E-values included, as for hmmbuild's own file).  WITCH never reads them
 * (hmmsearch -E 99999999, only bit scores are parsed); stock HMMER refuses a file without them.  Costs about 0.5 s
 * per 1 000-node model on one core, against 15 ms for the build itself: wh_hmmbuild_batch calibrates a whole eHMM
 * on the device instead. */
#define WH_BUILD_STATS 1
int  wh_hmmbuild2(const char *molecule, int32_t nseq, int64_t alen, const char *const *rows, const char *name,
                  double ere, double symfrac, double fragthresh, int32_t flags, char **out_text, int64_t *out_len,
                  int32_t *out_M, double *out_neff);
/* All models of an eHMM in one call: model i from nseq[i] rows of alen[i] characters (rows[i]), named names[i] (names or
 * names[i] NULL: "sub"), built on the host exactly as wh_hmmbuild2 builds it; out_text[i] is byte for byte what
 * wh_hmmbuild2 returns for it (release each with wh_free_text).  With WH_BUILD_STATS all n models are calibrated in one
 * batch: device >= 0 on that HIP device (wh_calibrate.hip: one lane per (model, random sequence), the host's sweeps
 * compiled for the device, the integer filters and the float64 Forward recurrence bit for bit the host's), device < 0
 * on the host, without any HIP call.  The device's row workspace is 200 x 62 x (M + 1) + 160 000 bytes per model (+ its tables, 124 (M + 1) bytes for DNA);
 * the models run in groups that fit a budget of 1 GiB (environment, read per call: WH_CALIB_WS_MB=<n> MiB) and half of
 * the device's free memory; a model that does not fit alone is refused with WH_ENOMEM before anything is launched
 * (wh_last_error: the figures).  out_M, out_neff (optional): [n]; out_stats (optional): [n][4] lambda, MSV mu, Viterbi mu,
 * Forward tau as doubles (the text holds them as float32; zeros without WH_BUILD_STATS).  On failure every out_text[i] is
 * NULL, nothing is left allocated and wh_last_error names the model.  n == 0: WH_OK. */
#define WH_BUILD_CALIB_NO_LDS 4   /* test hook: calibration tables from global memory whatever their size */
int  wh_hmmbuild_batch(int device, const char *molecule, int32_t n,
                       const int32_t *nseq, const int64_t *alen, const char *const *const *rows,
                       const char *const *names, double ere, double symfrac, double fragthresh, int32_t flags,
                       char **out_text, int64_t *out_len, int32_t *out_M, double *out_neff,
                       double *out_stats /* optional, [n][4]: lambda, MSV mu, Viterbi mu, Forward tau */);
void wh_free_text(char *text);

#ifdef __cplusplus
}
#endif
#endif /* WITCH_HIP_H */
