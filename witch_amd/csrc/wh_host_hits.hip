// Host side of hmmsearch -A (include/witch_hip.h: wh_hits_msa_dev, wh_hits_msa): the kernels of wh_hits.hip between the domain
// stage (wh_domain_paths_dev) and the alignment assembly (wh_msa_dev), which serves unchanged.
#include "wh_host.h"

namespace {

// ln(threshold / n) for the device's comparisons; a threshold of 0 includes nothing (-inf)
double ln_threshold(double thr, double n) { return thr > 0.0 ? std::log(thr / n) : -INFINITY; }

int check_hits_args(const char *who, const wh_ehmm *e, int32_t h, const wh_hits_opts *opts, int32_t msa_flags) {
  // (what needs no handle first: a caller's mistake in the thresholds is named whatever else is wrong)
  if (!opts) { set_error("%s: bad argument (no thresholds)", who); return WH_EINVAL; }
  if (!(opts->Z > 0.0) || !(opts->domZ > 0.0)) { set_error("%s: Z = %g and domZ = %g must both be > 0", who, opts->Z, opts->domZ); return WH_EINVAL; }
  if (!(opts->incE >= 0.0) || !(opts->incdomE >= 0.0)) { set_error("%s: incE = %g and incdomE = %g must both be >= 0", who, opts->incE, opts->incdomE); return WH_EINVAL; }
  if (msa_flags & ~WH_MSA_NO_LDS) { set_error("%s: bad argument (flags)", who); return WH_EINVAL; }
  if (h < 0) { set_error("%s: model position %d out of range", who, h); return WH_EINVAL; }
  if (!e) { set_error("%s: null handle", who); return WH_EINVAL; }
  if (h >= (int)e->hmms.size()) { set_error("%s: model position %d out of range (0..%d)", who, h, (int)e->hmms.size() - 1); return WH_EINVAL; }
  return WH_OK;
}

}  // namespace

extern "C" {

int wh_hits_msa_dev(wh_ehmm *e, const uint8_t *d_text, const int64_t *d_offsets, int64_t nq, const uint8_t *d_flags,
                    const wh_pair_detail *d_detail, const int64_t *d_dom_off, const wh_domain *d_dom, const int64_t *d_env_off,
                    const int32_t *d_cols, const float *d_pp, int32_t h, const int32_t *d_order, const wh_hits_opts *opts,
                    int32_t msa_flags, int64_t *out_nrows, wh_hit_row **out_rows_rec, int64_t *out_W, uint8_t **out_rows,
                    uint8_t **out_pp_rows, uint8_t **out_pp_cons, uint8_t **out_rf, int32_t **out_matmap, void *stream) {
  const char *who = "wh_hits_msa_dev";
  if (int rc = check_hits_args(who, e, h, opts, msa_flags)) return rc;
  if (nq < 0 || !out_nrows || !out_rows_rec || !out_W || !out_rows || !out_pp_rows || !out_pp_cons || !out_rf || !out_matmap ||
      (nq > 0 && (!d_offsets || !d_flags || !d_detail || !d_dom_off))) {
    set_error("%s: bad argument", who);
    return WH_EINVAL;
  }
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipSetDevice(e->device));
  const int H = (int)e->hmms.size();
  const int64_t npairs = nq * H;
  if (npairs > 0x7FFFFFFF) { set_error("%s: too many pairs", who); return WH_ERANGE; }
  e->timers[8].launches = 0; e->timers[8].ms = 0; e->timers[8].pending = false;
  *out_nrows = 0; *out_rows_rec = nullptr;
  int64_t pathless = 0;
  int64_t ndom = 0;
  if (npairs > 0) {
    HIPCHK(hipMemcpyAsync(&ndom, d_dom_off + npairs, sizeof ndom, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (ndom < 0 || ndom > npairs * WH_MAX_ENVELOPES) { set_error("%s: dom_off ends at %lld for %lld pairs", who, (long long)ndom, (long long)npairs); return WH_EINVAL; }
    if (ndom > 0 && (!d_dom || !d_env_off || !d_cols || !d_pp || !d_text)) { set_error("%s: bad argument", who); return WH_EINVAL; }
  }
  if (ndom == 0)                 // nothing to include: the model's columns alone
    return wh_msa_dev(e, nullptr, nullptr, nullptr, nullptr, 0, 0, h, msa_flags | WH_MSA_CONS_HMMER, out_W, out_rows, out_pp_rows, out_pp_cons, out_rf, out_matmap, &pathless, stream);

  const HostHMM &m = e->hmms[(size_t)h];
  HitsArgs a;
  memset(&a, 0, sizeof a);
  a.flags = d_flags; a.detail = d_detail; a.dom_off = d_dom_off; a.dom = d_dom; a.npairs = npairs; a.ndom = ndom; a.nq = nq; a.H = H; a.h = h;
  a.env_off = d_env_off; a.cols = d_cols; a.pp = d_pp; a.text = d_text; a.offsets = d_offsets; a.order = d_order;
  a.tau = m.has_fstats ? m.ftau : NAN; a.lambda = m.has_fstats ? m.flambda : NAN;
  a.ln_inc_seq = ln_threshold(opts->incE, opts->Z); a.ln_inc_dom = ln_threshold(opts->incdomE, opts->domZ);
  a.nblk = hits_scan_blocks(nq);
  // d_hits_work: totals [2] | bad [1 int, padded] | blk_row [nblk] | blk_res [nblk] | pos_res [nq] | row_dom [ndom] |
  // row_off [ndom + 1] (8-byte words), then row_rec [ndom] (16 bytes), then pos_row [nq] | len [ndom] (ints)
  const size_t n8 = 3 + 2 * (size_t)a.nblk + (size_t)nq + 2 * (size_t)ndom + 1;
  const size_t rec_at = (n8 * 8 + 15) & ~(size_t)15, int_at = rec_at + sizeof(wh_hit_row) * (size_t)ndom;
  if (e->d_hits_work.ensure(int_at + sizeof(int32_t) * ((size_t)nq + (size_t)ndom) + 16)) return WH_ENOMEM;
  long long *w8 = (long long *)e->d_hits_work.p;
  a.totals = w8; a.bad = (int *)(w8 + 2); a.blk_row = w8 + 3; a.blk_res = a.blk_row + a.nblk; a.pos_res = a.blk_res + a.nblk;
  a.row_dom = (int64_t *)(a.pos_res + nq); a.row_off = a.row_dom + ndom;
  a.row_rec = (wh_hit_row *)((char *)e->d_hits_work.p + rec_at);
  a.pos_row = (int32_t *)((char *)e->d_hits_work.p + int_at); a.len = a.pos_row + nq;
  if (timer_begin(e, 8, s)) return WH_EHIP;
  HIPCHK(hipMemsetAsync(w8, 0, 3 * sizeof(long long), s));
  hipError_t err = launch_hits_mark(a, s);
  if (err == hipSuccess) err = launch_hits_scan(a, s);
  if (err != hipSuccess) { set_error("%s: mark / scan kernels failed to launch: %s", who, hipGetErrorString(err)); return WH_EHIP; }
  // the row count and the residue total come back once: they size the batch (as wh_msa_dev reads W)
  long long tot[3] = {0, 0, 0};
  HIPCHK(hipMemcpyAsync(tot, w8, sizeof tot, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if ((int)tot[2] != 0) { set_error("%s: a domain record does not fit dom_off, its envelope or its query, or order[] names a query outside 0..%lld", who, (long long)nq - 1); return WH_EINVAL; }
  // (each domain gives at most one row: more means order[] names a query twice)
  a.nrows = tot[0]; a.nres = tot[1];
  if (a.nrows < 0 || a.nrows > ndom || a.nres < a.nrows) { set_error("%s: %lld rows from %lld domains: order[] is not a permutation of the queries", who, tot[0], (long long)ndom); return WH_EINVAL; }
  if (a.nrows == 0) {
    if (timer_end(e, 8, s, 3)) return WH_EHIP;
    return wh_msa_dev(e, nullptr, nullptr, nullptr, nullptr, 0, 0, h, msa_flags | WH_MSA_CONS_HMMER, out_W, out_rows, out_pp_rows, out_pp_cons, out_rf, out_matmap, &pathless, stream);
  }
  if (e->d_hits_text.ensure((size_t)a.nres + 16) || e->d_hits_cols.ensure(sizeof(int32_t) * (size_t)a.nres + 16) ||
      e->d_hits_pp.ensure(sizeof(float) * (size_t)a.nres + 16))
    return WH_ENOMEM;
  a.out_text = (uint8_t *)e->d_hits_text.p; a.out_cols = (int32_t *)e->d_hits_cols.p; a.out_pp = (float *)e->d_hits_pp.p;
  // (a row the place kernel does not reach - order[] with a repeated and a missing query of equal counts - stays a row of no residues)
  HIPCHK(hipMemsetAsync(a.row_off, 0, sizeof(int64_t) * ((size_t)a.nrows + 1), s));
  HIPCHK(hipMemsetAsync(a.row_dom, 0, sizeof(int64_t) * (size_t)a.nrows, s));
  HIPCHK(hipMemsetAsync(a.row_rec, 0xFF, sizeof(wh_hit_row) * (size_t)a.nrows, s));
  err = launch_hits_place(a, s);
  if (err == hipSuccess) err = launch_hits_slice(a, s);
  if (err != hipSuccess) { set_error("%s: place / slice kernels failed to launch: %s", who, hipGetErrorString(err)); return WH_EHIP; }
  if (timer_end(e, 8, s, 5)) return WH_EHIP;
  wh_hit_row *recs = (wh_hit_row *)malloc(sizeof(wh_hit_row) * (size_t)a.nrows);
  if (!recs) { set_error("%s: out of host memory (%lld rows)", who, (long long)a.nrows); return WH_ENOMEM; }
  hipError_t cerr = hipMemcpyAsync(recs, a.row_rec, sizeof(wh_hit_row) * (size_t)a.nrows, hipMemcpyDeviceToHost, s);
  if (cerr != hipSuccess) { free(recs); set_error("%s: hipMemcpyAsync failed: %s", who, hipGetErrorString(cerr)); return WH_EHIP; }
  // the assembly waits for the stream before it returns: the records have arrived by then
  const int rc = wh_msa_dev(e, a.out_cols, a.out_pp, a.out_text, a.row_off, a.nrows, a.nres, h, msa_flags | WH_MSA_CONS_HMMER, out_W, out_rows, out_pp_rows, out_pp_cons,
                            out_rf, out_matmap, &pathless, stream);
  if (rc) { (void)hipStreamSynchronize(s); free(recs); return rc; }
  for (int64_t r = 0; r < a.nrows; r++)
    if (recs[r].query < 0) { free(recs); wh_free_text((char *)*out_rows); wh_free_text((char *)*out_pp_rows); wh_free_text((char *)*out_pp_cons); wh_free_text((char *)*out_rf); wh_free_text((char *)*out_matmap);
      *out_rows = *out_pp_rows = *out_pp_cons = *out_rf = nullptr; *out_matmap = nullptr;
      set_error("%s: order[] is not a permutation of the queries", who); return WH_EINVAL; }
  *out_nrows = a.nrows; *out_rows_rec = recs;
  return WH_OK;
}

int wh_hits_msa(wh_ehmm *e, const uint8_t *residues, const int64_t *offsets, const uint8_t *text, int64_t nq, const uint8_t *flags,
                const wh_pair_detail *detail, const int64_t *dom_off, int32_t h, const int32_t *order, const wh_hits_opts *opts,
                int32_t msa_flags, wh_domain *out_dom, int64_t *out_nrows, wh_hit_row **out_rows_rec, int64_t *out_W, uint8_t **out_rows,
                uint8_t **out_pp_rows, uint8_t **out_pp_cons, uint8_t **out_rf, int32_t **out_matmap) {
  const char *who = "wh_hits_msa";
  if (int rc = check_hits_args(who, e, h, opts, msa_flags)) return rc;
  if (nq < 0 || !out_nrows || !out_rows_rec || !out_W || !out_rows || !out_pp_rows || !out_pp_cons || !out_rf || !out_matmap ||
      (nq > 0 && (!residues || !offsets || !text || !flags || !detail || !dom_off))) {
    set_error("%s: bad argument", who);
    return WH_EINVAL;
  }
  if (nq == 0)
    return wh_hits_msa_dev(e, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, h, nullptr, opts, msa_flags, out_nrows,
                           out_rows_rec, out_W, out_rows, out_pp_rows, out_pp_cons, out_rf, out_matmap, nullptr);
  HIPCHK(hipSetDevice(e->device));
  const size_t np = (size_t)nq * e->hmms.size();
  const int64_t total = offsets[nq], ndom = dom_off[np];
  if (total < 0 || offsets[0] != 0 || ndom < 0) { set_error("%s: bad offsets", who); return WH_EINVAL; }
  if (check_residues(e->Kp, residues, total)) return WH_EINVAL;
  Staging st(e);
  const uint8_t *d_res = st.in(residues, (size_t)total, 16);
  const int64_t *d_off = st.in(offsets, sizeof(int64_t) * (size_t)(nq + 1));
  const uint8_t *d_text = st.in(text, (size_t)total, 16);
  const uint8_t *d_flags = st.in(flags, np);
  const wh_pair_detail *d_det = st.in(detail, sizeof(wh_pair_detail) * np);
  const int64_t *d_doff = st.in(dom_off, sizeof(int64_t) * (np + 1));
  const int32_t *d_order = st.in(order, sizeof(int32_t) * (size_t)nq);
  if (st.rc) return st.rc;
  if (e->d_hits_dom.ensure(sizeof(wh_domain) * (size_t)ndom + 16)) return WH_ENOMEM;
  wh_domain *d_dom = (wh_domain *)e->d_hits_dom.p;
  const int64_t *d_env = nullptr;
  const int32_t *d_cols = nullptr;
  const float *d_pp = nullptr;
  int64_t total_env = 0;
  if (int rc = wh_domain_paths_dev(e, d_res, d_off, nq, total, max_query_len(offsets, nq), d_flags, d_det, d_doff, d_dom, &d_env, &d_cols, &d_pp,
                                   &total_env, nullptr)) {
    const std::string why = wh_last_error();      // (the stage names its own entry point: say whose call it was)
    set_error("%s: %s", who, why.c_str());
    return rc;
  }
  if (int rc = wh_hits_msa_dev(e, d_text, d_off, nq, d_flags, d_det, d_doff, d_dom, d_env, d_cols, d_pp, h, d_order, opts, msa_flags, out_nrows,
                               out_rows_rec, out_W, out_rows, out_pp_rows, out_pp_cons, out_rf, out_matmap, nullptr))
    return rc;
  if (out_dom && ndom > 0) {
    const hipError_t err = hipMemcpy(out_dom, d_dom, sizeof(wh_domain) * (size_t)ndom, hipMemcpyDeviceToHost);
    if (err != hipSuccess) {
      free(*out_rows_rec); free(*out_rows); free(*out_pp_rows); free(*out_pp_cons); free(*out_rf); free(*out_matmap);
      *out_rows_rec = nullptr; *out_rows = *out_pp_rows = *out_pp_cons = *out_rf = nullptr; *out_matmap = nullptr; *out_nrows = 0;
      set_error("%s: copying the domain records back failed: %s", who, hipGetErrorString(err));
      return WH_EHIP;
    }
  }
  return WH_OK;
}

}  // extern "C"
