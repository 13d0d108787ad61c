// Host side of the per-domain results (include/witch_hip.h: wh_domain_counts, wh_domains, wh_domain_paths, wh_ehmm_evparams):
// the kernels of wh_domains.hip around one wh_align_pp_dev call on the packed envelopes.
#include <limits>

#include "wh_host.h"

extern "C" {

int wh_ehmm_evparams(const wh_ehmm *e, float *tau, float *lambda, int32_t *present) {
  if (!e) { set_error("wh_ehmm_evparams: null handle"); return WH_EINVAL; }
  const float nan = std::numeric_limits<float>::quiet_NaN();
  for (size_t i = 0; i < e->hmms.size(); i++) {
    const HostHMM &h = e->hmms[i];
    if (tau) tau[i] = h.has_fstats ? h.ftau : nan;
    if (lambda) lambda[i] = h.has_fstats ? h.flambda : nan;
    if (present) present[i] = h.has_fstats ? 1 : 0;
  }
  return WH_OK;
}

int wh_hmm_evparams(const char *hmm_path, float *tau, float *lambda, int32_t *present) {
  if (!hmm_path) { set_error("wh_hmm_evparams: bad argument"); return WH_EINVAL; }
  HostHMM h;
  if (int rc = parse_hmm_file(hmm_path, h)) return rc;
  const float nan = std::numeric_limits<float>::quiet_NaN();
  if (tau) *tau = h.has_fstats ? h.ftau : nan;
  if (lambda) *lambda = h.has_fstats ? h.flambda : nan;
  if (present) *present = h.has_fstats ? 1 : 0;
  return WH_OK;
}

int wh_set_domain_length_model(wh_ehmm *e, int model) {
  if (model != WH_LENMODEL_ENVELOPE && model != WH_LENMODEL_SEQUENCE) { set_error("wh_set_domain_length_model: unknown length model %d (WH_LENMODEL_ENVELOPE = %d, WH_LENMODEL_SEQUENCE = %d)", model, WH_LENMODEL_ENVELOPE, WH_LENMODEL_SEQUENCE); return WH_EINVAL; }
  if (!e) { set_error("wh_set_domain_length_model: null handle"); return WH_EINVAL; }
  e->dom_lenmodel = model;
  return WH_OK;
}

int wh_get_domain_length_model(const wh_ehmm *e) {
  if (!e) { set_error("wh_get_domain_length_model: null handle"); return WH_EINVAL; }
  return e->dom_lenmodel;
}

int wh_domain_counts_dev(wh_ehmm *e, const uint8_t *d_flags, const wh_pair_detail *d_detail, int64_t nq,
                         int32_t *d_counts, int32_t *d_n_unlisted, void *stream) {
  if (!e || !d_flags || !d_detail || !d_counts || nq < 0) { set_error("wh_domain_counts_dev: bad argument"); return WH_EINVAL; }
  HIPCHK(hipSetDevice(e->device));
  DomainArgs a;
  memset(&a, 0, sizeof a);
  a.flags = d_flags; a.detail = d_detail; a.H = (int)e->hmms.size(); a.npairs = nq * a.H;
  a.counts = d_counts; a.n_unlisted = d_n_unlisted;
  if (a.npairs > 0x7FFFFFFF) { set_error("too many pairs"); return WH_ERANGE; }
  hipError_t err = launch_domain_count(a, (hipStream_t)stream);
  if (err != hipSuccess) { set_error("domain count kernel launch failed: %s", hipGetErrorString(err)); return WH_EHIP; }
  return WH_OK;
}

}  // extern "C"

namespace {

// The domain stage, for wh_domains_dev and wh_domain_paths_dev (<who>) alike: both run these steps.  What the stage leaves in
// the handle's workspace - the envelope CSR (d_env_off), the alignment's columns (d_dom_cols) and posteriors (d_dom_pp) -
// is what wh_domain_paths_dev hands on; <out_ndom>, <out_total_env> (optional): the domains and the envelope residues.
int domains_run(const char *who, wh_ehmm *e, const uint8_t *d_residues, const int64_t *d_offsets, int64_t nq,
                int32_t max_len, const uint8_t *d_flags, const wh_pair_detail *d_detail, const int64_t *d_dom_off,
                wh_domain *d_out, int64_t *out_ndom, int64_t *out_total_env, void *stream) {
  if (out_ndom) *out_ndom = 0;
  if (out_total_env) *out_total_env = 0;
  if (!e || !d_residues || !d_offsets || !d_flags || !d_detail || !d_dom_off || nq < 0 || max_len < 0) { set_error("%s: bad argument", who); return WH_EINVAL; }
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipSetDevice(e->device));
  const int H = (int)e->hmms.size();
  const int64_t npairs = nq * H;
  if (npairs > 0x7FFFFFFF) { set_error("too many pairs"); return WH_ERANGE; }
  e->timers[5].launches = 0; e->timers[5].ms = 0; e->timers[5].pending = false;
  if (npairs == 0) return WH_OK;
  int64_t ndom = 0;
  HIPCHK(hipMemcpyAsync(&ndom, d_dom_off + npairs, sizeof ndom, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (ndom < 0 || ndom > npairs * WH_MAX_ENVELOPES || ndom > 0x7FFFFFFF) { set_error("%s: dom_off ends at %lld for %lld pairs", who, (long long)ndom, (long long)npairs); return WH_EINVAL; }
  if (ndom > 0 && !d_out) { set_error("%s: bad argument", who); return WH_EINVAL; }
  // Forward tau / lambda per model, uploaded once per handle, on the call's stream, from a vector the handle keeps
  if (!e->d_evp.p) {
    e->h_evp.assign((size_t)2 * H, std::numeric_limits<float>::quiet_NaN());
    for (int h = 0; h < H; h++) {
      const HostHMM &m = e->hmms[(size_t)h];
      if (m.has_fstats) { e->h_evp[(size_t)2 * h] = m.ftau; e->h_evp[(size_t)2 * h + 1] = m.flambda; }
    }
    if (e->d_evp.ensure(sizeof(float) * e->h_evp.size())) return WH_ENOMEM;
    HIPCHK(hipMemcpyAsync(e->d_evp.p, e->h_evp.data(), sizeof(float) * e->h_evp.size(), hipMemcpyHostToDevice, s));
  }
  // (dom_len: ndom lengths, then the word the list kernel sets when dom_off does not match the records)
  if (e->d_dom_pair.ensure(sizeof(int64_t) * (size_t)ndom + 8) || e->d_dom_len.ensure(sizeof(int32_t) * ((size_t)ndom + 1)) ||
      e->d_env_off.ensure(sizeof(int64_t) * ((size_t)ndom + 1)) || e->d_dom_q.ensure(sizeof(int64_t) * (size_t)ndom + 8) ||
      e->d_dom_h.ensure(sizeof(int32_t) * (size_t)ndom + 8))
    return WH_ENOMEM;
  const bool seq_model = e->dom_lenmodel == WH_LENMODEL_SEQUENCE;
  if (seq_model && e->d_dom_seqlen.ensure(sizeof(int32_t) * (size_t)ndom + 8)) return WH_ENOMEM;
  if (timer_begin(e, 5, s)) return WH_EHIP;
  DomainArgs a;
  memset(&a, 0, sizeof a);
  a.flags = d_flags; a.detail = d_detail; a.npairs = npairs; a.H = H;
  a.dom_off = d_dom_off; a.ndom = ndom;
  a.dom_pair = (int64_t *)e->d_dom_pair.p; a.dom_len = (int32_t *)e->d_dom_len.p; a.bad = (int *)e->d_dom_len.p + ndom;
  a.residues = d_residues; a.offsets = d_offsets;
  a.dom_seqlen = seq_model ? (int32_t *)e->d_dom_seqlen.p : nullptr;
  // every length starts as -1 (a slot the list kernel does not reach is refused like a malformed envelope), the word as 0
  if (ndom > 0) HIPCHK(hipMemsetAsync(a.dom_len, 0xFF, sizeof(int32_t) * (size_t)ndom, s));
  HIPCHK(hipMemsetAsync(a.bad, 0, sizeof(int), s));
  hipError_t err = launch_domain_list(a, s);
  if (err != hipSuccess) { set_error("domain list kernel launch failed: %s", hipGetErrorString(err)); return WH_EHIP; }
  std::vector<int32_t> len((size_t)ndom + 1);
  HIPCHK(hipMemcpyAsync(len.data(), a.dom_len, sizeof(int32_t) * len.size(), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (len[(size_t)ndom] != 0) { set_error("%s: dom_off is not the prefix sum of wh_domain_counts over these flags and detail records", who); return WH_EINVAL; }
  std::vector<int64_t> &env_off = e->h_env_off;      // (the handle's: the upload below needs it beyond this function's return)
  env_off.assign((size_t)ndom + 1, 0);
  int32_t max_env = 0;
  for (int64_t d = 0; d < ndom; d++) {
    if (len[(size_t)d] < 1) { set_error("%s: domain %lld has an envelope outside its query (or dom_off skips it)", who, (long long)d); return WH_EINVAL; }
    env_off[(size_t)d + 1] = env_off[(size_t)d] + len[(size_t)d];
    max_env = std::max(max_env, len[(size_t)d]);
  }
  if (max_env > max_len) { set_error("%s: an envelope of %d residues, but max_len is %d", who, max_env, max_len); return WH_EINVAL; }
  const int64_t total_env = env_off[(size_t)ndom];
  int launches = 1;
  if (ndom > 0) {
    if (e->d_env_res.ensure((size_t)total_env + 16) || e->d_dom_cols.ensure(sizeof(int32_t) * (size_t)total_env + 16) ||
        e->d_dom_pp.ensure(sizeof(float) * (size_t)total_env + 16))
      return WH_ENOMEM;
    HIPCHK(hipMemcpyAsync(e->d_env_off.p, env_off.data(), sizeof(int64_t) * env_off.size(), hipMemcpyHostToDevice, s));
    a.env_off = (const int64_t *)e->d_env_off.p; a.env_res = (uint8_t *)e->d_env_res.p;
    a.dom_q = (int64_t *)e->d_dom_q.p; a.dom_h = (int32_t *)e->d_dom_h.p;
    err = launch_envelope_gather(a, s);
    if (err != hipSuccess) { set_error("envelope gather kernel launch failed: %s", hipGetErrorString(err)); return WH_EHIP; }
    // the alignment: "query" d is envelope d, its model the pair's; one pair per envelope, so its columns share the CSR.
    // Its length model is the envelope's own (a null d_cfg_len) or, under WH_LENMODEL_SEQUENCE, the sequence's
    int rc = wh_align_pp_len_dev(e, a.env_res, a.env_off, ndom, total_env, max_env, a.dom_q, a.dom_h, ndom, a.env_off,
                                 (int32_t *)e->d_dom_cols.p, (float *)e->d_dom_pp.p, a.dom_seqlen, s);
    if (rc) return rc;
    a.cols = (const int32_t *)e->d_dom_cols.p; a.pp = (const float *)e->d_dom_pp.p; a.evp = (const float *)e->d_evp.p; a.out = d_out;
    err = launch_domain_summary(a, s);
    if (err != hipSuccess) { set_error("domain summary kernel launch failed: %s", hipGetErrorString(err)); return WH_EHIP; }
    launches = 3 + e->timers[2].launches;
  }
  if (timer_end(e, 5, s, launches)) return WH_EHIP;
  if (out_ndom) *out_ndom = ndom;
  if (out_total_env) *out_total_env = total_env;
  return WH_OK;
}

}  // namespace

extern "C" {

int wh_domains_dev(wh_ehmm *e, const uint8_t *d_residues, const int64_t *d_offsets, int64_t nq, int64_t total_residues,
                   int32_t max_len, const uint8_t *d_flags, const wh_pair_detail *d_detail, const int64_t *d_dom_off,
                   wh_domain *d_out, void *stream) {
  (void)total_residues;          // (as in wh_align_dev: the residues are read through the offsets)
  return domains_run("wh_domains_dev", e, d_residues, d_offsets, nq, max_len, d_flags, d_detail, d_dom_off, d_out, nullptr, nullptr, stream);
}

int wh_domain_paths_dev(wh_ehmm *e, const uint8_t *d_residues, const int64_t *d_offsets, int64_t nq, int64_t total_residues,
                        int32_t max_len, const uint8_t *d_flags, const wh_pair_detail *d_detail, const int64_t *d_dom_off,
                        wh_domain *d_out, const int64_t **d_env_off, const int32_t **d_cols, const float **d_pp,
                        int64_t *total_env, void *stream) {
  (void)total_residues;
  if (!d_env_off || !d_cols || !d_pp || !total_env) { set_error("wh_domain_paths_dev: bad argument"); return WH_EINVAL; }
  *d_env_off = nullptr; *d_cols = nullptr; *d_pp = nullptr;
  int64_t ndom = 0;
  if (int rc = domains_run("wh_domain_paths_dev", e, d_residues, d_offsets, nq, max_len, d_flags, d_detail, d_dom_off, d_out, &ndom, total_env, stream)) return rc;
  if (ndom == 0) {               // no domain: a CSR of one entry (the stage above uploaded none)
    if (e->d_env_off.ensure(sizeof(int64_t))) return WH_ENOMEM;
    HIPCHK(hipMemsetAsync(e->d_env_off.p, 0, sizeof(int64_t), (hipStream_t)stream));
  } else {
    *d_cols = (const int32_t *)e->d_dom_cols.p; *d_pp = (const float *)e->d_dom_pp.p;
  }
  *d_env_off = (const int64_t *)e->d_env_off.p;
  return WH_OK;
}

int wh_domain_counts(wh_ehmm *e, const uint8_t *flags, const wh_pair_detail *detail, int64_t nq, int32_t *counts, int32_t *n_unlisted) {
  if (!e || !flags || !detail || !counts || nq < 0) { set_error("wh_domain_counts: bad argument"); return WH_EINVAL; }
  if (nq == 0) return WH_OK;
  HIPCHK(hipSetDevice(e->device));
  const size_t np = (size_t)nq * e->hmms.size();
  Staging st(e);
  const uint8_t *d_flags = st.in(flags, np);
  const wh_pair_detail *d_det = st.in(detail, sizeof(wh_pair_detail) * np);
  int32_t *d_cnt = st.out(counts, sizeof(int32_t) * np);
  int32_t *d_unl = st.out(n_unlisted, sizeof(int32_t) * np);
  if (st.rc) return st.rc;
  return st.finish(wh_domain_counts_dev(e, d_flags, d_det, nq, d_cnt, d_unl, nullptr));
}

int wh_domains(wh_ehmm *e, const uint8_t *residues, const int64_t *offsets, int64_t nq, const uint8_t *flags,
               const wh_pair_detail *detail, const int64_t *dom_off, wh_domain *out) {
  if (!e || !residues || !offsets || !flags || !detail || !dom_off || nq < 0) { set_error("wh_domains: bad argument"); return WH_EINVAL; }
  if (nq == 0) return WH_OK;
  HIPCHK(hipSetDevice(e->device));
  const size_t np = (size_t)nq * e->hmms.size();
  const int64_t total = offsets[nq], ndom = dom_off[np];
  if (ndom < 0 || (ndom > 0 && !out)) { set_error("wh_domains: bad argument"); return WH_EINVAL; }
  if (check_residues(e->Kp, residues, total)) return WH_EINVAL;
  Staging st(e);
  const uint8_t *d_res = st.in(residues, (size_t)total, 16);
  const int64_t *d_off = st.in(offsets, sizeof(int64_t) * (size_t)(nq + 1));
  const uint8_t *d_flags = st.in(flags, np);
  const wh_pair_detail *d_det = st.in(detail, sizeof(wh_pair_detail) * np);
  const int64_t *d_doff = st.in(dom_off, sizeof(int64_t) * (np + 1));
  wh_domain *d_out = st.out(out, sizeof(wh_domain) * (size_t)ndom, 16);
  if (st.rc) return st.rc;
  return st.finish(wh_domains_dev(e, d_res, d_off, nq, total, max_query_len(offsets, nq), d_flags, d_det, d_doff, d_out, nullptr));
}

int wh_domain_paths(wh_ehmm *e, const uint8_t *residues, const int64_t *offsets, int64_t nq, const uint8_t *flags,
                    const wh_pair_detail *detail, const int64_t *dom_off, wh_domain *out, int64_t *env_off, int32_t **out_cols,
                    float **out_pp) {
  if (!e) { set_error("wh_domain_paths: null handle"); return WH_EINVAL; }
  if (!residues || !offsets || !flags || !detail || !dom_off || !env_off || !out_cols || !out_pp || nq < 0) { set_error("wh_domain_paths: bad argument"); return WH_EINVAL; }
  *out_cols = nullptr; *out_pp = nullptr; env_off[0] = 0;
  if (nq == 0) return WH_OK;
  HIPCHK(hipSetDevice(e->device));
  const size_t np = (size_t)nq * e->hmms.size();
  const int64_t total = offsets[nq], ndom = dom_off[np];
  if (ndom < 0 || (ndom > 0 && !out)) { set_error("wh_domain_paths: bad argument"); return WH_EINVAL; }
  if (check_residues(e->Kp, residues, total)) return WH_EINVAL;
  Staging st(e);
  const uint8_t *d_res = st.in(residues, (size_t)total, 16);
  const int64_t *d_off = st.in(offsets, sizeof(int64_t) * (size_t)(nq + 1));
  const uint8_t *d_flags = st.in(flags, np);
  const wh_pair_detail *d_det = st.in(detail, sizeof(wh_pair_detail) * np);
  const int64_t *d_doff = st.in(dom_off, sizeof(int64_t) * (np + 1));
  wh_domain *d_out = st.out(out, sizeof(wh_domain) * (size_t)ndom, 16);
  if (st.rc) return st.rc;
  const int64_t *d_env = nullptr;
  const int32_t *d_cols = nullptr;
  const float *d_pp = nullptr;
  int64_t total_env = 0;
  if (int rc = st.finish(wh_domain_paths_dev(e, d_res, d_off, nq, total, max_query_len(offsets, nq), d_flags, d_det, d_doff, d_out, &d_env,
                                             &d_cols, &d_pp, &total_env, nullptr)))
    return rc;
  if (ndom == 0 || total_env == 0) return WH_OK;
  int32_t *cols = (int32_t *)malloc(sizeof(int32_t) * (size_t)total_env);
  float *pp = (float *)malloc(sizeof(float) * (size_t)total_env);
  hipError_t err = cols && pp ? hipSuccess : hipErrorOutOfMemory;
  if (err == hipSuccess) err = hipMemcpy(env_off, d_env, sizeof(int64_t) * ((size_t)ndom + 1), hipMemcpyDeviceToHost);
  if (err == hipSuccess) err = hipMemcpy(cols, d_cols, sizeof(int32_t) * (size_t)total_env, hipMemcpyDeviceToHost);
  if (err == hipSuccess) err = hipMemcpy(pp, d_pp, sizeof(float) * (size_t)total_env, hipMemcpyDeviceToHost);
  if (err != hipSuccess) { free(cols); free(pp); set_error("wh_domain_paths: copying the paths back failed: %s", hipGetErrorString(err)); return cols && pp ? WH_EHIP : WH_ENOMEM; }
  *out_cols = cols; *out_pp = pp;
  return WH_OK;
}

}  // extern "C"
