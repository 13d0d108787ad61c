// Host side of hmmsearch's alignment display (include/witch_hip.h: wh_ehmm_consensus, wh_domain_display_dev,
// wh_domain_display): the kernels of wh_display.hip behind the domain stage (wh_domain_paths_dev), and the models' display
// tables, which are built and uploaded at the first display call of a model.
#include <string>

#include "wh_host.h"

struct DisplayState {
  std::map<int, DevBuf> tab;      // model position -> odds [(M + 1) x Kp] floats | cons [M + 1] | code [M + 1] | sym [32]
  DevBuf work;                    // scan workspace of a call
  DevBuf dom, off, recs, lines;   // wh_domain_display: the domain records, and the outputs before they are copied back
};
void wh_ehmm::DisplayStateDelete::operator()(DisplayState *f) const { delete f; }

namespace {

int check_display_args(const char *who, const wh_ehmm *e, int32_t h, double domE, double domZ) {
  if (!(domZ > 0.0)) { set_error("%s: domZ = %g must be > 0", who, domZ); return WH_EINVAL; }
  if (!(domE >= 0.0)) { set_error("%s: domE = %g must be >= 0", who, domE); return WH_EINVAL; }
  if (h < 0) { set_error("%s: model position %d out of range", who, h); return WH_EINVAL; }
  if (!e) { set_error("%s: null handle", who); return WH_EINVAL; }
  if (h >= (int)e->hmms.size()) { set_error("%s: model position %d out of range (0..%d)", who, h, (int)e->hmms.size() - 1); return WH_EINVAL; }
  const HostHMM &m = e->hmms[(size_t)h];
  // HMMER prints an RF and a CS line above the model line for such models, and no model line can be printed without CONS
  if (!m.has_cons) { set_error("%s: model %s has no consensus line (header key CONS is not \"yes\"): its alignments cannot be displayed", who, m.name.c_str()); return WH_EINVAL; }
  if (m.has_rf) { set_error("%s: model %s has a reference line (header key RF yes): its display is not implemented", who, m.name.c_str()); return WH_EINVAL; }
  if (m.has_cs) { set_error("%s: model %s has a consensus structure line (header key CS yes): its display is not implemented", who, m.name.c_str()); return WH_EINVAL; }
  return WH_OK;
}

// the display table of model h on the device: made at the first call that needs it
int display_table(wh_ehmm *e, int32_t h, DisplayArgs &a) {
  if (!e->display) e->display.reset(new DisplayState);
  const HostHMM &m = e->hmms[(size_t)h];
  const size_t M1 = (size_t)m.M + 1, Kp = (size_t)m.Kp;
  const size_t cons_at = sizeof(float) * M1 * Kp, code_at = cons_at + M1, sym_at = code_at + M1, bytes = sym_at + 32;
  auto it = e->display->tab.find(h);
  if (it == e->display->tab.end()) {
    std::vector<uint8_t> host(bytes, 0);
    float *odds = (float *)host.data();
    // the float32 value of the odds ratio the scoring tables hold (wh_hmm.cpp: build_tables), node-major here
    for (size_t k = 1; k < M1; k++)
      for (size_t x = 0; x < Kp; x++) odds[k * Kp + x] = (float)m.odds[x * M1 + k];
    for (size_t k = 1; k < M1; k++) host[cons_at + k] = (uint8_t)m.cons[k];
    digitize(m.alphabet, m.cons.data() + 1, (int64_t)m.M, host.data() + code_at + 1);
    // the alphabet's symbols: what digitize maps back onto 0 .. Kp - 1
    for (int c = 33; c < 127; c++) {
      const char ch = (char)c;
      uint8_t x = 255;
      if (ch >= 'a' && ch <= 'z') continue;
      if (digitize(m.alphabet, &ch, 1, &x) == 0 && x < 32 && host[sym_at + x] == 0) host[sym_at + x] = (uint8_t)c;
    }
    DevBuf &b = e->display->tab[h];
    if (b.ensure(bytes)) { e->display->tab.erase(h); return WH_ENOMEM; }
    const hipError_t err = hipMemcpy(b.p, host.data(), bytes, hipMemcpyHostToDevice);
    if (err != hipSuccess) { e->display->tab.erase(h); set_error("uploading the display table failed: %s", hipGetErrorString(err)); return WH_EHIP; }
    it = e->display->tab.find(h);
  }
  const uint8_t *p = (const uint8_t *)it->second.p;
  a.tab_odds = (const float *)p; a.tab_cons = p + cons_at; a.tab_code = p + code_at; a.tab_sym = p + sym_at;
  return WH_OK;
}

}  // namespace

extern "C" {

int wh_ehmm_consensus(const wh_ehmm *e, int h, char *out, int32_t *present) {
  if (!e || h < 0 || h >= (int)e->hmms.size() || !present) { set_error("wh_ehmm_consensus: bad argument"); return WH_EINVAL; }
  const HostHMM &m = e->hmms[(size_t)h];
  *present = m.has_cons ? 1 : 0;
  if (m.has_cons && out) memcpy(out, m.cons.data() + 1, (size_t)m.M);
  return WH_OK;
}

int wh_hmm_consensus(const char *hmm_path, char *out, int32_t cap, int32_t *out_M, int32_t *present) {
  if (!hmm_path || !present || cap < 0) { set_error("wh_hmm_consensus: bad argument"); return WH_EINVAL; }
  HostHMM m;
  if (int rc = parse_hmm_file(hmm_path, m)) return rc;
  if (out_M) *out_M = m.M;
  *present = (m.has_cons ? 1 : 0) | (m.has_rf ? 2 : 0) | (m.has_cs ? 4 : 0);
  if (m.has_cons && out) memcpy(out, m.cons.data() + 1, (size_t)std::min<int32_t>(cap, m.M));
  return WH_OK;
}

int wh_domain_display_dev(wh_ehmm *e, const uint8_t *d_residues, const int64_t *d_offsets, int64_t nq, const uint8_t *d_flags,
                          const int64_t *d_dom_off, const wh_domain *d_dom, const int64_t *d_env_off, const int32_t *d_cols,
                          const float *d_pp, int32_t h, double domE, double domZ, int64_t cap, int64_t *d_disp_off,
                          wh_display_rec *d_recs, uint8_t *d_model, uint8_t *d_match, uint8_t *d_target, uint8_t *d_ppline,
                          int64_t *out_nsel, int64_t *out_total, void *stream) {
  const char *who = "wh_domain_display_dev";
  if (int rc = check_display_args(who, e, h, domE, domZ)) return rc;
  if (nq < 0 || cap < 0 || !out_nsel || !out_total || !d_disp_off || (nq > 0 && (!d_offsets || !d_flags || !d_dom_off))) {
    set_error("%s: bad argument", who);
    return WH_EINVAL;
  }
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipSetDevice(e->device));
  const int H = (int)e->hmms.size();
  const int64_t npairs = nq * H;
  if (npairs > 0x7FFFFFFF) { set_error("%s: too many pairs", who); return WH_ERANGE; }
  e->timers[9].launches = 0; e->timers[9].ms = 0; e->timers[9].pending = false;
  *out_nsel = 0; *out_total = 0;
  const int64_t zero = 0;
  int64_t ndom = 0;
  if (npairs > 0) {
    HIPCHK(hipMemcpyAsync(&ndom, d_dom_off + npairs, sizeof ndom, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (ndom < 0 || ndom > npairs * WH_MAX_ENVELOPES) { set_error("%s: dom_off ends at %lld for %lld pairs", who, (long long)ndom, (long long)npairs); return WH_EINVAL; }
    if (ndom > 0 && (!d_dom || !d_env_off || !d_cols || !d_pp || !d_residues || !d_recs)) { set_error("%s: bad argument", who); return WH_EINVAL; }
  }
  if (ndom == 0) {               // nothing to display: the CSR of no lines
    HIPCHK(hipMemcpyAsync(d_disp_off, &zero, sizeof zero, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    return WH_OK;
  }
  const HostHMM &m = e->hmms[(size_t)h];
  DisplayArgs a;
  memset(&a, 0, sizeof a);
  if (int rc = display_table(e, h, a)) return rc;
  a.flags = d_flags; a.dom_off = d_dom_off; a.dom = d_dom; a.npairs = npairs; a.ndom = ndom; a.nq = nq; a.H = H; a.h = h; a.M = m.M; a.Kp = m.Kp;
  a.residues = d_residues; a.offsets = d_offsets; a.env_off = d_env_off; a.cols = d_cols; a.pp = d_pp;
  a.ln_rep_dom = domE > 0.0 ? std::log(domE / domZ) : -INFINITY;
  a.nblk = display_scan_blocks(ndom);
  // work: totals [2] | bad [1 int, padded] | blk_sel [nblk] | blk_len [nblk] | pos_len [ndom] (8-byte words), then len [ndom] | pos_sel [ndom] (ints)
  const size_t n8 = 3 + 2 * (size_t)a.nblk + (size_t)ndom;
  DevBuf &work = e->display->work;
  if (work.ensure(n8 * 8 + sizeof(int32_t) * 2 * (size_t)ndom + 16)) return WH_ENOMEM;
  long long *w8 = (long long *)work.p;
  a.totals = w8; a.bad = (int *)(w8 + 2); a.blk_sel = w8 + 3; a.blk_len = a.blk_sel + a.nblk; a.pos_len = a.blk_len + a.nblk;
  a.len = (int32_t *)(w8 + n8); a.pos_sel = a.len + ndom;
  a.disp_off = d_disp_off; a.recs = d_recs; a.model = d_model; a.match = d_match; a.target = d_target; a.ppline = d_ppline;
  if (timer_begin(e, 9, s)) return WH_EHIP;
  HIPCHK(hipMemsetAsync(w8, 0, 3 * sizeof(long long), s));
  hipError_t err = launch_display_count(a, s);
  if (err == hipSuccess) err = launch_display_scan(a, s);
  if (err != hipSuccess) { set_error("%s: count / scan kernels failed to launch: %s", who, hipGetErrorString(err)); return WH_EHIP; }
  // the number of selected domains and their columns come back once: they are checked against the caller's arrays
  long long tot[3] = {0, 0, 0};
  HIPCHK(hipMemcpyAsync(tot, w8, sizeof tot, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if ((int)tot[2] != 0) { set_error("%s: a domain record does not fit dom_off, its envelope, its query or its path (nodes rising from hmm_i to hmm_j)", who); return WH_EINVAL; }
  a.nsel = tot[0]; a.total = tot[1];
  if (a.nsel < 0 || a.nsel > ndom || a.total < a.nsel) { set_error("%s: internal error: %lld selected domains of %lld, %lld columns", who, tot[0], (long long)ndom, tot[1]); return WH_EINVAL; }
  *out_total = a.total;
  if (a.total > cap) { set_error("%s: the lines take %lld bytes each, the arrays hold %lld", who, tot[1], (long long)cap); return WH_ERANGE; }
  if (a.nsel == 0) {
    HIPCHK(hipMemcpyAsync(d_disp_off, &zero, sizeof zero, hipMemcpyHostToDevice, s));
    if (timer_end(e, 9, s, 3)) return WH_EHIP;
    HIPCHK(hipStreamSynchronize(s));
    return WH_OK;
  }
  if (!d_model || !d_match || !d_target || !d_ppline) { set_error("%s: bad argument (no room for the lines)", who); return WH_EINVAL; }
  err = launch_display_render(a, s);
  if (err != hipSuccess) { set_error("%s: render kernel failed to launch: %s", who, hipGetErrorString(err)); return WH_EHIP; }
  if (timer_end(e, 9, s, 4)) return WH_EHIP;
  *out_nsel = a.nsel;
  return WH_OK;
}

int wh_domain_display(wh_ehmm *e, const uint8_t *residues, const int64_t *offsets, int64_t nq, const uint8_t *flags,
                      const wh_pair_detail *detail, const int64_t *dom_off, int32_t h, double domE, double domZ,
                      wh_domain *out_dom, int64_t *out_nsel, int64_t **out_disp_off, wh_display_rec **out_recs,
                      uint8_t **out_model, uint8_t **out_match, uint8_t **out_target, uint8_t **out_pp) {
  const char *who = "wh_domain_display";
  if (int rc = check_display_args(who, e, h, domE, domZ)) return rc;
  if (nq < 0 || !out_nsel || !out_disp_off || !out_recs || !out_model || !out_match || !out_target || !out_pp ||
      (nq > 0 && (!residues || !offsets || !flags || !detail || !dom_off))) {
    set_error("%s: bad argument", who);
    return WH_EINVAL;
  }
  *out_nsel = 0; *out_disp_off = nullptr; *out_recs = nullptr; *out_model = *out_match = *out_target = *out_pp = nullptr;
  if (nq == 0) return WH_OK;
  HIPCHK(hipSetDevice(e->device));
  const size_t np = (size_t)nq * e->hmms.size();
  const int64_t total = offsets[nq], ndom = dom_off[np];
  if (total < 0 || offsets[0] != 0 || ndom < 0) { set_error("%s: bad offsets", who); return WH_EINVAL; }
  if (check_residues(e->Kp, residues, total)) return WH_EINVAL;
  if (ndom == 0) return WH_OK;
  if (!e->display) e->display.reset(new DisplayState);
  DisplayState &st8 = *e->display;
  Staging st(e);
  const uint8_t *d_res = st.in(residues, (size_t)total, 16);
  const int64_t *d_off = st.in(offsets, sizeof(int64_t) * (size_t)(nq + 1));
  const uint8_t *d_flags = st.in(flags, np);
  const wh_pair_detail *d_det = st.in(detail, sizeof(wh_pair_detail) * np);
  const int64_t *d_doff = st.in(dom_off, sizeof(int64_t) * (np + 1));
  if (st.rc) return st.rc;
  if (st8.dom.ensure(sizeof(wh_domain) * (size_t)ndom + 16)) return WH_ENOMEM;
  wh_domain *d_dom = (wh_domain *)st8.dom.p;
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
  // room for every domain, selected or not: its nodes and its envelope's residues
  const int64_t cap = ndom * (int64_t)e->hmms[(size_t)h].M + total_env;
  if (st8.off.ensure(sizeof(int64_t) * ((size_t)ndom + 1)) || st8.recs.ensure(sizeof(wh_display_rec) * (size_t)ndom + 16) || st8.lines.ensure(4 * (size_t)cap + 16))
    return WH_ENOMEM;
  uint8_t *lines = (uint8_t *)st8.lines.p;
  int64_t nsel = 0, tot = 0;
  if (int rc = wh_domain_display_dev(e, d_res, d_off, nq, d_flags, d_doff, d_dom, d_env, d_cols, d_pp, h, domE, domZ, cap, (int64_t *)st8.off.p,
                                     (wh_display_rec *)st8.recs.p, lines, lines + cap, lines + 2 * cap, lines + 3 * cap, &nsel, &tot, nullptr))
    return rc;
  HIPCHK(hipDeviceSynchronize());
  if (out_dom) HIPCHK(hipMemcpy(out_dom, d_dom, sizeof(wh_domain) * (size_t)ndom, hipMemcpyDeviceToHost));
  if (nsel == 0) return WH_OK;
  int64_t *h_off = (int64_t *)malloc(sizeof(int64_t) * ((size_t)nsel + 1));
  wh_display_rec *h_recs = (wh_display_rec *)malloc(sizeof(wh_display_rec) * (size_t)nsel);
  uint8_t *h_lines[4] = {nullptr, nullptr, nullptr, nullptr};
  bool mem = h_off && h_recs;
  for (int t = 0; t < 4; t++) { h_lines[t] = (uint8_t *)malloc((size_t)tot + 1); mem = mem && h_lines[t]; }
  hipError_t err = hipSuccess;
  if (mem) err = hipMemcpy(h_off, st8.off.p, sizeof(int64_t) * ((size_t)nsel + 1), hipMemcpyDeviceToHost);
  if (mem && err == hipSuccess) err = hipMemcpy(h_recs, st8.recs.p, sizeof(wh_display_rec) * (size_t)nsel, hipMemcpyDeviceToHost);
  for (int t = 0; t < 4 && mem && err == hipSuccess; t++) err = hipMemcpy(h_lines[t], lines + (size_t)t * cap, (size_t)tot, hipMemcpyDeviceToHost);
  if (!mem || err != hipSuccess) {
    free(h_off); free(h_recs);
    for (int t = 0; t < 4; t++) free(h_lines[t]);
    if (!mem) { set_error("%s: out of host memory (%lld domains, %lld columns)", who, (long long)nsel, (long long)tot); return WH_ENOMEM; }
    set_error("%s: copying the lines back failed: %s", who, hipGetErrorString(err));
    return WH_EHIP;
  }
  *out_nsel = nsel; *out_disp_off = h_off; *out_recs = h_recs;
  *out_model = h_lines[0]; *out_match = h_lines[1]; *out_target = h_lines[2]; *out_pp = h_lines[3];
  return WH_OK;
}

}  // extern "C"
