// Host side of the multi-sequence alignment (include/witch_hip.h: wh_msa_dev, wh_msa): the kernels of wh_msa.hip behind
// one wh_align_pp_dev call for the pairs (q, h).
#include "wh_host.h"

namespace {

// the buffers a call returns; what a failed call has allocated is released
struct MsaOut {
  uint8_t *rows = nullptr, *pp_rows = nullptr, *pp_cons = nullptr, *rf = nullptr;
  int32_t *matmap = nullptr;
  ~MsaOut() { free(rows); free(pp_rows); free(pp_cons); free(rf); free(matmap); }
  int alloc(int64_t nq, int64_t W, int M, const char *who) {
    const size_t nb = (size_t)nq * (size_t)W;
    rows = (uint8_t *)malloc(nb + 1); pp_rows = (uint8_t *)malloc(nb + 1);
    pp_cons = (uint8_t *)malloc((size_t)W + 1); rf = (uint8_t *)malloc((size_t)W + 1);
    matmap = (int32_t *)malloc(sizeof(int32_t) * ((size_t)M + 1));
    if (!rows || !pp_rows || !pp_cons || !rf || !matmap) { set_error("%s: out of host memory (%lld rows x %lld columns)", who, (long long)nq, (long long)W); return WH_ENOMEM; }
    return WH_OK;
  }
  void give(uint8_t **o_rows, uint8_t **o_pp_rows, uint8_t **o_pp_cons, uint8_t **o_rf, int32_t **o_matmap) {
    *o_rows = rows; *o_pp_rows = pp_rows; *o_pp_cons = pp_cons; *o_rf = rf; *o_matmap = matmap;
    rows = pp_rows = pp_cons = rf = nullptr; matmap = nullptr;
  }
};

constexpr size_t kMsaChunkBytes = (size_t)64 << 20;     // of the posterior matrix [rows of a chunk][M] the PP_cons kernel reads

}  // namespace

extern "C" {

int wh_msa_dev(wh_ehmm *e, const int32_t *d_cols, const float *d_pp, const uint8_t *d_text, const int64_t *d_offsets, int64_t nq,
               int64_t total_residues, int32_t h, int32_t flags, int64_t *out_W, uint8_t **out_rows, uint8_t **out_pp_rows,
               uint8_t **out_pp_cons, uint8_t **out_rf, int32_t **out_matmap, int64_t *out_pathless, void *stream) {
  if (!e) { set_error("wh_msa_dev: null handle"); return WH_EINVAL; }
  if (h < 0 || h >= (int)e->hmms.size()) { set_error("wh_msa_dev: model position %d out of range (0..%d)", h, (int)e->hmms.size() - 1); return WH_EINVAL; }
  if (nq < 0 || total_residues < 0 || !out_W || !out_rows || !out_pp_rows || !out_pp_cons || !out_rf || !out_matmap || !out_pathless ||
      (nq > 0 && !d_offsets) || (total_residues > 0 && (!d_cols || !d_pp || !d_text)) || (flags & ~(WH_MSA_TRIM | WH_MSA_NO_LDS))) {
    set_error("wh_msa_dev: bad argument");
    return WH_EINVAL;
  }
  const int M = e->hmms[(size_t)h].M;
  e->timers[6].launches = 0; e->timers[6].ms = 0; e->timers[6].pending = false;
  MsaOut o;
  if (nq == 0) {                 // no sequences: the model's columns alone; no device work
    if (int rc = o.alloc(0, M, M, "wh_msa_dev")) return rc;
    for (int k = 0; k < M; k++) { o.rf[k] = 'x'; o.pp_cons[k] = '.'; o.matmap[k] = k; }
    *out_W = M; *out_pathless = 0;
    o.give(out_rows, out_pp_rows, out_pp_cons, out_rf, out_matmap);
    return WH_OK;
  }
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipSetDevice(e->device));
  // d_msa_lay: width [M + 1] | matmap [M] | cons_cnt [M] | pathless [1] (ints), then layout [M + 2] (8-byte aligned), cons_sum [M]
  const size_t n_int = (size_t)3 * M + 2, lay_at = (n_int * sizeof(int32_t) + 7) & ~(size_t)7;
  const size_t lay_bytes = lay_at + sizeof(long long) * ((size_t)M + 2) + sizeof(float) * (size_t)M;
  const size_t wmax = (size_t)M + (size_t)total_residues;          // no alignment is wider
  if (e->d_msa_lay.ensure(lay_bytes) || e->d_msa_res.ensure(2 * sizeof(int32_t) * (size_t)total_residues + 16) || e->d_msa_gc.ensure(2 * (wmax + 16)))
    return WH_ENOMEM;
  if (timer_begin(e, 6, s)) return WH_EHIP;
  HIPCHK(hipMemsetAsync(e->d_msa_lay.p, 0, lay_bytes, s));
  MsaArgs a;
  memset(&a, 0, sizeof a);
  a.cols = d_cols; a.pp = d_pp; a.text = d_text; a.off = d_offsets; a.nq = nq; a.total = total_residues; a.M = M; a.trim = (flags & WH_MSA_TRIM) ? 1 : 0;
  a.width = (int32_t *)e->d_msa_lay.p; a.matmap = a.width + (M + 1); a.cons_cnt = a.matmap + M; a.pathless = a.cons_cnt + M;
  a.layout = (long long *)((char *)e->d_msa_lay.p + lay_at); a.cons_sum = (float *)(a.layout + (M + 2));
  a.res_blk = (int32_t *)e->d_msa_res.p; a.res_k = a.res_blk + total_residues;
  a.rf = (uint8_t *)e->d_msa_gc.p; a.pp_cons = a.rf + ((wmax + 15) & ~(size_t)15);
  hipError_t err = launch_msa_widths(a, s);
  if (err == hipSuccess) err = launch_msa_layout(a, s);
  if (err != hipSuccess) { set_error("wh_msa_dev: width / layout kernels failed to launch: %s", hipGetErrorString(err)); return WH_EHIP; }
  // the one value the host needs before it can go on: W sizes the rows
  long long W = 0;
  HIPCHK(hipMemcpyAsync(&W, a.layout + (M + 1), sizeof W, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (W < M || (size_t)W > wmax) { set_error("wh_msa_dev: a width of %lld columns for %d nodes and %lld residues (offsets and total_residues disagree?)", W, M, (long long)total_residues); return WH_EINVAL; }
  const size_t nb = (size_t)nq * (size_t)W;
  const int64_t chunk = (int64_t)std::max<size_t>(1, std::min<size_t>((size_t)nq, kMsaChunkBytes / (sizeof(float) * (size_t)std::max(M, 1))));
  if (e->d_msa_rows.ensure(nb + 16) || e->d_msa_pprows.ensure(nb + 16) || e->d_msa_ppm.ensure(sizeof(float) * (size_t)chunk * (size_t)M + 16)) return WH_ENOMEM;
  a.rows = (uint8_t *)e->d_msa_rows.p; a.pp_rows = (uint8_t *)e->d_msa_pprows.p; a.ppm = (float *)e->d_msa_ppm.p;
  const bool lds = !(flags & WH_MSA_NO_LDS) && msa_render_lds_bytes(W) <= kMsaLdsBudget;
  int launches = 2;
  for (int64_t q0 = 0; q0 < nq; q0 += chunk) {
    a.q0 = q0; a.q1 = std::min(nq, q0 + chunk); a.last = a.q1 == nq ? 1 : 0;
    err = launch_msa_render(a, W, lds, s);
    if (err == hipSuccess) err = launch_msa_cons(a, s);
    if (err != hipSuccess) { set_error("wh_msa_dev: render / PP_cons kernels failed to launch: %s", hipGetErrorString(err)); return WH_EHIP; }
    launches += 2;
  }
  if (timer_end(e, 6, s, launches)) return WH_EHIP;
  if (int rc = o.alloc(nq, W, M, "wh_msa_dev")) return rc;
  int pathless = 0;
  HIPCHK(hipMemcpyAsync(o.rows, a.rows, nb, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(o.pp_rows, a.pp_rows, nb, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(o.pp_cons, a.pp_cons, (size_t)W, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(o.rf, a.rf, (size_t)W, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(o.matmap, a.matmap, sizeof(int32_t) * (size_t)M, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&pathless, a.pathless, sizeof pathless, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *out_W = W; *out_pathless = pathless;
  o.give(out_rows, out_pp_rows, out_pp_cons, out_rf, out_matmap);
  return WH_OK;
}

int wh_msa(wh_ehmm *e, const uint8_t *residues, const int64_t *offsets, const uint8_t *text, int64_t nq, int32_t h, int32_t flags,
           int64_t *out_W, uint8_t **out_rows, uint8_t **out_pp_rows, uint8_t **out_pp_cons, uint8_t **out_rf, int32_t **out_matmap,
           int64_t *out_pathless) {
  if (!e) { set_error("wh_msa: null handle"); return WH_EINVAL; }
  if (h < 0 || h >= (int)e->hmms.size()) { set_error("wh_msa: model position %d out of range (0..%d)", h, (int)e->hmms.size() - 1); return WH_EINVAL; }
  if (nq < 0 || (nq > 0 && (!offsets || !residues || !text)) || !out_W || !out_rows || !out_pp_rows || !out_pp_cons || !out_rf || !out_matmap || !out_pathless) {
    set_error("wh_msa: bad argument");
    return WH_EINVAL;
  }
  if (nq == 0) return wh_msa_dev(e, nullptr, nullptr, nullptr, nullptr, 0, 0, h, flags, out_W, out_rows, out_pp_rows, out_pp_cons, out_rf, out_matmap, out_pathless, nullptr);
  if (nq > 0x7FFFFFFF) { set_error("wh_msa: too many sequences"); return WH_ERANGE; }
  HIPCHK(hipSetDevice(e->device));
  const int64_t total = offsets[nq];
  if (total < 0 || offsets[0] != 0) { set_error("wh_msa: bad offsets"); return WH_EINVAL; }
  if (check_residues(e->Kp, residues, total)) return WH_EINVAL;
  // the pairs (q, h): one per sequence, so the columns and posteriors share the sequences' CSR
  std::vector<int64_t> pq((size_t)nq);
  std::vector<int32_t> ph((size_t)nq, h);
  for (int64_t q = 0; q < nq; q++) pq[(size_t)q] = q;
  Staging st(e);
  const uint8_t *d_res = st.in(residues, (size_t)total, 16);
  const int64_t *d_off = st.in(offsets, sizeof(int64_t) * (size_t)(nq + 1));
  const uint8_t *d_text = st.in(text, (size_t)total, 16);
  const int64_t *d_pq = st.in(pq.data(), sizeof(int64_t) * (size_t)nq);
  const int32_t *d_ph = st.in(ph.data(), sizeof(int32_t) * (size_t)nq);
  if (st.rc) return st.rc;
  if (e->d_msa_cols.ensure(sizeof(int32_t) * (size_t)total + 16) || e->d_msa_pp.ensure(sizeof(float) * (size_t)total + 16)) return WH_ENOMEM;
  HIPCHK(hipMemset(e->d_msa_cols.p, 0xFF, sizeof(int32_t) * (size_t)total + 16));     // (a residue the alignment leaves out: -1)
  HIPCHK(hipMemset(e->d_msa_pp.p, 0, sizeof(float) * (size_t)total + 16));
  if (int rc = wh_align_pp_dev(e, d_res, d_off, nq, total, max_query_len(offsets, nq), d_pq, d_ph, nq, d_off, (int32_t *)e->d_msa_cols.p,
                               (float *)e->d_msa_pp.p, nullptr))
    return rc;
  return wh_msa_dev(e, (const int32_t *)e->d_msa_cols.p, (const float *)e->d_msa_pp.p, d_text, d_off, nq, total, h, flags, out_W, out_rows,
                    out_pp_rows, out_pp_cons, out_rf, out_matmap, out_pathless, nullptr);
}

}  // extern "C"
