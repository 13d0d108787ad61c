// Host side of the multi-sequence alignment (include/witch_hip.h: wh_msa_dev, wh_msa): the kernels of wh_msa.hip behind
// one wh_align_pp_dev call for the pairs (q, h); and of hmmalign --mapali (wh_msa_mapali_dev, wh_msa_mapali): the kernels of
// wh_mapali.hip turn the rows of the model's own alignment into sequences without posteriors in front of the new ones.
#include "wh_host.h"

namespace {

// the buffers a call returns; what a failed call has allocated is released
struct MsaOut {
  uint8_t *rows = nullptr, *pp_rows = nullptr, *pp_cons = nullptr, *rf = nullptr;
  int32_t *matmap = nullptr;
  ~MsaOut() { free(rows); free(pp_rows); free(pp_cons); free(rf); free(matmap); }
  // <nq> rows, <npp> of them with a PP row
  int alloc(int64_t nq, int64_t npp, int64_t W, int M, const char *who) {
    const size_t nb = (size_t)nq * (size_t)W;
    rows = (uint8_t *)malloc(nb + 1); pp_rows = (uint8_t *)malloc((size_t)npp * (size_t)W + 1);
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

// The assembly of <nq> sequences (arguments checked by the caller, <who>): the first <n_nopp> of them - residues
// 0 .. pp_shift - 1 - without posteriors (d_pp holds those of the residues from pp_shift on), the rows of a --mapali alignment.
int msa_assemble(const char *who, wh_ehmm *e, const int32_t *d_cols, const float *d_pp, const uint8_t *d_text, const int64_t *d_offsets,
                 int64_t nq, int64_t n_nopp, int64_t pp_shift, int64_t total_residues, int32_t h, int32_t flags, int64_t *out_W,
                 uint8_t **out_rows, uint8_t **out_pp_rows, uint8_t **out_pp_cons, uint8_t **out_rf, int32_t **out_matmap,
                 int64_t *out_pathless, void *stream) {
  const int M = e->hmms[(size_t)h].M;
  e->timers[6].launches = 0; e->timers[6].ms = 0; e->timers[6].pending = false;
  MsaOut o;
  if (nq == 0) {                 // no sequences: the model's columns alone; no device work
    if (int rc = o.alloc(0, 0, M, M, who)) return rc;
    for (int k = 0; k < M; k++) { o.rf[k] = 'x'; o.pp_cons[k] = '.'; o.matmap[k] = k; }
    *out_W = M; *out_pathless = 0;
    o.give(out_rows, out_pp_rows, out_pp_cons, out_rf, out_matmap);
    return WH_OK;
  }
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipSetDevice(e->device));
  // d_msa_lay: width [M + 1] | matmap [M] | cons_cnt [M] | pathless [1] (ints), then layout [M + 2] (8-byte aligned), cons_sum [M]
  const size_t n_int = (size_t)3 * M + 2, lay_at = (n_int * sizeof(int32_t) + 7) & ~(size_t)7;
  const size_t sum64_at = (lay_at + sizeof(long long) * ((size_t)M + 2) + sizeof(float) * (size_t)M + 7) & ~(size_t)7;     // (WH_MSA_CONS_HMMER)
  const size_t lay_bytes = (flags & WH_MSA_CONS_HMMER) ? sum64_at + sizeof(double) * (size_t)M : lay_at + sizeof(long long) * ((size_t)M + 2) + sizeof(float) * (size_t)M;
  const size_t wmax = (size_t)M + (size_t)total_residues;          // no alignment is wider
  if (e->d_msa_lay.ensure(lay_bytes) || e->d_msa_res.ensure(2 * sizeof(int32_t) * (size_t)total_residues + 16) || e->d_msa_gc.ensure(2 * (wmax + 16)))
    return WH_ENOMEM;
  if (timer_begin(e, 6, s)) return WH_EHIP;
  HIPCHK(hipMemsetAsync(e->d_msa_lay.p, 0, lay_bytes, s));
  MsaArgs a;
  memset(&a, 0, sizeof a);
  a.cols = d_cols; a.pp = d_pp; a.text = d_text; a.off = d_offsets; a.nq = nq; a.total = total_residues; a.n_nopp = n_nopp; a.pp_shift = pp_shift; a.M = M; a.trim = (flags & WH_MSA_TRIM) ? 1 : 0;
  a.width = (int32_t *)e->d_msa_lay.p; a.matmap = a.width + (M + 1); a.cons_cnt = a.matmap + M; a.pathless = a.cons_cnt + M;
  a.layout = (long long *)((char *)e->d_msa_lay.p + lay_at); a.cons_sum = (float *)(a.layout + (M + 2));
  if (flags & WH_MSA_CONS_HMMER) a.cons_sum64 = (double *)((char *)e->d_msa_lay.p + sum64_at);
  a.res_blk = (int32_t *)e->d_msa_res.p; a.res_k = a.res_blk + total_residues;
  a.rf = (uint8_t *)e->d_msa_gc.p; a.pp_cons = a.rf + ((wmax + 15) & ~(size_t)15);
  hipError_t err = launch_msa_widths(a, s);
  if (err == hipSuccess) err = launch_msa_layout(a, s);
  if (err != hipSuccess) { set_error("%s: width / layout kernels failed to launch: %s", who, hipGetErrorString(err)); return WH_EHIP; }
  // the one value the host needs before it can go on: W sizes the rows
  long long W = 0;
  HIPCHK(hipMemcpyAsync(&W, a.layout + (M + 1), sizeof W, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (W < M || (size_t)W > wmax) { set_error("%s: a width of %lld columns for %d nodes and %lld residues (offsets and total_residues disagree?)", who, W, M, (long long)total_residues); return WH_EINVAL; }
  const size_t nb = (size_t)nq * (size_t)W, nbpp = (size_t)(nq - n_nopp) * (size_t)W;
  const int64_t chunk = (int64_t)std::max<size_t>(1, std::min<size_t>((size_t)std::max<int64_t>(nq - n_nopp, 1), kMsaChunkBytes / (sizeof(float) * (size_t)std::max(M, 1))));
  if (e->d_msa_rows.ensure(nb + 16) || e->d_msa_pprows.ensure(nbpp + 16) || e->d_msa_ppm.ensure(sizeof(float) * (size_t)chunk * (size_t)M + 16)) return WH_ENOMEM;
  a.rows = (uint8_t *)e->d_msa_rows.p; a.pp_rows = (uint8_t *)e->d_msa_pprows.p; a.ppm = (float *)e->d_msa_ppm.p;
  const bool lds = !(flags & WH_MSA_NO_LDS) && msa_render_lds_bytes(W) <= kMsaLdsBudget;
  int launches = 2;
  if (n_nopp > 0) {              // the rows without posteriors: the sequence rows alone, no part in PP_cons
    a.q0 = 0; a.q1 = n_nopp; a.last = 0;
    err = launch_msa_render(a, W, lds, s);
    if (err != hipSuccess) { set_error("%s: render kernel failed to launch: %s", who, hipGetErrorString(err)); return WH_EHIP; }
    launches++;
  }
  for (int64_t q0 = n_nopp; q0 < nq; q0 += chunk) {
    a.q0 = q0; a.q1 = std::min(nq, q0 + chunk); a.last = a.q1 == nq ? 1 : 0;
    err = launch_msa_render(a, W, lds, s);
    if (err == hipSuccess) err = launch_msa_cons(a, s);
    if (err != hipSuccess) { set_error("%s: render / PP_cons kernels failed to launch: %s", who, hipGetErrorString(err)); return WH_EHIP; }
    launches += 2;
  }
  if (timer_end(e, 6, s, launches)) return WH_EHIP;
  if (int rc = o.alloc(nq, nq - n_nopp, W, M, who)) return rc;
  int pathless = 0;
  HIPCHK(hipMemcpyAsync(o.rows, a.rows, nb, hipMemcpyDeviceToHost, s));
  if (nbpp) HIPCHK(hipMemcpyAsync(o.pp_rows, a.pp_rows, nbpp, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(o.pp_cons, a.pp_cons, (size_t)W, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(o.rf, a.rf, (size_t)W, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(o.matmap, a.matmap, sizeof(int32_t) * (size_t)M, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&pathless, a.pathless, sizeof pathless, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *out_W = W; *out_pathless = pathless;
  o.give(out_rows, out_pp_rows, out_pp_cons, out_rf, out_matmap);
  return WH_OK;
}

// colcode[alen] of model <m> (wh_mapali.hip), or the reason why the model cannot take a --mapali alignment of alen columns
int mapali_colcode(const char *who, const HostHMM &m, int64_t alen, std::vector<int32_t> &code) {
  if (!m.has_map || !m.has_cksum) { set_error("%s: model %s has no %s line (--mapali needs the model's MAP annotation and the checksum of its alignment)", who, m.name.c_str(), m.has_map ? "CKSUM" : "MAP yes"); return WH_EINVAL; }
  for (int k = 1; k <= m.M; k++)
    if (m.map[(size_t)k] <= m.map[(size_t)k - 1]) { set_error("%s: model %s: the MAP column of node %d is %d, not beyond node %d's", who, m.name.c_str(), k, m.map[(size_t)k], k - 1); return WH_EINVAL; }
  if (alen < m.map[(size_t)m.M]) { set_error("%s: an alignment of %lld columns does not reach the model's last MAP column %d", who, (long long)alen, m.map[(size_t)m.M]); return WH_EINVAL; }
  code.resize((size_t)alen);
  int k = 0;                                             // nodes whose column lies at or before the current one
  for (int64_t c = 0; c < alen; c++) {
    if (k < m.M && m.map[(size_t)k + 1] == c + 1) code[(size_t)c] = k++;
    else code[(size_t)c] = -(k + 2);
  }
  return WH_OK;
}

const char *molecule_of(int alphabet) { return alphabet == WH_ALPH_AMINO ? "amino" : alphabet == WH_ALPH_RNA ? "rna" : "dna"; }

}  // namespace

extern "C" {

int wh_msa_dev(wh_ehmm *e, const int32_t *d_cols, const float *d_pp, const uint8_t *d_text, const int64_t *d_offsets, int64_t nq,
               int64_t total_residues, int32_t h, int32_t flags, int64_t *out_W, uint8_t **out_rows, uint8_t **out_pp_rows,
               uint8_t **out_pp_cons, uint8_t **out_rf, int32_t **out_matmap, int64_t *out_pathless, void *stream) {
  if (!e) { set_error("wh_msa_dev: null handle"); return WH_EINVAL; }
  if (h < 0 || h >= (int)e->hmms.size()) { set_error("wh_msa_dev: model position %d out of range (0..%d)", h, (int)e->hmms.size() - 1); return WH_EINVAL; }
  if (nq < 0 || total_residues < 0 || !out_W || !out_rows || !out_pp_rows || !out_pp_cons || !out_rf || !out_matmap || !out_pathless ||
      (nq > 0 && !d_offsets) || (total_residues > 0 && (!d_cols || !d_pp || !d_text)) || (flags & ~(WH_MSA_TRIM | WH_MSA_NO_LDS | WH_MSA_CONS_HMMER))) {
    set_error("wh_msa_dev: bad argument");
    return WH_EINVAL;
  }
  return msa_assemble("wh_msa_dev", e, d_cols, d_pp, d_text, d_offsets, nq, 0, 0, total_residues, h, flags, out_W, out_rows, out_pp_rows,
                      out_pp_cons, out_rf, out_matmap, out_pathless, stream);
}

int wh_msa_mapali_dev(wh_ehmm *e, const int32_t *d_cols, const float *d_pp, const uint8_t *d_text, const int64_t *d_offsets, int64_t nq,
                      int64_t total_residues, int32_t h, int32_t flags, const uint8_t *d_map_rows, int64_t n_map, int64_t alen,
                      int64_t *out_W, uint8_t **out_rows, uint8_t **out_pp_rows, uint8_t **out_pp_cons, uint8_t **out_rf,
                      int32_t **out_matmap, int64_t *out_pathless, void *stream) {
  const char *who = "wh_msa_mapali_dev";
  if (!e) { set_error("%s: null handle", who); return WH_EINVAL; }
  if (h < 0 || h >= (int)e->hmms.size()) { set_error("%s: model position %d out of range (0..%d)", who, h, (int)e->hmms.size() - 1); return WH_EINVAL; }
  if (nq < 0 || total_residues < 0 || n_map < 0 || !out_W || !out_rows || !out_pp_rows || !out_pp_cons || !out_rf || !out_matmap || !out_pathless ||
      (nq > 0 && !d_offsets) || (total_residues > 0 && (!d_cols || !d_pp || !d_text)) || (flags & ~(WH_MSA_TRIM | WH_MSA_NO_LDS)) ||
      (n_map > 0 && (!d_map_rows || alen < 1))) {
    set_error("%s: bad argument", who);
    return WH_EINVAL;
  }
  e->timers[7].launches = 0; e->timers[7].ms = 0; e->timers[7].pending = false;
  if (n_map == 0)
    return wh_msa_dev(e, d_cols, d_pp, d_text, d_offsets, nq, total_residues, h, flags, out_W, out_rows, out_pp_rows, out_pp_cons, out_rf,
                      out_matmap, out_pathless, stream);
  if (n_map + nq > 0x7FFFFFFF || n_map > (int64_t)0x7FFFFFFFFFFF / alen) { set_error("%s: too many rows", who); return WH_ERANGE; }
  std::vector<int32_t> code;
  if (int rc = mapali_colcode(who, e->hmms[(size_t)h], alen, code)) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipSetDevice(e->device));
  if (e->d_map_code.ensure(sizeof(int32_t) * (size_t)alen) || e->d_map_cnt.ensure(sizeof(int32_t) * (size_t)n_map) ||
      e->d_map_off.ensure(sizeof(int64_t) * ((size_t)n_map + 1)) || e->d_map_alloff.ensure(sizeof(int64_t) * ((size_t)(n_map + nq) + 1)))
    return WH_ENOMEM;
  MapaliArgs m;
  memset(&m, 0, sizeof m);
  m.rows = d_map_rows; m.n_map = n_map; m.alen = alen; m.colcode = (const int32_t *)e->d_map_code.p; m.count = (int32_t *)e->d_map_cnt.p;
  m.off = (const int64_t *)e->d_map_off.p; m.seq_off = d_offsets; m.nq = nq; m.all_off = (int64_t *)e->d_map_alloff.p;
  if (timer_begin(e, 7, s)) return WH_EHIP;
  HIPCHK(hipMemcpyAsync(e->d_map_code.p, code.data(), sizeof(int32_t) * (size_t)alen, hipMemcpyHostToDevice, s));
  hipError_t err = launch_mapali_count(m, s);
  if (err != hipSuccess) { set_error("%s: count kernel failed to launch: %s", who, hipGetErrorString(err)); return WH_EHIP; }
  // the residue counts come back once; the host forms the rows' CSR (wh_domains_dev's precedent)
  std::vector<int32_t> cnt((size_t)n_map);
  std::vector<int64_t> off((size_t)n_map + 1, 0);
  HIPCHK(hipMemcpyAsync(cnt.data(), m.count, sizeof(int32_t) * (size_t)n_map, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  for (int64_t i = 0; i < n_map; i++) {
    if (cnt[(size_t)i] < 0 || cnt[(size_t)i] > alen) { set_error("%s: row %lld counts %d residues in %lld columns", who, (long long)i, cnt[(size_t)i], (long long)alen); return WH_EHIP; }
    off[(size_t)i + 1] = off[(size_t)i] + cnt[(size_t)i];
  }
  const int64_t total_map = off[(size_t)n_map], total = total_map + total_residues;
  if (e->d_map_cols.ensure(sizeof(int32_t) * (size_t)total + 16) || e->d_map_text.ensure((size_t)total + 16)) return WH_ENOMEM;
  m.text = (uint8_t *)e->d_map_text.p; m.cols = (int32_t *)e->d_map_cols.p; m.shift = total_map;
  HIPCHK(hipMemcpyAsync(e->d_map_off.p, off.data(), sizeof(int64_t) * ((size_t)n_map + 1), hipMemcpyHostToDevice, s));
  err = launch_mapali_map(m, s);
  if (err != hipSuccess) { set_error("%s: map kernel failed to launch: %s", who, hipGetErrorString(err)); return WH_EHIP; }
  if (total_residues > 0) {      // the new sequences behind the rows' residues
    HIPCHK(hipMemcpyAsync(m.cols + total_map, d_cols, sizeof(int32_t) * (size_t)total_residues, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(m.text + total_map, d_text, (size_t)total_residues, hipMemcpyDeviceToDevice, s));
  }
  if (timer_end(e, 7, s, 2)) return WH_EHIP;
  HIPCHK(hipStreamSynchronize(s));          // (off, code: the uploads have left the host vectors)
  return msa_assemble(who, e, m.cols, d_pp, m.text, m.all_off, n_map + nq, n_map, total_map, total, h, flags, out_W, out_rows, out_pp_rows,
                      out_pp_cons, out_rf, out_matmap, out_pathless, stream);
}

int wh_msa_mapali(wh_ehmm *e, const uint8_t *residues, const int64_t *offsets, const uint8_t *text, int64_t nq, int32_t h, int32_t flags,
                  const uint8_t *map_rows, int64_t n_map, int64_t alen, int64_t *out_W, uint8_t **out_rows, uint8_t **out_pp_rows,
                  uint8_t **out_pp_cons, uint8_t **out_rf, int32_t **out_matmap, int64_t *out_pathless) {
  const char *who = "wh_msa_mapali";
  if (!e) { set_error("%s: null handle", who); return WH_EINVAL; }
  if (h < 0 || h >= (int)e->hmms.size()) { set_error("%s: model position %d out of range (0..%d)", who, h, (int)e->hmms.size() - 1); return WH_EINVAL; }
  if (nq < 0 || n_map < 0 || (nq > 0 && (!offsets || !residues || !text)) || (n_map > 0 && (!map_rows || alen < 1)) || !out_W || !out_rows ||
      !out_pp_rows || !out_pp_cons || !out_rf || !out_matmap || !out_pathless || (flags & ~(WH_MSA_TRIM | WH_MSA_NO_LDS))) {
    set_error("%s: bad argument", who);
    return WH_EINVAL;
  }
  if (n_map == 0) return wh_msa(e, residues, offsets, text, nq, h, flags, out_W, out_rows, out_pp_rows, out_pp_cons, out_rf, out_matmap, out_pathless);
  if (n_map + nq > 0x7FFFFFFF || n_map > (int64_t)0x7FFFFFFF) { set_error("%s: too many rows", who); return WH_ERANGE; }
  const HostHMM &m = e->hmms[(size_t)h];
  std::vector<int32_t> code;
  if (int rc = mapali_colcode(who, m, alen, code)) return rc;
  uint32_t cksum = 0;
  if (wh_alignment_checksum(molecule_of(e->alphabet), (const char *)map_rows, (int32_t)n_map, alen, &cksum)) {
    const std::string why = wh_last_error();
    set_error("%s: %s", who, why.c_str());
    return WH_EINVAL;
  }
  if (cksum != m.cksum) { set_error("%s: the alignment's checksum %u is not the model's CKSUM %u (checksum mismatch): not the alignment %s came from", who, cksum, m.cksum, m.name.c_str()); return WH_EINVAL; }
  HIPCHK(hipSetDevice(e->device));
  const int64_t total = nq > 0 ? offsets[nq] : 0;
  if (total < 0 || (nq > 0 && offsets[0] != 0)) { set_error("%s: bad offsets", who); return WH_EINVAL; }
  if (check_residues(e->Kp, residues, total)) return WH_EINVAL;
  const size_t map_bytes = (size_t)n_map * (size_t)alen;
  if (e->d_map_rows.ensure(map_bytes + 16)) return WH_ENOMEM;
  HIPCHK(hipMemcpy(e->d_map_rows.p, map_rows, map_bytes, hipMemcpyHostToDevice));
  const uint8_t *d_rows = (const uint8_t *)e->d_map_rows.p;
  if (nq == 0)
    return wh_msa_mapali_dev(e, nullptr, nullptr, nullptr, nullptr, 0, 0, h, flags, d_rows, n_map, alen, out_W, out_rows, out_pp_rows,
                             out_pp_cons, out_rf, out_matmap, out_pathless, nullptr);
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
  return wh_msa_mapali_dev(e, (const int32_t *)e->d_msa_cols.p, (const float *)e->d_msa_pp.p, d_text, d_off, nq, total, h, flags, d_rows, n_map,
                           alen, out_W, out_rows, out_pp_rows, out_pp_cons, out_rf, out_matmap, out_pathless, nullptr);
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
