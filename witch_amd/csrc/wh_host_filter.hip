// Host side of hmmsearch's acceleration filters (wh_filter.h: the pipeline; wh_filter.hip: the kernels): wh_filter_dev /
// wh_filter, the device-free wh_filter_host, and wh_score_filtered_dev / wh_score_filtered - filters, then the EXISTING
// scoring path on the queries with a surviving pair, then the Forward stage and the scatter back.
#include <memory>

#include "wh_host.h"
#include "wh_filter.h"

using namespace whf;

// what the handle keeps for the filters: made by the first call that filters
struct FilterState {
  std::vector<FilterModel> models;
  std::vector<FilterDevModel> desc;          // host copy; the thresholds are the call's
  std::vector<FilterLen> lens;               // [0 .. lens.size())
  std::vector<int> lists[kFilterClasses];    // models by register class
  std::vector<int> big;                      // models beyond the classes
  size_t list_off[kFilterClasses] = {0, 0, 0, 0, 0, 0};
  DevBuf d_tables, d_desc, d_lens, d_list, d_ws, d_counts;
  size_t lens_on_device = 0;
  // the bias filter: per model (uploaded with the tables), per length (uploaded by the first call that runs the stage)
  std::vector<FilterBias> bias;
  std::vector<FilterBiasLen> blens;
  DevBuf d_biasm, d_blens;
  size_t blens_on_device = 0;
  int64_t handed = 0;                        // wh_score_filtered: pairs handed to the scoring kernels
  bool scored = false;                       // the last filtering call was wh_score_filtered
  // wh_score_filtered: stage / bias of the call, the kept queries, the compacted batch and its results
  DevBuf d_stage, d_bias, d_keep, d_qmap, d_qlist, d_coff, d_cres, d_cdeci, d_cflags, d_cfwd, d_cdet, d_x3;
  std::vector<uint8_t> h_keep;
  std::vector<int64_t> h_off, h_coff, h_qlist, h_qmap;
  std::vector<float> h_x3;
};

void wh_ehmm::FilterStateDelete::operator()(FilterState *f) const { delete f; }

namespace {

size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

int options_of(const wh_filter_opts *o, FilterOpts &fo, const char *what) {
  if (o) { fo.F1 = o->F1; fo.F2 = o->F2; fo.F3 = o->F3; fo.nobias = o->nobias; }
  if (!fo.nobias) {
    set_error("%s: the bias filter is not implemented; filtered search needs nobias = 1 (hmmsearch --nobias)", what);
    return WH_EINVAL;
  }
  if (fo.nobias != 1 && fo.nobias != WH_BIAS_FILTER_ON) {
    set_error("%s: nobias = %d is neither 1 (hmmsearch --nobias) nor WH_BIAS_FILTER_ON", what, fo.nobias);
    return WH_EINVAL;
  }
  if (!(fo.F1 == fo.F1) || !(fo.F2 == fo.F2) || !(fo.F3 == fo.F3)) { set_error("%s: a threshold is not a number", what); return WH_EINVAL; }
  return WH_OK;
}

// a parsed model -> its filter tables; WH_EINVAL (naming the model) without the three STATS LOCAL lines
int model_of(const HostHMM &h, const uint32_t *degen, FilterModel &fm) {
  const char *missing = filter_model_of(h, degen, fm);
  if (!missing) return WH_OK;
  set_error("model %s (%s) has no STATS LOCAL %s line: a model without E-value statistics cannot be filtered (hmmbuild writes them, as does "
            "wh_hmmbuild2 with WH_BUILD_STATS)", h.name.c_str(), h.path.c_str(), missing);
  return WH_EINVAL;
}

// the handle's filter state: tables of every model on the device, the class lists
int state_of(wh_ehmm *e, FilterState **out) {
  if (e->filter) { *out = e->filter.get(); return WH_OK; }
  std::unique_ptr<FilterState> f(new FilterState);
  const int H = (int)e->hmms.size();
  f->models.resize((size_t)H);
  f->desc.resize((size_t)H);
  f->bias.resize((size_t)H);
  std::vector<unsigned char> tab;
  for (int h = 0; h < H; h++) {
    FilterModel &fm = f->models[(size_t)h];
    const int rc = model_of(e->hmms[(size_t)h], e->degen, fm);
    if (rc) return rc;
    f->bias[(size_t)h] = fm.bias;
    FilterDevModel &d = f->desc[(size_t)h];
    memset(&d, 0, sizeof d);
    const int M = fm.M, Kp = fm.Kp, cls = filter_class(M);
    const size_t W = (size_t)M + 1;
    d.M = M; d.Kp = Kp;
    d.base_b = fm.msv.base; d.bias_b = fm.msv.bias; d.tbm = fm.msv.tbm; d.tec = fm.msv.tec;
    d.base_w = fm.vit.base; d.xE_loop = fm.vit.xE_loop; d.xE_move = fm.vit.xE_move;
    d.scale_b = fm.msv.scale; d.scale_w = fm.vit.scale;
    if (cls >= 0) {
      const int Q = kFilterQ[cls], Mpad = 64 * Q;
      d.rb = tab.size(); tab.resize(tab.size() + up16((size_t)Kp * Mpad), 255);
      for (int x = 0; x < Kp; x++) memcpy(&tab[d.rb + (size_t)x * Mpad], &fm.msv.rb[(size_t)x * W + 1], (size_t)M);
      d.rw = tab.size(); tab.resize(tab.size() + up16((size_t)2 * Kp * Mpad));
      d.tw = tab.size(); tab.resize(tab.size() + up16((size_t)2 * 8 * Mpad));
      int16_t *rw = reinterpret_cast<int16_t *>(&tab[d.rw]), *tw = reinterpret_cast<int16_t *>(&tab[d.tw]);
      for (size_t i = 0; i < (size_t)Kp * Mpad; i++) rw[i] = -32768;
      for (size_t i = 0; i < (size_t)8 * Mpad; i++) tw[i] = -32768;
      for (int x = 0; x < Kp; x++) memcpy(&rw[(size_t)x * Mpad], &fm.vit.rw[(size_t)x * W + 1], (size_t)M * 2);
      for (int k = 1; k <= M; k++)
        for (int z = 0; z < 8; z++) tw[(size_t)z * Mpad + (size_t)(k - 1)] = fm.vit.tw[(size_t)k * 8 + z];
      f->lists[cls].push_back(h);
    } else {
      d.rb = tab.size(); tab.resize(tab.size() + up16((size_t)Kp * W));
      memcpy(&tab[d.rb], fm.msv.rb.data(), (size_t)Kp * W);
      d.rw = tab.size(); tab.resize(tab.size() + up16((size_t)2 * Kp * W));
      memcpy(&tab[d.rw], fm.vit.rw.data(), (size_t)2 * Kp * W);
      d.tw = tab.size(); tab.resize(tab.size() + up16((size_t)16 * W));
      memcpy(&tab[d.tw], fm.vit.tw.data(), (size_t)16 * W);
      f->big.push_back(h);
    }
  }
  std::vector<int> all;
  for (int c = 0; c < kFilterClasses; c++) { f->list_off[c] = all.size(); all.insert(all.end(), f->lists[c].begin(), f->lists[c].end()); }
  if (f->d_tables.ensure(tab.size() + 16) || f->d_desc.ensure(sizeof(FilterDevModel) * (size_t)H) || f->d_list.ensure(sizeof(int) * (all.size() + 1)) ||
      f->d_counts.ensure(8 * sizeof(unsigned long long)) || f->d_biasm.ensure(sizeof(FilterBias) * (size_t)H))
    return WH_ENOMEM;
  if (hipMemcpy(f->d_tables.p, tab.data(), tab.size(), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(f->d_biasm.p, f->bias.data(), sizeof(FilterBias) * (size_t)H, hipMemcpyHostToDevice) != hipSuccess ||
      (all.size() && hipMemcpy(f->d_list.p, all.data(), sizeof(int) * all.size(), hipMemcpyHostToDevice) != hipSuccess)) {
    set_error("wh_filter: uploading the filter tables failed");
    return WH_EHIP;
  }
  e->filter.reset(f.release());
  *out = e->filter.get();
  return WH_OK;
}

// ---- wh_score_filtered's own kernels ---------------------------------------------------------------------------------
// keep[q] = 1 where a pair of query q is past the Viterbi stage
__global__ void keep_kernel(const uint8_t *stage, long long nq, int H, uint8_t *keep) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  unsigned any = 0;
  for (int h = 0; h < H; h++) any |= stage[q * H + h] & (unsigned)kStageVit;
  keep[q] = any ? 1 : 0;
}
// the residues of kept query kq (block kq) into the compacted batch
__global__ void gather_kernel(const uint8_t *res, const long long *off, const long long *qlist, const long long *coff, uint8_t *cres) {
  const long long q = qlist[blockIdx.x];
  const long long s = off[q], n = off[q + 1] - s, d = coff[blockIdx.x];
  for (long long i = threadIdx.x; i < n; i += blockDim.x) cres[d + i] = res[s + i];
}
struct ScatterArgs {
  long long nq; int H;
  const long long *qmap;             // [nq]: position in the compacted batch, -1: not scored
  const float *x3;                   // [H] Forward-stage thresholds
  const float *bias;
  uint8_t *stage;
  const int32_t *cdeci; const uint8_t *cflags; const float *cfwd; const wh_pair_detail *cdet;
  int32_t *deci; uint8_t *flags; float *fwd; wh_pair_detail *det;
  unsigned long long *counts;        // [4] += pairs past the Forward stage
};
__global__ void scatter_kernel(ScatterArgs a) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned pass = 0;
  if (p < a.nq * a.H) {
    const long long q = p / a.H;
    const int h = (int)(p % a.H);
    const long long kq = a.qmap[q];
    const long long src = kq * a.H + h;
    unsigned st = a.stage[p];
    const float fwdv = kq >= 0 ? a.cfwd[src] : 0.f;
    if (kq >= 0 && (st & kStageVit)) {
      FilterThr t; t.x1 = t.x2m = t.x2v = 0.f; t.x3 = a.x3[h];
      // (a pair without a Forward result - fwd_bits not finite - is not reported by the scoring path either)
      if (filter_stage4(fwdv, a.bias[p], t)) pass = 1;
    }
    if (pass) {
      a.stage[p] = (uint8_t)(st | kStageFwd);
      a.deci[p] = a.cdeci[src];
      a.flags[p] = a.cflags[src];
      if (a.det) a.det[p] = a.cdet[src];
    } else {
      a.deci[p] = 0;
      a.flags[p] = WH_FLAG_FILTERED;
      if (a.det) { wh_pair_detail z; memset(&z, 0, sizeof z); z.fwd_bits = fwdv; a.det[p] = z; }
    }
    if (a.fwd) a.fwd[p] = fwdv;
  }
  const unsigned long long m = __ballot(pass);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&a.counts[4], (unsigned long long)__builtin_popcountll(m));
}

// the filters of one call; counts [0..3] are left on the device
int run_filters(wh_ehmm *e, FilterState *f, const FilterOpts &fo, const uint8_t *d_res, const int64_t *d_off, int64_t nq, int32_t max_len, uint8_t *d_stage,
                float *d_bias, int32_t *d_msv, int32_t *d_vit, hipStream_t s) {
  const int H = (int)e->hmms.size();
  if ((double)nq * (double)H >= 2147483648.0) { set_error("wh_filter: %lld queries x %d models is 2^31 pairs or more: feed the queries in chunks", (long long)nq, H); return WH_ERANGE; }
  // per-length settings up to the call's longest query
  if ((size_t)max_len + 1 > f->lens.size()) {
    const size_t old = f->lens.size();
    f->lens.resize((size_t)max_len + 1);
    for (size_t L = old; L < f->lens.size(); L++) f->lens[L] = filter_len((int)L);
  }
  if (f->lens_on_device < f->lens.size()) {
    HIPCHK(hipStreamSynchronize(s));       // (an earlier call may still read the table that ensure() would free)
    if (f->d_lens.ensure(sizeof(FilterLen) * f->lens.size())) return WH_ENOMEM;
    HIPCHK(hipMemcpy(f->d_lens.p, f->lens.data(), sizeof(FilterLen) * f->lens.size(), hipMemcpyHostToDevice));
    f->lens_on_device = f->lens.size();
  }
  // the bias filter's per-length records, to the same length as the others: only for a call that runs the stage
  const bool bias = fo.bias();
  if (bias && f->blens_on_device < f->lens_on_device) {
    const size_t old = f->blens.size();
    f->blens.resize(f->lens_on_device);
    for (size_t L = old; L < f->blens.size(); L++) f->blens[L] = filter_bias_len((int)std::max<size_t>(L, 1));
    HIPCHK(hipStreamSynchronize(s));
    if (f->d_blens.ensure(sizeof(FilterBiasLen) * f->blens.size())) return WH_ENOMEM;
    HIPCHK(hipMemcpy(f->d_blens.p, f->blens.data(), sizeof(FilterBiasLen) * f->blens.size(), hipMemcpyHostToDevice));
    f->blens_on_device = f->blens.size();
  }
  for (int h = 0; h < H; h++) f->desc[(size_t)h].thr = filter_thresholds(f->models[(size_t)h].evp, fo);
  HIPCHK(hipMemcpyAsync(f->d_desc.p, f->desc.data(), sizeof(FilterDevModel) * (size_t)H, hipMemcpyHostToDevice, s));
  FilterBiasArgs a;
  memset(&a, 0, sizeof a);
  a.models = (const FilterDevModel *)f->d_desc.p;
  a.tables = (const unsigned char *)f->d_tables.p;
  a.lens = (const FilterLen *)f->d_lens.p;
  a.lmax = (int)f->lens_on_device - 1;
  a.residues = d_res; a.offsets = (const long long *)d_off; a.nq = nq; a.H = H;
  a.stage = d_stage; a.bias_nats = d_bias; a.msv_raw = d_msv; a.vit_raw = d_vit;
  a.bias = (const FilterBias *)f->d_biasm.p; a.blens = (const FilterBiasLen *)f->d_blens.p;
  for (int c = 0; c < kFilterClasses; c++) {
    if (f->lists[c].empty()) continue;
    a.list = (const int *)f->d_list.p + f->list_off[c];
    const long long np = (long long)nq * (long long)f->lists[c].size();
    if (bias ? launch_filter_class_bias(c, a, np, s) : launch_filter_class(c, a, np, s)) { set_error("wh_filter: launching the filter kernel failed: %s", hipGetErrorString(hipGetLastError())); return WH_EHIP; }
  }
  // models beyond the register classes: one lane per pair, rows in HBM, in chunks of queries that fit the row budget
  for (int h : f->big) {
    const size_t per_lane = (size_t)14 * ((size_t)f->models[(size_t)h].M + 1);
    size_t budget = (size_t)256 << 20;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget = std::min(budget, (free_b + f->d_ws.cap) / 2);
    int64_t lanes = std::min<int64_t>(nq, std::max<int64_t>(1, (int64_t)(budget / per_lane)));
    if (f->d_ws.ensure((size_t)lanes * per_lane + 16)) return WH_ENOMEM;
    for (int64_t q0 = 0; q0 < nq; q0 += lanes) {
      a.ws = (unsigned char *)f->d_ws.p; a.q0 = q0; a.q1 = std::min(nq, q0 + lanes); a.h = h;
      if (bias ? launch_filter_hbm_bias(a, s) : launch_filter_hbm(a, s)) { set_error("wh_filter: launching the long-model filter kernel failed: %s", hipGetErrorString(hipGetLastError())); return WH_EHIP; }
    }
  }
  HIPCHK(hipMemsetAsync(f->d_counts.p, 0, 8 * sizeof(unsigned long long), s));
  if (launch_filter_count(d_stage, (long long)nq * H, (unsigned long long *)f->d_counts.p, s)) { set_error("wh_filter: launching the count kernel failed"); return WH_EHIP; }
  f->handed = 0; f->scored = false;
  return WH_OK;
}

}  // namespace

extern "C" {

int wh_filter_dev(wh_ehmm *e, const uint8_t *d_residues, const int64_t *d_offsets, int64_t nq, int64_t total_residues, int32_t max_len,
                  const wh_filter_opts *opts, uint8_t *d_stage, float *d_filter_bias_nats, int32_t *d_msv_raw, int32_t *d_vit_raw, void *stream) {
  (void)total_residues;
  if (!e || !d_residues || !d_offsets || !d_stage || nq < 0 || max_len < 0) { set_error("wh_filter_dev: bad argument"); return WH_EINVAL; }
  FilterOpts fo;
  int rc = options_of(opts, fo, "wh_filter");
  if (rc) return rc;
  HIPCHK(hipSetDevice(e->device));
  FilterState *f = nullptr;
  if ((rc = state_of(e, &f))) return rc;
  if (nq == 0) return WH_OK;
  return run_filters(e, f, fo, d_residues, d_offsets, nq, max_len, d_stage, d_filter_bias_nats, d_msv_raw, d_vit_raw, (hipStream_t)stream);
}

int wh_filter(wh_ehmm *e, const uint8_t *residues, const int64_t *offsets, int64_t nq, const wh_filter_opts *opts, uint8_t *stage,
              float *filter_bias_nats, int32_t *msv_raw, int32_t *vit_raw) {
  if (!e || !residues || !offsets || !stage || nq < 0) { set_error("wh_filter: bad argument"); return WH_EINVAL; }
  FilterOpts fo;
  int rc = options_of(opts, fo, "wh_filter");
  if (rc) return rc;
  HIPCHK(hipSetDevice(e->device));
  FilterState *f = nullptr;
  if ((rc = state_of(e, &f))) return rc;
  if (nq == 0) return WH_OK;
  const int64_t total = offsets[nq];
  if (check_residues(e->Kp, residues, total)) return WH_EINVAL;
  const size_t np = (size_t)nq * e->hmms.size();
  Staging st(e);
  const uint8_t *d_res = st.in(residues, (size_t)total, 16);
  const int64_t *d_off = st.in(offsets, sizeof(int64_t) * (size_t)(nq + 1));
  uint8_t *d_stage = st.out(stage, np);
  float *d_bias = st.out(filter_bias_nats, 4 * np);
  int32_t *d_msv = st.out(msv_raw, 4 * np);
  int32_t *d_vit = st.out(vit_raw, 4 * np);
  if (st.rc) return st.rc;
  return st.finish(run_filters(e, f, fo, d_res, d_off, nq, max_query_len(offsets, nq), d_stage, d_bias, d_msv, d_vit, nullptr));
}

int wh_filter_host(const char *const *hmm_paths, int n, const uint8_t *residues, const int64_t *offsets, int64_t nq, const wh_filter_opts *opts,
                   uint8_t *stage, float *filter_bias_nats, int32_t *msv_raw, int32_t *vit_raw, int64_t *counts4) {
  if (!hmm_paths || n <= 0 || !residues || !offsets || !stage || nq < 0) { set_error("wh_filter_host: bad argument"); return WH_EINVAL; }
  FilterOpts fo;
  int rc = options_of(opts, fo, "wh_filter_host");
  if (rc) return rc;
  std::vector<FilterModel> models((size_t)n);
  std::vector<FilterThr> thr((size_t)n);
  int Kp = 0, maxM = 0;
  for (int h = 0; h < n; h++) {
    HostHMM hm;
    if ((rc = parse_hmm_file(hmm_paths[h], hm))) return rc;
    if (h && hm.Kp != Kp) { set_error("wh_filter_host: %s: the models' alphabets differ", hmm_paths[h]); return WH_EINVAL; }
    Kp = hm.Kp;
    uint32_t degen[32];
    degen_masks(hm.alphabet, degen);
    if ((rc = model_of(hm, degen, models[(size_t)h]))) return rc;
    thr[(size_t)h] = filter_thresholds(models[(size_t)h].evp, fo);
    maxM = std::max(maxM, hm.M);
  }
  const int64_t total = offsets[nq];
  if (check_residues(Kp, residues, total)) return WH_EINVAL;
  std::vector<int16_t> rows((size_t)7 * ((size_t)maxM + 1));
  int64_t c[4] = {nq * n, 0, 0, 0};
  for (int64_t q = 0; q < nq; q++)
    for (int h = 0; h < n; h++) {
      const FilterPairOut r = filter_pair_host(models[(size_t)h], thr[(size_t)h], residues + offsets[q], (int)(offsets[q + 1] - offsets[q]), rows.data(), fo.bias());
      const size_t p = (size_t)q * n + h;
      stage[p] = (uint8_t)r.stage;
      if (filter_bias_nats) filter_bias_nats[p] = r.bias_nats;
      if (msv_raw) msv_raw[p] = r.msv_raw;
      if (vit_raw) vit_raw[p] = r.vit_raw;
      c[1] += (r.stage & kStageMSV) != 0; c[2] += (r.stage & kStageBias) != 0; c[3] += (r.stage & kStageVit) != 0;
    }
  if (counts4) for (int i = 0; i < 4; i++) counts4[i] = c[i];
  return WH_OK;
}

int wh_score_filtered_dev(wh_ehmm *e, const uint8_t *d_residues, const int64_t *d_offsets, int64_t nq, int64_t total_residues, int32_t max_len,
                          const wh_filter_opts *opts, int32_t *d_decibits, uint8_t *d_flags, float *d_fwd_bits, wh_pair_detail *d_detail,
                          uint8_t *d_stage, void *stream) {
  if (!e || !d_residues || !d_offsets || !d_decibits || !d_flags || nq < 0 || max_len < 0) { set_error("wh_score_filtered_dev: bad argument"); return WH_EINVAL; }
  FilterOpts fo;
  int rc = options_of(opts, fo, "wh_score_filtered");
  if (rc) return rc;
  HIPCHK(hipSetDevice(e->device));
  FilterState *f = nullptr;
  if ((rc = state_of(e, &f))) return rc;
  if (nq == 0) return WH_OK;
  hipStream_t s = (hipStream_t)stream;
  const int H = (int)e->hmms.size();
  const size_t np = (size_t)nq * H;
  if (f->d_bias.ensure(4 * np) || f->d_keep.ensure((size_t)nq) || f->d_qmap.ensure(8 * (size_t)nq) || (!d_stage && f->d_stage.ensure(np)) || f->d_x3.ensure(4 * (size_t)H)) return WH_ENOMEM;
  uint8_t *stage = d_stage ? d_stage : (uint8_t *)f->d_stage.p;
  // 1. the filters
  if ((rc = run_filters(e, f, fo, d_residues, d_offsets, nq, max_len, stage, (float *)f->d_bias.p, nullptr, nullptr, s))) return rc;
  // 2. the queries with a pair past the Viterbi stage; their CSR on the host (one read-back)
  hipLaunchKernelGGL(keep_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, (const uint8_t *)stage, (long long)nq, H, (uint8_t *)f->d_keep.p);
  HIPCHK(hipGetLastError());
  f->h_keep.resize((size_t)nq); f->h_off.resize((size_t)nq + 1);
  HIPCHK(hipMemcpyAsync(f->h_keep.data(), f->d_keep.p, (size_t)nq, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(f->h_off.data(), d_offsets, 8 * ((size_t)nq + 1), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  f->h_qlist.clear(); f->h_coff.assign(1, 0); f->h_qmap.assign((size_t)nq, -1);
  int64_t cmax = 0;
  for (int64_t q = 0; q < nq; q++)
    if (f->h_keep[(size_t)q]) {
      const int64_t L = f->h_off[(size_t)q + 1] - f->h_off[(size_t)q];
      f->h_qmap[(size_t)q] = (int64_t)f->h_qlist.size();
      f->h_qlist.push_back(q);
      f->h_coff.push_back(f->h_coff.back() + L);
      cmax = std::max(cmax, L);
    }
  const int64_t nk = (int64_t)f->h_qlist.size(), ctotal = f->h_coff.back();
  const size_t nkp = (size_t)nk * H;
  HIPCHK(hipMemcpyAsync(f->d_qmap.p, f->h_qmap.data(), 8 * (size_t)nq, hipMemcpyHostToDevice, s));
  // 3. - 4. compact, score with the existing path
  if (nk > 0) {
    if (f->d_qlist.ensure(8 * (size_t)nk) || f->d_coff.ensure(8 * ((size_t)nk + 1)) || f->d_cres.ensure((size_t)ctotal + 16) || f->d_cdeci.ensure(4 * nkp) ||
        f->d_cflags.ensure(nkp) || f->d_cfwd.ensure(4 * nkp) || (d_detail && f->d_cdet.ensure(sizeof(wh_pair_detail) * nkp)))
      return WH_ENOMEM;
    HIPCHK(hipMemcpyAsync(f->d_qlist.p, f->h_qlist.data(), 8 * (size_t)nk, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(f->d_coff.p, f->h_coff.data(), 8 * ((size_t)nk + 1), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(gather_kernel, dim3((unsigned)nk), dim3(256), 0, s, d_residues, (const long long *)d_offsets, (const long long *)f->d_qlist.p,
                       (const long long *)f->d_coff.p, (uint8_t *)f->d_cres.p);
    HIPCHK(hipGetLastError());
    if ((rc = wh_score_dev(e, (const uint8_t *)f->d_cres.p, (const int64_t *)f->d_coff.p, nk, ctotal, (int32_t)cmax, (int32_t *)f->d_cdeci.p, (uint8_t *)f->d_cflags.p,
                           (float *)f->d_cfwd.p, d_detail ? (wh_pair_detail *)f->d_cdet.p : nullptr, stream)))
      return rc;
  }
  // 5. - 7. the Forward stage, the scatter back, the flags
  f->h_x3.resize((size_t)H);
  for (int h = 0; h < H; h++) f->h_x3[(size_t)h] = f->desc[(size_t)h].thr.x3;
  HIPCHK(hipMemcpyAsync(f->d_x3.p, f->h_x3.data(), 4 * (size_t)H, hipMemcpyHostToDevice, s));
  ScatterArgs sa;
  sa.nq = nq; sa.H = H; sa.qmap = (const long long *)f->d_qmap.p; sa.x3 = (const float *)f->d_x3.p; sa.bias = (const float *)f->d_bias.p; sa.stage = stage;
  sa.cdeci = (const int32_t *)f->d_cdeci.p; sa.cflags = (const uint8_t *)f->d_cflags.p; sa.cfwd = (const float *)f->d_cfwd.p; sa.cdet = (const wh_pair_detail *)f->d_cdet.p;
  sa.deci = d_decibits; sa.flags = d_flags; sa.fwd = d_fwd_bits; sa.det = d_detail; sa.counts = (unsigned long long *)f->d_counts.p;
  hipLaunchKernelGGL(scatter_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, s, sa);
  HIPCHK(hipGetLastError());
  f->handed = (int64_t)nkp; f->scored = true;
  return WH_OK;
}

int wh_score_filtered(wh_ehmm *e, const uint8_t *residues, const int64_t *offsets, int64_t nq, const wh_filter_opts *opts, int32_t *decibits,
                      uint8_t *flags, float *fwd_bits, wh_pair_detail *detail, uint8_t *stage) {
  if (!e || !residues || !offsets || !decibits || !flags || nq < 0) { set_error("wh_score_filtered: bad argument"); return WH_EINVAL; }
  FilterOpts fo;
  int rc = options_of(opts, fo, "wh_score_filtered");
  if (rc) return rc;
  if (nq == 0) return WH_OK;
  HIPCHK(hipSetDevice(e->device));
  FilterState *f = nullptr;
  if ((rc = state_of(e, &f))) return rc;
  const int64_t total = offsets[nq];
  if (check_residues(e->Kp, residues, total)) return WH_EINVAL;
  const size_t np = (size_t)nq * e->hmms.size();
  Staging st(e);
  const uint8_t *d_res = st.in(residues, (size_t)total, 16);
  const int64_t *d_off = st.in(offsets, sizeof(int64_t) * (size_t)(nq + 1));
  int32_t *d_deci = st.out(decibits, 4 * np);
  uint8_t *d_flags = st.out(flags, np);
  float *d_fwd = st.out(fwd_bits, 4 * np);
  wh_pair_detail *d_det = st.out(detail, sizeof(wh_pair_detail) * np);
  uint8_t *d_stage = st.out(stage, np);
  if (st.rc) return st.rc;
  return st.finish(wh_score_filtered_dev(e, d_res, d_off, nq, total, max_query_len(offsets, nq), opts, d_deci, d_flags, d_fwd, d_det, d_stage, nullptr));
}

/* test hook: how many float32 bit patterns in [first, last] have filter_log(x) != (float) log((double) x) of the host's libm */
int64_t wh_filter_log_differences(uint32_t first, uint32_t last) {
  int64_t n = 0;
  for (uint64_t u = first; u <= last; u++) {
    const uint32_t b = (uint32_t)u;
    float x, a, c;
    memcpy(&x, &b, 4);
    a = filter_log(x);
    c = (float)std::log((double)x);
    n += memcmp(&a, &c, 4) != 0;
  }
  return n;
}

int wh_last_filter_counts(wh_ehmm *e, int64_t out[6]) {
  if (!e || !out) { set_error("wh_last_filter_counts: bad argument"); return WH_EINVAL; }
  for (int i = 0; i < 6; i++) out[i] = 0;
  FilterState *f = e->filter.get();
  if (!f) return WH_OK;
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipDeviceSynchronize());
  unsigned long long c[8];
  HIPCHK(hipMemcpy(c, f->d_counts.p, sizeof c, hipMemcpyDeviceToHost));
  for (int i = 0; i < 4; i++) out[i] = (int64_t)c[i];
  out[4] = f->scored ? (int64_t)c[4] : 0;
  out[5] = f->scored ? f->handed : 0;
  return WH_OK;
}

}  // extern "C"
