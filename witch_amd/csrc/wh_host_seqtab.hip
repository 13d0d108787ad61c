// Host side of hmmsearch --tblout (include/witch_hip.h: wh_seq_expect, wh_seq_table, wh_last_seq_table_status): the
// counting sweep's launches (wh_seqtab.hip) over the pair list ordered by model, the row assembly around it, and the two
// device-free replicas (wh_seq_expect_host, wh_seq_table_host: the inline code of wh_seqtab.h).
#include <limits>

#include "wh_host.h"
#include "wh_seqtab.h"

using namespace whs;

// what the handle keeps for the stage: made by the first call
struct SeqTabState {
  DevBuf d_ws, d_gws, d_order, d_items, d_list, d_expect, d_count, d_evp;
  // host sources of asynchronous uploads: they outlive the call
  std::vector<int64_t> h_list, h_order, h_any;
  std::vector<SeqItem> h_items;
  std::vector<float> h_evp;
  int64_t rows = 0, any_pairs = 0;     // of the last wh_seq_table call; the last sweep's pairs on the any-size path
  bool table_called = false;
};

void wh_ehmm::SeqTabStateDelete::operator()(SeqTabState *f) const { delete f; }

namespace {

// d_count: [0 .. 3] the status words of the assembly (64-bit), behind them the work-queue heads of the sweep's launches
constexpr int kCountWords = 4, kMaxSeqLaunches = 16;
constexpr size_t kCountBytes = kCountWords * sizeof(unsigned long long) + kMaxSeqLaunches * sizeof(int);

int state_of(wh_ehmm *e, SeqTabState **out) {
  if (!e->seqtab) {
    std::unique_ptr<SeqTabState> f(new SeqTabState);
    if (f->d_count.ensure(kCountBytes)) return WH_ENOMEM;
    HIPCHK(hipMemset(f->d_count.p, 0, kCountBytes));
    e->seqtab.reset(f.release());
  }
  *out = e->seqtab.get();
  return WH_OK;
}

}  // namespace

extern "C" {

int wh_seq_expect_dev(wh_ehmm *e, const uint8_t *d_residues, const int64_t *d_offsets, int64_t nq, int64_t total_residues,
                      int32_t max_len, const int64_t *d_pair_list, int64_t n_pairs, wh_seq_expect_rec *d_out, void *stream) {
  (void)total_residues;
  if (!e || nq < 0 || n_pairs < 0 || max_len < 0 || (n_pairs > 0 && (!d_residues || !d_offsets || !d_pair_list || !d_out))) {
    set_error("wh_seq_expect_dev: bad argument");
    return WH_EINVAL;
  }
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipSetDevice(e->device));
  SeqTabState *st = nullptr;
  if (int rc = state_of(e, &st)) return rc;
  st->any_pairs = 0;
  if (n_pairs == 0) return WH_OK;
  if (n_pairs > 0x7FFFFFFF) { set_error("wh_seq_expect_dev: too many pairs"); return WH_ERANGE; }
  const int H = (int)e->hmms.size();
  const int64_t npairs_all = nq * H;
  // the pair list, read back: the work is ordered by model (a workgroup keeps one model's tables in LDS)
  st->h_list.resize((size_t)n_pairs);
  HIPCHK(hipMemcpyAsync(st->h_list.data(), d_pair_list, sizeof(int64_t) * (size_t)n_pairs, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  std::vector<int64_t> start((size_t)H + 1, 0);
  for (int64_t t = 0; t < n_pairs; t++) {
    const int64_t p = st->h_list[(size_t)t];
    if (p < 0 || p >= npairs_all) { set_error("wh_seq_expect_dev: pair_list[%lld] = %lld is not a pair of %lld queries x %d models", (long long)t, (long long)p, (long long)nq, H); return WH_EINVAL; }
    start[(size_t)(p % H) + 1]++;
  }
  for (int h = 0; h < H; h++) start[(size_t)h + 1] += start[(size_t)h];
  st->h_order.resize((size_t)n_pairs);
  {
    std::vector<int64_t> cur(start.begin(), start.end() - 1);
    for (int64_t t = 0; t < n_pairs; t++) st->h_order[(size_t)cur[(size_t)(st->h_list[(size_t)t] % H)]++] = t;
  }
  if (st->d_order.ensure(sizeof(int64_t) * (size_t)n_pairs)) return WH_ENOMEM;
  HIPCHK(hipMemcpyAsync(st->d_order.p, st->h_order.data(), sizeof(int64_t) * (size_t)n_pairs, hipMemcpyHostToDevice, s));
  // work items by register class; the models beyond the classes follow as one list of pairs
  struct ClassLaunch { int Q; size_t item0; int n_items; };
  std::vector<ClassLaunch> launches;
  st->h_items.clear();
  for (auto &kv : e->by_q) {
    ClassLaunch cl = {kv.first, st->h_items.size(), 0};
    for (int32_t h : kv.second)
      for (int64_t lo = start[(size_t)h]; lo < start[(size_t)h + 1]; lo += kSeqItemPairs) {
        SeqItem it;
        it.h = h; it.n = (int32_t)std::min<int64_t>(kSeqItemPairs, start[(size_t)h + 1] - lo); it.lo = lo;
        st->h_items.push_back(it);
        cl.n_items++;
      }
    if (cl.n_items > 0) launches.push_back(cl);
  }
  if ((int)launches.size() + 1 > kMaxSeqLaunches) { set_error("wh_seq_expect_dev: internal error: %zu register classes", launches.size()); return WH_EINVAL; }
  std::vector<int64_t> &any_order = st->h_any;
  any_order.clear();
  for (int32_t h : e->generic)
    for (int64_t t = start[(size_t)h]; t < start[(size_t)h + 1]; t++) any_order.push_back(st->h_order[(size_t)t]);
  st->any_pairs = (int64_t)any_order.size();
  const int Lcap = std::max(1, (int)max_len);
  SeqExpArgs a;
  memset(&a, 0, sizeof a);
  a.hmms = e->d_hmms.p; a.tables = (const float *)e->d_tables.p; a.gtab = (const double *)e->d_gtab.p;
  a.residues = d_residues; a.offsets = d_offsets; a.pair_list = d_pair_list; a.order = (const int64_t *)st->d_order.p;
  a.H = H; a.K = e->K; a.Kp = e->Kp; a.Lcap = Lcap; a.SP = row_stride(Lcap); a.Qmax = e->max_Q;
  a.out = d_out;
  int *heads = (int *)((unsigned long long *)st->d_count.p + kCountWords);
  HIPCHK(hipMemsetAsync(heads, 0, kMaxSeqLaunches * sizeof(int), s));
  // the items, and behind them the pairs of the any-size path
  const size_t any_at = (sizeof(SeqItem) * st->h_items.size() + 15) & ~(size_t)15;
  if (st->d_items.ensure(any_at + sizeof(int64_t) * any_order.size() + 16)) return WH_ENOMEM;
  if (!st->h_items.empty()) HIPCHK(hipMemcpyAsync(st->d_items.p, st->h_items.data(), sizeof(SeqItem) * st->h_items.size(), hipMemcpyHostToDevice, s));
  int64_t *d_any = (int64_t *)((char *)st->d_items.p + any_at);
  if (!any_order.empty()) HIPCHK(hipMemcpyAsync(d_any, any_order.data(), sizeof(int64_t) * any_order.size(), hipMemcpyHostToDevice, s));
  // every class launch of the call shares one workspace (they follow one another on the stream): sized for the largest
  struct ClassPlan { int Klds, seq_lds, blocks; size_t lds; int64_t ws_stride; };
  std::vector<ClassPlan> plans;
  size_t ws_bytes = 0;
  for (const ClassLaunch &cl : launches) {
    const int Q = cl.Q;
    ClassPlan pl;
    pl.Klds = seq_expect_lds_bytes(Q, e->K, 0) <= kLdsBudget ? e->K : 0;
    const int want = (Lcap + 15) & ~15;
    pl.seq_lds = seq_expect_lds_bytes(Q, pl.Klds, want) <= kLdsBudget ? want : 0;
    pl.lds = seq_expect_lds_bytes(Q, pl.Klds, pl.seq_lds);
    if (pl.lds > kLdsBudget) { set_error("wh_seq_expect_dev: the tables of %d cells per lane do not fit in LDS", Q); return WH_EINVAL; }
    pl.ws_stride = (int64_t)kSeqSpecArrays * a.SP + (pl.seq_lds ? 0 : residue_words(Lcap));
    pl.blocks = (int)std::min<int64_t>(cl.n_items, (int64_t)e->cu_count * std::max<size_t>(1, std::min<size_t>(3, kLdsBudget / pl.lds)));
    const size_t per_block = (size_t)kSeqWaves * (size_t)pl.ws_stride * sizeof(float);
    pl.blocks = clamp_blocks(pl.blocks, per_block, st->d_ws, e->max_M, Lcap, "wh_seq_expect_dev");
    if (pl.blocks < 0) return WH_ENOMEM;
    ws_bytes = std::max(ws_bytes, (size_t)pl.blocks * per_block);
    plans.push_back(pl);
  }
  if (st->d_ws.ensure(ws_bytes)) return WH_ENOMEM;
  int nl = 0;
  for (size_t c = 0; c < launches.size(); c++) {
    const ClassLaunch &cl = launches[c];
    const ClassPlan &pl = plans[c];
    a.Klds = pl.Klds; a.seq_lds = pl.seq_lds; a.ws_stride = pl.ws_stride;
    a.ws = (float *)st->d_ws.p;
    a.items = (const SeqItem *)st->d_items.p + cl.item0; a.n_items = cl.n_items;
    a.counter = heads + nl++;
    const hipError_t err = (hipError_t)seq_expect_launch(cl.Q, a, pl.blocks, pl.lds, s);
    if (err != hipSuccess) { set_error("wh_seq_expect_dev: launch of the %d-cell class failed: %s", cl.Q, hipGetErrorString(err)); return WH_EHIP; }
  }
  if (!any_order.empty()) {
    const size_t n_any = any_order.size();
    a.order = d_any; a.n_items = (int)n_any; a.items = nullptr;
    a.gws_stride = (int64_t)((seq_expect_any_doubles(Lcap, e->max_Q) + 1) & ~(size_t)1);
    int blocks = (int)std::min<int64_t>((int64_t)n_any, (int64_t)e->cu_count * 8);
    blocks = clamp_blocks(blocks, (size_t)a.gws_stride * sizeof(double), st->d_gws, e->max_M, Lcap, "wh_seq_expect_dev");
    if (blocks < 0) return WH_ENOMEM;
    if (st->d_gws.ensure((size_t)blocks * (size_t)a.gws_stride * sizeof(double))) return WH_ENOMEM;
    a.gws = (double *)st->d_gws.p;
    a.counter = heads + nl++;
    const hipError_t err = (hipError_t)seq_expect_any_launch(a, blocks, s);
    if (err != hipSuccess) { set_error("wh_seq_expect_dev: launch of the any-size kernel failed: %s", hipGetErrorString(err)); return WH_EHIP; }
  }
  return WH_OK;
}

int wh_seq_expect(wh_ehmm *e, const uint8_t *residues, const int64_t *offsets, int64_t nq, const int64_t *pair_list,
                  int64_t n_pairs, wh_seq_expect_rec *out) {
  if (!e || !residues || !offsets || nq < 0 || n_pairs < 0 || (n_pairs > 0 && (!pair_list || !out))) { set_error("wh_seq_expect: bad argument"); return WH_EINVAL; }
  if (n_pairs == 0) return WH_OK;
  HIPCHK(hipSetDevice(e->device));
  const int64_t total = offsets[nq];
  if (check_residues(e->Kp, residues, total)) return WH_EINVAL;
  Staging st(e);
  const uint8_t *d_res = st.in(residues, (size_t)total, 16);
  const int64_t *d_off = st.in(offsets, sizeof(int64_t) * (size_t)(nq + 1));
  const int64_t *d_list = st.in(pair_list, sizeof(int64_t) * (size_t)n_pairs);
  wh_seq_expect_rec *d_out = st.out(out, sizeof(wh_seq_expect_rec) * (size_t)n_pairs);
  if (st.rc) return st.rc;
  return st.finish(wh_seq_expect_dev(e, d_res, d_off, nq, total, max_query_len(offsets, nq), d_list, n_pairs, d_out, nullptr));
}

int wh_seq_expect_host(const char *const *hmm_paths, int n, const uint8_t *residues, const int64_t *offsets, int64_t nq,
                       const int64_t *pair_list, int64_t n_pairs, wh_seq_expect_rec *out) {
  if (!hmm_paths || n < 1 || !residues || !offsets || nq < 0 || n_pairs < 0 || (n_pairs > 0 && (!pair_list || !out))) { set_error("wh_seq_expect_host: bad argument"); return WH_EINVAL; }
  std::vector<HostHMM> hmms((size_t)n);
  std::vector<char> loaded((size_t)n, 0);
  for (int64_t t = 0; t < n_pairs; t++) {
    const int64_t p = pair_list[t];
    if (p < 0 || p >= nq * n) { set_error("wh_seq_expect_host: pair_list[%lld] = %lld is not a pair of %lld queries x %d models", (long long)t, (long long)p, (long long)nq, n); return WH_EINVAL; }
    const int h = (int)(p % n);
    if (!loaded[(size_t)h]) {
      if (!hmm_paths[h]) { set_error("wh_seq_expect_host: bad argument"); return WH_EINVAL; }
      if (int rc = parse_hmm_file(hmm_paths[h], hmms[(size_t)h])) return rc;
      configure_profile(hmms[(size_t)h]);
      loaded[(size_t)h] = 1;
    }
    const int64_t q = p / n;
    out[t] = seq_expect_pair_host(hmms[(size_t)h], residues + offsets[q], (int)(offsets[q + 1] - offsets[q]));
  }
  return WH_OK;
}

static int table_options(const wh_seq_table_opts *opts, wh_seq_table_opts &o, const char *who) {
  o.Z = 0; o.domZ = 0; o.E = 10.0; o.domE = 10.0; o.incE = 0.01; o.incdomE = 0.01;
  if (opts) o = *opts;
  if (!(o.E >= 0) || !(o.domE >= 0) || !(o.incE >= 0) || !(o.incdomE >= 0) || o.Z != o.Z || o.domZ != o.domZ) {
    set_error("%s: a threshold is negative or not a number", who);
    return WH_EINVAL;
  }
  return WH_OK;
}

int wh_seq_table_dev(wh_ehmm *e, const uint8_t *d_residues, const int64_t *d_offsets, int64_t nq, int64_t total_residues,
                     int32_t max_len, const uint8_t *d_flags, const wh_pair_detail *d_detail, const wh_seq_table_opts *opts,
                     wh_seq_row *d_out, int64_t cap, void *stream) {
  if (!e || nq < 0 || max_len < 0 || cap < 0 || (nq > 0 && (!d_residues || !d_offsets || !d_flags || !d_detail))) { set_error("wh_seq_table_dev: bad argument"); return WH_EINVAL; }
  wh_seq_table_opts o;
  if (int rc = table_options(opts, o, "wh_seq_table_dev")) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipSetDevice(e->device));
  SeqTabState *st = nullptr;
  if (int rc = state_of(e, &st)) return rc;
  const int H = (int)e->hmms.size();
  const int64_t npairs = nq * H;
  if (npairs > 0x7FFFFFFF) { set_error("wh_seq_table_dev: too many pairs"); return WH_ERANGE; }
  st->table_called = true; st->rows = 0; st->any_pairs = 0;
  unsigned long long *status = (unsigned long long *)st->d_count.p;
  HIPCHK(hipMemsetAsync(status, 0, kCountWords * sizeof(unsigned long long), s));
  if (npairs == 0) return 0;
  const int64_t list_cap = std::min(cap, npairs);
  if (st->d_list.ensure(sizeof(int64_t) * (size_t)list_cap + 16)) return WH_ENOMEM;
  hipError_t err = (hipError_t)seq_table_compact_launch(d_flags, npairs, (int64_t *)st->d_list.p, status, list_cap, s);
  if (err != hipSuccess) { set_error("wh_seq_table_dev: compaction kernel launch failed: %s", hipGetErrorString(err)); return WH_EHIP; }
  unsigned long long rows_u = 0;
  HIPCHK(hipMemcpyAsync(&rows_u, status, sizeof rows_u, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const int64_t rows = (int64_t)rows_u;
  st->rows = rows;
  if (rows > cap) { set_error("wh_seq_table_dev: %lld reported pairs, room for %lld rows", (long long)rows, (long long)cap); return WH_ERANGE; }
  if (rows == 0) return 0;
  if (!d_out) { set_error("wh_seq_table_dev: bad argument"); return WH_EINVAL; }
  if (!st->d_evp.p) {
    st->h_evp.assign((size_t)2 * H, std::numeric_limits<float>::quiet_NaN());
    for (int h = 0; h < H; h++) {
      const HostHMM &m = e->hmms[(size_t)h];
      if (m.has_fstats) { st->h_evp[(size_t)2 * h] = m.ftau; st->h_evp[(size_t)2 * h + 1] = m.flambda; }
    }
    if (st->d_evp.ensure(sizeof(float) * st->h_evp.size())) return WH_ENOMEM;
    HIPCHK(hipMemcpyAsync(st->d_evp.p, st->h_evp.data(), sizeof(float) * st->h_evp.size(), hipMemcpyHostToDevice, s));
  }
  if (st->d_expect.ensure(sizeof(wh_seq_expect_rec) * (size_t)rows)) return WH_ENOMEM;
  if (int rc = wh_seq_expect_dev(e, d_residues, d_offsets, nq, total_residues, max_len, (const int64_t *)st->d_list.p, rows,
                                 (wh_seq_expect_rec *)st->d_expect.p, stream))
    return rc;
  const double Z = o.Z > 0 ? o.Z : (double)nq, domZ = o.domZ > 0 ? o.domZ : (double)rows;
  SeqTabArgs a;
  memset(&a, 0, sizeof a);
  a.flags = d_flags; a.detail = d_detail; a.offsets = d_offsets; a.evp = (const float *)st->d_evp.p;
  a.expect = (const wh_seq_expect_rec *)st->d_expect.p; a.pair_list = (const int64_t *)st->d_list.p;
  a.npairs = npairs; a.rows = rows; a.H = H;
  a.lnE_Z = std::log(o.E / Z); a.lnIncE_Z = std::log(o.incE / Z); a.lnDomE_domZ = std::log(o.domE / domZ); a.lnIncDomE_domZ = std::log(o.incdomE / domZ);
  a.out = d_out; a.status = status;
  err = (hipError_t)seq_table_rows_launch(a, s);
  if (err != hipSuccess) { set_error("wh_seq_table_dev: row kernel launch failed: %s", hipGetErrorString(err)); return WH_EHIP; }
  return (int)rows;
}

int wh_seq_table(wh_ehmm *e, const uint8_t *residues, const int64_t *offsets, int64_t nq, const uint8_t *flags,
                 const wh_pair_detail *detail, const wh_seq_table_opts *opts, wh_seq_row *out, int64_t cap) {
  if (!e || !residues || !offsets || !flags || !detail || nq < 0 || cap < 0 || (cap > 0 && !out)) { set_error("wh_seq_table: bad argument"); return WH_EINVAL; }
  if (nq == 0) return 0;
  HIPCHK(hipSetDevice(e->device));
  const size_t np = (size_t)nq * e->hmms.size();
  const int64_t total = offsets[nq];
  if (check_residues(e->Kp, residues, total)) return WH_EINVAL;
  Staging st(e);
  const uint8_t *d_res = st.in(residues, (size_t)total, 16);
  const int64_t *d_off = st.in(offsets, sizeof(int64_t) * (size_t)(nq + 1));
  const uint8_t *d_flags = st.in(flags, np);
  const wh_pair_detail *d_det = st.in(detail, sizeof(wh_pair_detail) * np);
  wh_seq_row *d_out = st.out(out, sizeof(wh_seq_row) * (size_t)std::min<int64_t>(cap, (int64_t)np));
  if (st.rc) return st.rc;
  const int rows = wh_seq_table_dev(e, d_res, d_off, nq, total, max_query_len(offsets, nq), d_flags, d_det, opts, d_out, std::min<int64_t>(cap, (int64_t)np), nullptr);
  if (rows < 0) return rows;
  if (int rc = st.finish(WH_OK)) return rc;
  return rows;
}

int wh_seq_table_host(int H, const float *tau, const float *lambda, const int64_t *lengths, int64_t nq, const uint8_t *flags,
                      const wh_pair_detail *detail, const wh_seq_expect_rec *expect, const wh_seq_table_opts *opts,
                      wh_seq_row *out, int64_t cap) {
  if (H < 1 || !tau || !lambda || nq < 0 || cap < 0 || (nq > 0 && (!lengths || !flags || !detail))) { set_error("wh_seq_table_host: bad argument"); return WH_EINVAL; }
  wh_seq_table_opts o;
  if (int rc = table_options(opts, o, "wh_seq_table_host")) return rc;
  int64_t rows = 0;
  for (int64_t p = 0; p < nq * H; p++) rows += (flags[p] & WH_FLAG_REPORTED) ? 1 : 0;
  if (rows > cap) { set_error("wh_seq_table_host: %lld reported pairs, room for %lld rows", (long long)rows, (long long)cap); return WH_ERANGE; }
  if (rows > 0 && (!expect || !out)) { set_error("wh_seq_table_host: bad argument"); return WH_EINVAL; }
  int64_t status[4];
  return (int)seq_table_rows_host(H, tau, lambda, lengths, nq, flags, detail, expect, o, out, cap, status);
}

int wh_last_seq_table_status(wh_ehmm *e, int64_t out[4]) {
  if (!e || !out) { set_error("wh_last_seq_table_status: bad argument"); return WH_EINVAL; }
  out[0] = out[1] = out[2] = out[3] = 0;
  if (!e->seqtab || !e->seqtab->table_called) return WH_OK;
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipDeviceSynchronize());
  unsigned long long w[kCountWords];
  HIPCHK(hipMemcpy(w, e->seqtab->d_count.p, sizeof w, hipMemcpyDeviceToHost));
  out[0] = e->seqtab->rows; out[1] = (int64_t)w[1]; out[2] = (int64_t)w[2]; out[3] = e->seqtab->any_pairs;
  return WH_OK;
}

}  // extern "C"
