// Host side of wh_align_dev: the pairs grouped by model, the one-wave classes in float32 and (for the pairs that leave
// its range) in log space, then the wide and the float64 kernels for the models beyond them.  Each pass plans the launches
// of every class once, sizes and allocates the workspace from the plans, and launches from them.
#include "wh_host.h"

struct AlignCall {
  wh_ehmm *e;
  hipStream_t s;
  const uint8_t *d_residues; const int64_t *d_offsets; const int64_t *d_pair_q; const int32_t *d_pair_h; int64_t npairs;
  const int64_t *d_col_offsets; int32_t *d_cols;
  float *d_pp;                   // per-residue posterior probabilities, CSR like d_cols (wh_align_pp_dev), or NULL
  double *d_pp64;                // ... or as doubles (wh_align_pp64_dev); at most one of the two
  int32_t max_len; int Lc;
  int Lm;                        // length cap of the class launches (= Lc unless a class cannot plan the call's longest query: the longer queries' pairs go to the float64 kernel)
  int64_t n_long;                // such pairs of this call
  bool want_redo;                // pairs whose Backward sweep leaves float32 range are queued on the device and redone in log space
  int *d_redo_count; int32_t *d_redo_list;
  int launches;                  // of this call so far
  const int32_t *d_cfg_len;      // per query: the length its pairs' length model is configured for (wh_align_pp_len_dev), or NULL: its own
};

struct AlignClassPlan {
  int Q, first, n_items;         // cells per lane; the class's work items in d_items
  int waves, SP, wave_lds, Klds;
  size_t lds;
  bool spec_in_hbm;              // special-state rows in the wave's HBM region (long queries, long models)
  bool swap;                     // pass-synchronous variant: one orientation resident
  size_t scratch_stride, spec_stride;
  int blocks;
};

// pairs <pairs[0..n)> (ascending; NULL: all of 0..n) grouped by model: <cnt> prefix counts per model, <order> the pairs model by model
static void group_by_model(const int32_t *pairs, int64_t n, const std::vector<int32_t> &ph, int H, std::vector<int32_t> &order, std::vector<int32_t> &cnt) {
  cnt.assign((size_t)H + 1, 0);
  for (int64_t t = 0; t < n; t++) cnt[(size_t)ph[(size_t)(pairs ? pairs[t] : t)] + 1]++;
  for (int h = 0; h < H; h++) cnt[(size_t)h + 1] += cnt[(size_t)h];
  std::vector<int32_t> cursor(cnt.begin(), cnt.end() - 1);
  order.resize((size_t)n);
  for (int64_t t = 0; t < n; t++) { const int32_t p = pairs ? pairs[t] : (int32_t)t; order[(size_t)cursor[(size_t)ph[(size_t)p]]++] = p; }
}

// LDS plan of the alignment kernel for one size class (wh_plan.h: plan_align_lds); workgroups and workspace come later
static int plan_align_class(const AlignCall &c, int Q, AlignClassPlan *out) {
  AlignLds l;
  const int why = plan_align_lds(c.e->knobs.force_specg, c.e->K, Q, c.Lm, &l);
  if (why == 1) { set_error("query length %d with model class Q=%d does not fit in LDS", c.max_len, Q); return WH_ERANGE; }
  if (why != 0) { set_error("model class Q=%d does not fit in LDS", Q); return WH_ERANGE; }
  AlignClassPlan p = {};
  p.Q = Q; p.waves = l.waves; p.SP = l.SP; p.wave_lds = l.wave_lds; p.Klds = l.Klds; p.lds = l.lds; p.spec_in_hbm = l.spec_in_hbm; p.swap = l.swap;
  *out = p;
  return WH_OK;
}

// one pass over the one-wave classes for the pairs in <order> (grouped by model, cnt = prefix counts per model)
static int align_pass(AlignCall &c, const std::vector<int32_t> &order, const std::vector<int32_t> &cnt, bool logsp) {
  wh_ehmm *e = c.e;
  hipStream_t s = c.s;
  HIPCHK(hipMemcpyAsync(e->d_order.p, order.data(), sizeof(int32_t) * order.size(), hipMemcpyHostToDevice, s));
  std::vector<int32_t> items;   // all classes back to back: h, start, count
  std::vector<AlignClassPlan> plans;
  for (auto &kv : e->by_q) {
    AlignClassPlan p;
    if (int rc = plan_align_class(c, kv.first, &p)) return rc;
    p.first = (int)items.size() / 3;
    for (int h : kv.second) {
      int lo = cnt[(size_t)h], hi = cnt[(size_t)h + 1];
      for (int st = lo; st < hi; st += p.waves) { items.push_back(h); items.push_back(st); items.push_back(std::min(p.waves, hi - st)); }
    }
    p.n_items = (int)items.size() / 3 - p.first;
    if (p.n_items > 0) plans.push_back(p);
  }
  const size_t nit = items.size() / 3;
  std::vector<int32_t> soa(items.size());
  for (size_t t = 0; t < nit; t++) { soa[t] = items[3 * t]; soa[nit + t] = items[3 * t + 1]; soa[2 * nit + t] = items[3 * t + 2]; }
  if (e->d_items.ensure(sizeof(int32_t) * soa.size() + 16)) return WH_ENOMEM;
  HIPCHK(hipMemcpyAsync(e->d_items.p, soa.data(), sizeof(int32_t) * soa.size(), hipMemcpyHostToDevice, s));
  // the workspace of every class is sized first and allocated once; the launches use the workgroup counts it was sized for
  if (c.launches + (int)plans.size() > kMaxLaunches) { set_error("wh_align_dev: too many launches in one call"); return WH_ERANGE; }
  size_t need_scratch = 0, need_spec = 0;
  for (AlignClassPlan &p : plans) {
    p.scratch_stride = (size_t)(c.Lm + 1) * 5 * p.Q * kWave;
    p.spec_stride = p.spec_in_hbm ? (size_t)kAlignSpecArrays * p.SP : 0;
    p.blocks = clamp_blocks(std::min(p.n_items, e->cu_count * std::max(1, 8 / p.waves)), (size_t)p.waves * (p.scratch_stride + p.spec_stride) * sizeof(float), e->d_ascratch, e->max_M, c.Lm, "alignment");
    if (p.blocks < 0) return WH_ENOMEM;
    need_scratch = std::max(need_scratch, (size_t)p.blocks * p.waves * p.scratch_stride * sizeof(float));
    need_spec = std::max(need_spec, (size_t)p.blocks * p.waves * p.spec_stride * sizeof(float));
  }
  if (e->d_ascratch.ensure(need_scratch) || (need_spec && e->d_spec.ensure(need_spec))) return WH_ENOMEM;
  for (const AlignClassPlan &p : plans) {
    AlignArgsPP a;
    memset(&a, 0, sizeof a);
    a.hmms = (const DevHMM *)e->d_hmms.p; a.tables = (const float *)e->d_tables.p;
    a.residues = c.d_residues; a.offsets = c.d_offsets; a.pair_q = c.d_pair_q;
    a.order = (const int32_t *)e->d_order.p;
    a.item_h = (const int32_t *)e->d_items.p + p.first;
    a.item_start = (const int32_t *)e->d_items.p + nit + p.first;
    a.item_count = (const int32_t *)e->d_items.p + 2 * nit + p.first;
    a.n_items = p.n_items;
    a.col_offsets = c.d_col_offsets; a.cols = c.d_cols; a.pp = c.d_pp; a.pp64 = c.d_pp64; a.cfg_len = c.d_cfg_len;
    a.counter = e->counter(kSlotLaunch0 + c.launches);
    a.Lcap = c.Lm; a.SP = p.SP; a.wave_lds = p.wave_lds;
    a.K = e->K; a.Kp = e->Kp; a.Klds = p.Klds; a.swap = p.swap ? 1 : 0;
    a.logsp = logsp ? 1 : 0;
    a.no_window = e->knobs.no_window ? 1 : 0;
    a.wstat = logsp ? nullptr : e->counter(kSlotAlignStat);
    a.wcyc = (!logsp && (e->knobs.trace || e->knobs.stats)) ? reinterpret_cast<unsigned long long *>(e->counter(kSlotAlignCycles)) : nullptr;
    a.redo_count = (!logsp && c.want_redo) ? c.d_redo_count : nullptr;
    a.redo_list = (!logsp && c.want_redo) ? c.d_redo_list : nullptr;
    a.scratch_stride = p.scratch_stride; a.spec_stride = p.spec_stride;
    if (p.spec_in_hbm) a.spec_scratch = (float *)e->d_spec.p;
    a.scratch = (float *)e->d_ascratch.p;
    if (e->knobs.trace) fprintf(stderr, "[wh] align Q=%d waves=%d blocks=%d lds=%zu SP=%d wave_lds=%d items=%d swap=%d Klds=%d\n", p.Q, p.waves, p.blocks, p.lds, a.SP, a.wave_lds, a.n_items, a.swap, a.Klds);
    HIPCHK(hipMemsetAsync(a.counter, 0, sizeof(int), s));
    hipError_t err = launch_align(p.Q, a, p.blocks, p.waves * kWave, p.lds, s);
    if (err != hipSuccess) { set_error("align kernel launch (Q=%d) failed: %s", p.Q, hipGetErrorString(err)); return WH_EHIP; }
    c.launches++;
  }
  // the host vectors of this pass are consumed by async copies: drain before they go out of scope
  HIPCHK(hipStreamSynchronize(s));
  return WH_OK;
}

// the log-space pass: the pairs the float32 pass queued, grouped by model again.  A call that asks for PP does not run it:
// float32 logarithms of thousands of nats give posteriors good to percents (measured: up to 0.03 off, and above 1), which is
// no confidence value - the queued pairs are returned in <pp_redo> and aligned by the float64 any-size kernel, whose own
// log-space code is float64 (the hand-over the several-waves kernel makes through <status>)
static int align_logspace_pass(AlignCall &c, const std::vector<int32_t> &ph, int *n_redo, std::vector<int32_t> *pp_redo) {
  wh_ehmm *e = c.e;
  *n_redo = 0;
  if (!c.want_redo) return WH_OK;
  HIPCHK(hipMemcpyAsync(n_redo, c.d_redo_count, sizeof(int), hipMemcpyDeviceToHost, c.s));
  HIPCHK(hipStreamSynchronize(c.s));
  if (*n_redo <= 0) return WH_OK;
  std::vector<int32_t> redo((size_t)*n_redo), order2, cnt2;
  HIPCHK(hipMemcpyAsync(redo.data(), c.d_redo_list, sizeof(int32_t) * redo.size(), hipMemcpyDeviceToHost, c.s));
  HIPCHK(hipStreamSynchronize(c.s));
  std::sort(redo.begin(), redo.end());
  if (c.d_pp || c.d_pp64) {
    if (e->knobs.trace) fprintf(stderr, "[wh] align: %d of %lld pairs left float32 range, handed to the float64 kernel (PP)\n", *n_redo, (long long)c.npairs);
    *pp_redo = redo;
    return WH_OK;
  }
  group_by_model(redo.data(), *n_redo, ph, (int)e->hmms.size(), order2, cnt2);
  if (e->knobs.trace) fprintf(stderr, "[wh] align: %d of %lld pairs left float32 range, redone in log space\n", *n_redo, (long long)c.npairs);
  return align_pass(c, order2, cnt2, true);
}

// the window statistics of the float32 pass: wh_last_align_paths, and a report under WH_TRACE / WH_STATS
static int read_align_stats(const AlignCall &c) {
  wh_ehmm *e = c.e;
  int ws[kAlignStatInts] = {0};
  HIPCHK(hipMemcpyAsync(ws, e->counter(kSlotAlignStat), sizeof ws, hipMemcpyDeviceToHost, c.s));
  HIPCHK(hipStreamSynchronize(c.s));
  for (int t = 0; t < 4; t++) e->last_align_paths[t] = ws[t];
  if (!e->knobs.trace && !e->knobs.stats) return WH_OK;
  unsigned long long cy[4];
  memcpy(cy, ws + (kSlotAlignCycles - kSlotAlignStat), sizeof cy);
  fprintf(stderr, "[wh] align: %d + %d pairs on a 256- / 512-node window, %d windows rejected (full width), %d without a window; wave cycles of the window pairs: "
          "Forward %.3g, Backward+posteriors %.3g, OA fill %.3g, traceback %.3g\n", ws[0], ws[3], ws[1], ws[2], (double)cy[0], (double)cy[1], (double)cy[2], (double)cy[3]);
  fprintf(stderr, "[wh] align: window attempts by slack (lane blocks between the path's span with margins and the window, 0..7+): accepted");
  for (int t = 0; t < 8; t++) fprintf(stderr, " %d", ws[12 + t]);
  fprintf(stderr, "; rejected");
  for (int t = 0; t < 8; t++) fprintf(stderr, " %d", ws[20 + t]);
  fprintf(stderr, "\n");
  return WH_OK;
}

// models of 3 073 - 12 288 nodes: the several-waves-per-pair alignment kernel (wh_score_wide.hip), one launch per class of
// <witems>; the pairs that leave float32 range there are appended to <gitems> (the float64 kernel's)
static int align_wide(AlignCall &c, const std::map<int, std::vector<int32_t>> &witems, std::vector<int32_t> &gitems) {
  wh_ehmm *e = c.e;
  hipStream_t s = c.s;
  const int Lc = c.Lc;
  const size_t walds = wide_align_lds_bytes(Lc);
  if (e->d_recs.ensure(sizeof(int32_t) * ((size_t)c.npairs + 4))) return WH_ENOMEM;
  HIPCHK(hipMemsetAsync(e->d_recs.p, 0, sizeof(int32_t) * (size_t)c.npairs, s));
  size_t ooff = 0;
  std::vector<int32_t> all;
  for (auto &kv : witems) all.insert(all.end(), kv.second.begin(), kv.second.end());
  if (e->d_order.ensure(sizeof(int32_t) * (all.size() + (size_t)c.npairs))) return WH_ENOMEM;
  HIPCHK(hipMemcpyAsync(e->d_order.p, all.data(), sizeof(int32_t) * all.size(), hipMemcpyHostToDevice, s));
  int wclass = 0;
  for (auto &kv : witems) {
    const int W = kv.first & 15, wq = kv.first >> 4;
    WideAlignArgs wa;
    memset(&wa, 0, sizeof wa);
    wa.hmms = (const DevHMM *)e->d_hmms.p; wa.tables = (const float *)e->d_tables.p;
    wa.residues = c.d_residues; wa.offsets = c.d_offsets;
    wa.items = (const int32_t *)e->d_order.p + ooff; wa.n_items = (int)kv.second.size();
    ooff += kv.second.size();
    wa.pair_q = c.d_pair_q; wa.pair_h = c.d_pair_h; wa.col_off = c.d_col_offsets; wa.cols = c.d_cols; wa.pp = c.d_pp; wa.pp64 = c.d_pp64; wa.cfg_len = c.d_cfg_len;
    wa.status = (int32_t *)e->d_recs.p;
    if (wclass >= kWideAlignClasses) { set_error("too many classes of long models"); return WH_ERANGE; }
    wa.counter = e->counter(kSlotWideAlign + wclass++);
    wa.Lcap = Lc; wa.SP = row_stride(Lc);
    wa.K = e->K; wa.Kp = e->Kp;
    wa.scratch_stride = (size_t)(Lc + 1) * 5 * wq * W * kWave;
    int blocks = (int)std::min<size_t>(kv.second.size(), (size_t)e->cu_count);
    blocks = clamp_blocks(blocks, wa.scratch_stride * sizeof(float), e->d_wscratch, e->max_M, Lc, "wide alignment");
    if (blocks < 0) return WH_ENOMEM;
    if (e->d_wscratch.ensure((size_t)blocks * wa.scratch_stride * sizeof(float))) return WH_ENOMEM;
    wa.scratch = (float *)e->d_wscratch.p;
    HIPCHK(hipMemsetAsync(wa.counter, 0, sizeof(int), s));
    if (e->knobs.trace) fprintf(stderr, "[wh] wide alignment: %zu pairs, %d waves per pair, %d workgroups, lds %zu, slab %zu MB per workgroup\n", kv.second.size(), W, blocks, walds, wa.scratch_stride * 4 >> 20);
    hipError_t werr = launch_align_wide(wq, wa, blocks, W, walds, s);
    if (werr != hipSuccess) { set_error("wide alignment kernel launch failed: %s", hipGetErrorString(werr)); return WH_EHIP; }
    c.launches++;
  }
  std::vector<int32_t> wst((size_t)c.npairs);
  HIPCHK(hipMemcpyAsync(wst.data(), e->d_recs.p, sizeof(int32_t) * wst.size(), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  int n_hand = 0;
  for (size_t p = 0; p < wst.size(); p++) if (wst[p] == 1) { gitems.push_back((int32_t)p); n_hand++; }
  std::sort(gitems.begin(), gitems.end());
  e->last_align_redo += n_hand;
  if (e->knobs.trace && n_hand) fprintf(stderr, "[wh] wide alignment: %d pairs left float32 range, handed to the float64 kernel\n", n_hand);
  return WH_OK;
}

// pairs on models of more than 3072 nodes that the wide kernel does not serve: the any-size float64 alignment kernel
// (wh_generic.hip), one wavefront per pair
// doubles of one wave's slab of the any-size kernel for this call.  <longq>: a query beyond the LDS block (or, with pairs of
// the long-query pass, WH_LONGQ_FORCE) - the residues behind the wave's slab
// A call that asks for PP keeps the unrounded posterior rows between the two (<pp_off>: where); without PP the slab is
// what it was.
static size_t align_float64_stride(const AlignCall &c, bool *longq, size_t *pp_off = nullptr) {
  const wh_ehmm *e = c.e;
  *longq = (size_t)c.Lc + 64 > kLdsBudget ? !e->knobs.no_long_score : e->knobs.longq_force && c.n_long > 0;
  const size_t base = (generic_align_doubles(c.Lc, e->max_Q) + 1) & ~(size_t)1;
  if (pp_off) *pp_off = base;
  return base + ((c.d_pp || c.d_pp64) ? generic_align_pp_doubles(c.Lc, e->max_Q) : 0) + (*longq ? generic_seq_doubles(c.Lc) : 0);
}

static int align_float64(AlignCall &c, const std::vector<int32_t> &gitems) {
  wh_ehmm *e = c.e;
  hipStream_t s = c.s;
  const int Lc = c.Lc;
  GenericAlignArgs g;
  memset(&g, 0, sizeof g);
  g.hmms = (const DevHMM *)e->d_hmms.p; g.gtab = (const double *)e->d_gtab.p;
  g.residues = c.d_residues; g.offsets = c.d_offsets;
  HIPCHK(hipMemcpyAsync(e->d_order.p, gitems.data(), sizeof(int32_t) * gitems.size(), hipMemcpyHostToDevice, s));
  g.items = (const int32_t *)e->d_order.p; g.n_items = (int)gitems.size();
  g.pair_q = c.d_pair_q; g.pair_h = c.d_pair_h; g.col_off = c.d_col_offsets; g.cols = c.d_cols; g.pp = c.d_pp; g.pp64 = c.d_pp64; g.cfg_len = c.d_cfg_len;
  if (e->d_recs.ensure(sizeof(int32_t) * ((size_t)c.npairs + 4))) return WH_ENOMEM;
  HIPCHK(hipMemsetAsync(e->d_recs.p, 0, sizeof(int32_t) * (size_t)c.npairs, s));
  g.status = (int32_t *)e->d_recs.p;
  g.counter = e->counter(kSlotGenericAlign);
  g.Lcap = Lc; g.Qmax = e->max_Q; g.Kp = e->Kp;
  bool longq = false;
  g.slab_stride = align_float64_stride(c, &longq, &g.pp_off);
  const size_t glds = longq ? 64 : (size_t)Lc + 64;
  if (glds > kLdsBudget) { set_error("query length %d does not fit the any-size kernel's LDS", c.max_len); return WH_ERANGE; }
  int blocks = (int)std::min<size_t>(gitems.size(), (size_t)e->cu_count * std::min<size_t>(12, kLdsBudget / glds));
  blocks = clamp_blocks(blocks, g.slab_stride * sizeof(double), e->d_rmx, e->max_M, Lc, "any-size alignment");
  if (blocks < 0) return WH_ENOMEM;
  if (e->d_rmx.ensure((size_t)blocks * g.slab_stride * sizeof(double))) return WH_ENOMEM;
  g.slab = (double *)e->d_rmx.p;
  HIPCHK(hipMemsetAsync(g.counter, 0, sizeof(int), s));
  if (e->knobs.trace) fprintf(stderr, "[wh] any-size alignment: %zu pairs (%lld of queries beyond %d residues), %d wavefronts, slab %zu MB per wave%s\n", gitems.size(), (long long)c.n_long, c.Lm, blocks, g.slab_stride * 8 >> 20, longq ? ", residues in HBM" : "");
  hipError_t gerr = launch_generic_align(g, blocks, glds, s, longq);
  if (gerr != hipSuccess) { set_error("any-size alignment kernel launch failed: %s", hipGetErrorString(gerr)); return WH_EHIP; }
  c.launches++;
  std::vector<int32_t> st((size_t)c.npairs);
  HIPCHK(hipMemcpyAsync(st.data(), e->d_recs.p, sizeof(int32_t) * st.size(), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));     // gitems is the caller's local
  int n_range = 0, n_log = 0;
  for (size_t p = 0; p < st.size(); p++) { n_range += st[p] == 3; n_log += st[p] == 4 || st[p] == 3; }
  e->last_align_unaligned = 0;        // (round 5: no pair is left unaligned for its range - see generic_align_kernel)
  e->last_align_redo += n_log;
  if (e->knobs.trace && n_log > 0) fprintf(stderr, "[wh] any-size alignment: %d pairs left float64 range, redone in log space\n", n_log);
  if (n_range > 0)
    fprintf(stderr, "[wh] note: on %d pair(s) on models of more than %d nodes the log-space Forward and Backward scores disagree; "
                    "aligned from the Forward-normalised posteriors, as hmmalign does\n", n_range, kMaxQ * kWave);
  return WH_OK;
}

extern "C" int wh_align_dev(wh_ehmm *e, const uint8_t *d_residues, const int64_t *d_offsets, int64_t nq, int64_t total_residues,
                            int32_t max_len, const int64_t *d_pair_q, const int32_t *d_pair_h, int64_t npairs,
                            const int64_t *d_col_offsets, int32_t *d_cols, void *stream) {
  return wh_align_pp_dev(e, d_residues, d_offsets, nq, total_residues, max_len, d_pair_q, d_pair_h, npairs, d_col_offsets, d_cols, nullptr, stream);
}

// both PP entry points: <d_pp> floats, or <d_pp64> doubles, or neither
static int align_dev(wh_ehmm *e, const uint8_t *d_residues, const int64_t *d_offsets, int64_t nq, int64_t total_residues,
                     int32_t max_len, const int64_t *d_pair_q, const int32_t *d_pair_h, int64_t npairs,
                     const int64_t *d_col_offsets, int32_t *d_cols, float *d_pp, double *d_pp64, const int32_t *d_cfg_len, void *stream);

extern "C" int wh_align_pp_dev(wh_ehmm *e, const uint8_t *d_residues, const int64_t *d_offsets, int64_t nq, int64_t total_residues,
                               int32_t max_len, const int64_t *d_pair_q, const int32_t *d_pair_h, int64_t npairs,
                               const int64_t *d_col_offsets, int32_t *d_cols, float *d_pp, void *stream) {
  return align_dev(e, d_residues, d_offsets, nq, total_residues, max_len, d_pair_q, d_pair_h, npairs, d_col_offsets, d_cols, d_pp, nullptr, nullptr, stream);
}

// wh_align_pp_dev under a length model of the caller's choice: <d_cfg_len>[nq], or NULL for wh_align_pp_dev itself
extern "C" int wh_align_pp_len_dev(wh_ehmm *e, const uint8_t *d_residues, const int64_t *d_offsets, int64_t nq, int64_t total_residues,
                                   int32_t max_len, const int64_t *d_pair_q, const int32_t *d_pair_h, int64_t npairs,
                                   const int64_t *d_col_offsets, int32_t *d_cols, float *d_pp, const int32_t *d_cfg_len, void *stream) {
  return align_dev(e, d_residues, d_offsets, nq, total_residues, max_len, d_pair_q, d_pair_h, npairs, d_col_offsets, d_cols, d_pp, nullptr, d_cfg_len, stream);
}

extern "C" int wh_align_pp64_dev(wh_ehmm *e, const uint8_t *d_residues, const int64_t *d_offsets, int64_t nq, int64_t total_residues,
                                 int32_t max_len, const int64_t *d_pair_q, const int32_t *d_pair_h, int64_t npairs,
                                 const int64_t *d_col_offsets, int32_t *d_cols, double *d_pp64, void *stream) {
  return align_dev(e, d_residues, d_offsets, nq, total_residues, max_len, d_pair_q, d_pair_h, npairs, d_col_offsets, d_cols, nullptr, d_pp64, nullptr, stream);
}

static int align_dev(wh_ehmm *e, const uint8_t *d_residues, const int64_t *d_offsets, int64_t nq, int64_t total_residues,
                     int32_t max_len, const int64_t *d_pair_q, const int32_t *d_pair_h, int64_t npairs,
                     const int64_t *d_col_offsets, int32_t *d_cols, float *d_pp, double *d_pp64, const int32_t *d_cfg_len, void *stream) {
  (void)nq; (void)total_residues;
  if (!e || !d_residues || !d_offsets || !d_pair_q || !d_pair_h || !d_col_offsets || !d_cols || npairs < 0 || max_len < 0) {
    set_error("wh_align_dev: bad argument");
    return WH_EINVAL;
  }
  AlignCall c = {e, (hipStream_t)stream, d_residues, d_offsets, d_pair_q, d_pair_h, npairs, d_col_offsets, d_cols, d_pp, d_pp64, max_len, std::max(max_len, 1)};
  c.d_cfg_len = d_cfg_len;
  hipStream_t s = c.s;
  HIPCHK(hipSetDevice(e->device));
  if (npairs == 0) { e->timers[2].launches = 0; e->timers[2].ms = 0; return WH_OK; }
  if (npairs > 0x7FFFFFFF) { set_error("too many pairs"); return WH_ERANGE; }
  // group the pairs by model on the host (the model's tables are shared through LDS by a workgroup)
  std::vector<int32_t> ph((size_t)npairs), order, cnt;
  HIPCHK(hipMemcpyAsync(ph.data(), d_pair_h, sizeof(int32_t) * (size_t)npairs, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const int H = (int)e->hmms.size();
  for (int64_t p = 0; p < npairs; p++)
    if (ph[(size_t)p] < 0 || ph[(size_t)p] >= H) { set_error("pair %lld: model position %d out of range", (long long)p, ph[(size_t)p]); return WH_EINVAL; }
  // The class launches keep the query in LDS.  A call whose longest query a size class cannot plan sizes them for the lengths
  // every class accepts (wh_plan.h); the pairs of longer queries on those classes' models are aligned by the any-size float64
  // kernel, which serves models beyond 3 072 nodes from a pair list already.  Every other pair keeps its class launch.
  c.Lm = main_length_cap(e, c.Lc, true, true);
  c.n_long = 0;
  e->last_long_align[0] = e->last_long_align[1] = 0;
  std::vector<int32_t> short_pairs, long_pairs;
  if (c.Lm < c.Lc) {
    std::vector<int64_t> offs((size_t)nq + 1), pq((size_t)npairs);
    HIPCHK(hipMemcpyAsync(offs.data(), d_offsets, sizeof(int64_t) * offs.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(pq.data(), d_pair_q, sizeof(int64_t) * pq.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int64_t p = 0; p < npairs; p++) {
      const int64_t q = pq[(size_t)p];
      if (q < 0 || q >= nq) { set_error("pair %lld: query %lld out of range", (long long)p, (long long)q); return WH_EINVAL; }
      const int64_t L = offs[(size_t)q + 1] - offs[(size_t)q];
      if (L > c.Lm && e->dev[(size_t)ph[(size_t)p]].Q <= kMaxQ) { long_pairs.push_back((int32_t)p); e->last_long_align[1] = std::max<int64_t>(e->last_long_align[1], L); }
      else short_pairs.push_back((int32_t)p);
    }
    c.n_long = (int64_t)long_pairs.size();
    e->last_long_align[0] = c.n_long;
  }
  if (c.n_long > 0) group_by_model(short_pairs.data(), (int64_t)short_pairs.size(), ph, H, order, cnt);
  else group_by_model(nullptr, npairs, ph, H, order, cnt);
  // a pair on a model beyond the register kernels may end on the float64 kernel, a pair of the long-query pass does: refuse
  // the call before anything is launched when not even one wave's slab of that kernel fits on the device
  for (int h = 0; h < H; h++)
    if (c.n_long > 0 || (cnt[(size_t)h + 1] > cnt[(size_t)h] && e->dev[(size_t)h].Q > kMaxQ)) {
      bool longq = false;
      if (!one_block_fits(align_float64_stride(c, &longq) * sizeof(double), e->d_rmx, e->max_M, c.Lc, "any-size alignment"))
        return WH_ENOMEM;
      break;
    }
  if (e->d_order.ensure(sizeof(int32_t) * (size_t)npairs)) return WH_ENOMEM;
  c.want_redo = !e->knobs.no_logspace;
  if (e->d_recs.ensure(sizeof(int32_t) * ((size_t)npairs + 4))) return WH_ENOMEM;
  c.d_redo_count = (int *)e->d_recs.p;
  c.d_redo_list = (int32_t *)e->d_recs.p + 4;
  HIPCHK(hipMemsetAsync(c.d_redo_count, 0, sizeof(int), s));
  HIPCHK(hipMemsetAsync(e->counter(kSlotAlignStat), 0, kAlignStatInts * sizeof(int), s));
  if (timer_begin(e, 2, s)) return WH_EHIP;
  int n_redo = 0;
  std::vector<int32_t> pp_redo;
  if (!order.empty()) {          // (empty: every pair of the call is the long-query pass's)
    if (int rc = align_pass(c, order, cnt, false)) return rc;
    if (int rc = align_logspace_pass(c, ph, &n_redo, &pp_redo)) return rc;
  }
  if (int rc = read_align_stats(c)) return rc;
  e->last_align_redo = n_redo;
  e->last_align_unaligned = 0;
  e->last_unaligned_pairs.clear();
  if (!e->generic.empty() || e->force_wide || c.n_long > 0 || !pp_redo.empty()) {
    // models of 3 073 - 12 288 nodes go to the wide kernel; pairs that leave float32 range there, longer queries and
    // larger models (the 48-cell scoring class included) to the float64 kernel
    const bool use_wide = wide_align_lds_bytes(c.Lc) <= kLdsBudget && !e->wide_by_w.empty() && !e->knobs.no_wide_align;
    std::vector<int32_t> gitems(long_pairs);
    gitems.insert(gitems.end(), pp_redo.begin(), pp_redo.end());
    std::map<int, std::vector<int32_t>> witems;
    std::vector<char> is_long(c.n_long > 0 ? (size_t)npairs : 0, 0);
    for (int32_t p : long_pairs) is_long[(size_t)p] = 1;
    for (int64_t p = 0; p < npairs; p++) {
      const DevHMM &dm = e->dev[(size_t)ph[(size_t)p]];
      if (c.n_long > 0 && is_long[(size_t)p]) continue;
      if (use_wide && dm.wideW > 0 && dm.wideQ != kWideQBig && (dm.Q > kMaxQ || e->force_wide)) witems[dm.wideQ * 16 + dm.wideW].push_back((int32_t)p);
      else if (dm.Q > kMaxQ) gitems.push_back((int32_t)p);
    }
    if (!witems.empty()) if (int rc = align_wide(c, witems, gitems)) return rc;
    std::sort(gitems.begin(), gitems.end());
    if (!gitems.empty()) if (int rc = align_float64(c, gitems)) return rc;
  }
  if (timer_end(e, 2, s, c.launches)) return WH_EHIP;
  return WH_OK;
}
