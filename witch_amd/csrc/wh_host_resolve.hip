// Host side of the resolver stage of wh_score_dev: the main resolver launch over the queue the scoring launches filled, and
// the follow-up passes inside the same call (long-list, big-region, long-query), each a function that returns a WH_* code.
#include <chrono>

#include "wh_host.h"

// The order of the resolver's queue, from the pairs' cost keys and models alone (no device work).  Pairs are grouped model
// by model (longest pair first inside a model): the waves of a workgroup work on ONE model at a time, so they share the
// staged tables and, for the models whose tables stay in L2, stream the same arrays (wh_resolve.hip: slots and segments).
struct QueueOrder {
  std::vector<int32_t> ord;      // queue positions in launch order
  std::vector<int32_t> chunks;   // one segment per model: start, count, model, its cells per lane
  std::vector<int32_t> slots;    // the segment each slot (a workgroup's turn) serves
};
static QueueOrder order_queue(const std::vector<float> &keys, const std::vector<int32_t> &models, const std::vector<DevHMM> &dev, bool small_queue, int cu_count, int waves) {
  const int n = (int)keys.size();
  QueueOrder o;
  o.ord.resize((size_t)n);
  for (int t = 0; t < n; t++) o.ord[(size_t)t] = t;
  const std::vector<int32_t> &ord = o.ord;
  // A small queue (fewer than eight pairs per wave: the reference's example data as shipped, 2 103 pairs) is ONE
  // segment in descending cost, models mixed, tables from L2: there the order decides the tail of the launch and
  // nothing else matters.  Otherwise: model by model.
  if (small_queue)
    std::stable_sort(o.ord.begin(), o.ord.end(), [&](int32_t x, int32_t y) { return keys[(size_t)x] > keys[(size_t)y]; });
  else
    std::stable_sort(o.ord.begin(), o.ord.end(), [&](int32_t x, int32_t y) {
      return models[(size_t)x] != models[(size_t)y] ? models[(size_t)x] < models[(size_t)y] : keys[(size_t)x] > keys[(size_t)y];
    });
  // one segment per model; slots in proportion to the segments' cost (four per workgroup in all, at least one per model)
  struct Seg { int start, count, h; double cost; };
  std::vector<Seg> segs;
  double total_cost = 0.0;
  if (small_queue) { segs.push_back({0, n, -1, 1.0}); total_cost = 1.0; }
  for (int t = small_queue ? n : 0; t < n;) {
    const int h = models[(size_t)ord[(size_t)t]];
    int u = t;
    double cost = 0.0;
    while (u < n && models[(size_t)ord[(size_t)u]] == h) { cost += std::max(1.0f, keys[(size_t)ord[(size_t)u]]); u++; }
    segs.push_back({t, u - t, h, cost});
    total_cost += cost;
    t = u;
  }
  std::vector<int> order_s(segs.size());
  for (size_t t = 0; t < segs.size(); t++) order_s[t] = (int)t;
  std::stable_sort(order_s.begin(), order_s.end(), [&](int x, int y) { return segs[(size_t)x].cost > segs[(size_t)y].cost; });
  const double per_slot = total_cost / (4.0 * (double)cu_count);
  for (int sidx : order_s) {
    const Seg &g = segs[(size_t)sidx];
    int ns = (int)std::ceil(g.cost / std::max(per_slot, 1e-30));
    ns = std::max(1, std::min(ns, std::max(1, (g.count + 7) / 8)));       // never more slots than groups of eight pairs
    if (small_queue) ns = std::max(1, std::min(cu_count, (g.count + waves - 1) / waves));
    for (int v = 0; v < ns; v++) o.slots.push_back(sidx);
  }
  o.chunks.reserve(segs.size() * 4);
  for (const Seg &g : segs) { o.chunks.push_back(g.start); o.chunks.push_back(g.count); o.chunks.push_back(g.h); o.chunks.push_back(g.h >= 0 ? dev[(size_t)g.h].Q : 0); }
  return o;
}

static int print_resolver_stats(const ScoreCall &c, const ResolveArgs &r, int n_multi, int blocks, int waves) {
  unsigned long long st[24];
  if (int rc = stats_read(c, r.stats, st)) return rc;
  const double tot = (double)(st[0] + st[1] + st[2] + st[3] + st[4]);
  const double fetches = (double)std::max<unsigned long long>(1, st[8] + st[9] + st[10]);
  fprintf(stderr, "[wh] resolver wave cycles: region Forward %.1f%%  traces %.1f%%  clustering %.1f%%  cluster statistics %.1f%%  envelope Forward %.1f%%  (%.3g cycles per pair)\n",
          100.0 * st[0] / tot, 100.0 * st[1] / tot, 100.0 * st[2] / tot, 100.0 * st[3] / tot, 100.0 * st[4] / tot, tot / n_multi);
  fprintf(stderr, "[wh]   inside the traces: decision fetches %.1f%%  E-state choice %.1f%%  null2/accumulators/segments %.1f%%  (of the trace cycles)\n",
          100.0 * st[5] / (double)st[1], 100.0 * st[6] / (double)st[1], 100.0 * st[7] / (double)st[1]);
  fprintf(stderr, "[wh]   per multidomain region and trace: %.1f fetches of M runs, %.1f of D runs, %.1f of flank (C/J) runs, %.1f single I steps; %.0f cycles per fetch\n",
          st[8] / (200.0 * n_multi), st[9] / (200.0 * n_multi), st[10] / (200.0 * n_multi), st[11] / (200.0 * n_multi), (double)st[5] / fetches);
  fprintf(stderr, "[wh]   threshold-line cache: %.1f%% of the fetches hit\n", 100.0 * st[12] / fetches);
  fprintf(stderr, "[wh]   fetch order: %.1f%% of the fetches are the one that followed the last matched fetch in the previous trace, %.1f%% re-synchronise elsewhere in it\n",
          100.0 * st[20] / fetches, 100.0 * st[21] / fetches);
  fprintf(stderr, "[wh]   the line's load alone (issue -> validated): %.0f cycles per fetch\n", (double)st[23] / fetches);
  fprintf(stderr, "[wh]   shader clock while a pair is resolved: %.2f GHz (cycle counter / 100 MHz real-time counter); pair cycles %.3g\n", st[15] ? 0.1 * (double)st[14] / (double)st[15] : 0.0, (double)st[14]);
  fprintf(stderr, "[wh]   wave lifetimes: %llu waves, mean %.1f ms, longest %.1f ms (a wave leaves when no slot is left)\n", st[19], st[19] ? 1e-5 * (double)st[17] / (double)st[19] : 0.0, 1e-5 * (double)st[18]);
  fprintf(stderr, "[wh]   waiting at the workgroup's slot barriers: %.1f%% on top of the pair cycles (%d slots on %d models, %d workgroups of %d waves)\n", 100.0 * st[13] / tot, r.n_slots, r.n_chunks, blocks, waves);
  return WH_OK;
}

// what every resolver launch of a call shares: tables, queue, outputs, the layout of a wave's matrix slab
// <Lc>: the launch's length cap (a pair of a longer query is listed for the long-query pass)
static ResolveArgs resolve_args(const ScoreCall &c, const int32_t *rext, int64_t rext_stride, int Lc) {
  wh_ehmm *e = c.e;
  const int Qmax = e->max_Q;
  ResolveArgs r;
  memset(&r, 0, sizeof r);
  r.rext = rext; r.rext_stride = rext_stride;
  r.hmms = (const DevHMM *)e->d_hmms.p; r.gtab = (const double *)e->d_gtab.p; r.ftab = (const float *)e->d_tables.p;
  r.residues = c.d_residues; r.offsets = c.d_offsets;
  r.recs = (const ResolveRec *)e->d_rrecs.p; r.count = e->counter(kSlotResolveCount); r.rec_cap = (int)e->rq_cap;
  r.counter = e->counter(kSlotResolveWork);
  r.Lcap = Lc; r.Mmax = e->max_M;
  // a wave's slab: matrix rows | threshold-line cache of the walk | E-state row cache (at the end)
  r.dc_off = ((size_t)(Lc + 2) * ((size_t)3 * Qmax * kWave + 8) + 1) & ~(size_t)1;
  r.mx_stride = r.dc_off + resolve_dcache_doubles() + (size_t)(Lc + 2) * resolve_tail_row_doubles();
  r.mx_stride = (r.mx_stride + 1) & ~(size_t)1;      // every wave's slab 16-byte aligned: the Forward sweep moves node pairs
  r.seg_cap = resolve_seg_cap();
  r.seg_stride = resolve_seg_ints(Lc, e->max_M);
  r.decibits = c.d_decibits; r.flags = c.d_flags; r.detail = c.d_detail;
  r.H = c.H; r.K = e->K; r.Kp = e->Kp;
  memcpy(r.degen, e->degen, sizeof r.degen);
  r.dbg = e->knobs.rdbg;
  r.launch_id = ++e->resolver_launches;
  r.fb = e->d_feedback();
  r.null2_gather = c.res_null2_gather ? 1 : 0;
  return r;
}

// The feedback block in front of a resolver launch: counts zeroed, the lists the launch appends to (a capacity of 0: none.
// Without a long list the launch's length cap is the call's longest query).  wrong_model is left alone: it is read by the
// NEXT call.
static int reset_feedback(const ScoreCall &c, int32_t *big_list, int big_cap, int32_t *long_list = nullptr, int long_cap = 0) {
  ResolveFeedback &fb = c.e->feedback;
  fb = {};
  fb.big_list = big_list; fb.big_cap = big_cap; fb.long_list = long_list; fb.long_cap = long_cap;
  HIPCHK(hipMemcpyAsync((char *)c.e->d_feedback() + kFeedbackUploadFrom, (const char *)&fb + kFeedbackUploadFrom, sizeof fb - kFeedbackUploadFrom, hipMemcpyHostToDevice, c.s));
  return WH_OK;
}
// ... and what the launches since then reported (synchronises)
static int read_feedback(const ScoreCall &c, ResolveFeedback *fb) {
  HIPCHK(hipMemcpyAsync(fb, c.e->d_feedback(), sizeof *fb, hipMemcpyDeviceToHost, c.s));
  HIPCHK(hipStreamSynchronize(c.s));
  return WH_OK;
}

// The queue a follow-up pass works on, which is the one of the launch that listed its pairs: d_rrecs, with the regions in
// <rext> for a round of the long-list pass; <n> records, so no list of queue positions is longer.
struct ListedQueue { const int32_t *rext; int64_t rext_stride; int n; };

// ---- the big-region pass.  The resolver keeps the domains of a sampled trace (32), the significant clusters (64) and the
// sampled segments (8 192) of a region in lists of fixed length: LDS and a small HBM block per wave, eight waves per CU.
// hmmsearch has no such limit (a tandem repeat of 96 copies is ONE region of 96 domains per trace, 19 200 segments, 96
// clusters).  A launch counts what such a region needs and lists the pair; this pass runs the listed pairs again with every
// list in HBM, sized from the counts: few waves (one per workgroup) with large blocks.
struct ListCaps { int dom, seg, clus; };     // entries per wave
// From the counts a launch recorded; a count of 0 means that list was long enough (all 0: the default sizes).  A significant
// cluster holds segments of at least 25 % of the 200 traces, so seg / 50 clusters are enough whatever the (truncated) first
// clustering counted.
static ListCaps plan_big_regions(const ResolveFeedback &fb) {
  const int seg = std::max(resolve_seg_cap(), (fb.big_segs + 255) & ~255);
  return {std::max(resolve_dom_max(), (fb.big_doms + 63) & ~63), seg, std::max(std::max(resolve_clus_max(), fb.big_clus), seg / 50 + 1)};
}
static void note_big_counts(wh_ehmm *e, const ResolveFeedback &fb) {
  e->last_big[1] = std::max<int64_t>(e->last_big[1], fb.big_doms);
  e->last_big[2] = std::max<int64_t>(e->last_big[2], fb.big_segs);
  e->last_big[3] = std::max<int64_t>(e->last_big[3], fb.big_clus);
}

// ONE launch of resolve_big_kernel, or of resolve_long_kernel (<long_q>), over the <n> positions of <q> listed in <src>, with
// the length cap <Lc> and lists of <caps> entries; a pair with a region beyond them is listed in <dst> (NULL: it keeps
// WH_FLAG_TRUNC).  <fb>: what the launch reported.  In the long kernel a wave's LDS block does not hold the query, so a
// workgroup runs several waves where the device has room for their slabs.
static int launch_listed(const ScoreCall &c, bool long_q, int Lc, const ListCaps &caps, const int32_t *src, int n, int32_t *dst, const ListedQueue &q, int *rlaunches, ResolveFeedback *fb) {
  wh_ehmm *e = c.e;
  const char *what = long_q ? "long-query pass" : "big-region pass";
  const size_t rlds = long_q ? resolve_long_lds_bytes(e->max_M) : resolve_lds_bytes(Lc, e->max_M);
  ResolveArgs r = resolve_args(c, q.rext, q.rext_stride, Lc);
  r.long_query = long_q ? 1 : 0;
  r.dom_cap = caps.dom; r.seg_cap = caps.seg; r.clus_cap = caps.clus;
  r.seg_stride = long_q ? resolve_long_seg_ints(Lc, e->max_M, caps.dom, caps.seg, caps.clus) : (resolve_big_seg_ints(Lc, e->max_M, caps.dom, caps.seg, caps.clus) + 3) & ~(size_t)3;
  r.wave_lds_ints = (int)(rlds / 4);
  const size_t per_wave = r.mx_stride * sizeof(double) + r.seg_stride * sizeof(int32_t);
  int waves = 1;
  if (long_q) {
    waves = std::max(1, std::min(std::min(resolve_waves_per_cu(), (int)((kLdsBudget - resolve_lds_header_bytes(0)) / rlds)), n / e->cu_count));
    if (c.res_waves > 0) waves = std::min(waves, c.res_waves);
    size_t free_b = 0, total_b = 0;
    if (waves > 1 && hipMemGetInfo(&free_b, &total_b) == hipSuccess)
      while (waves > 1 && (double)waves * (double)per_wave > 0.7 * (double)(free_b + e->d_rmx.cap)) waves--;
  }
  const size_t lds_total = resolve_lds_header_bytes(0) + (size_t)waves * rlds;
  int blocks = std::min((n + waves - 1) / waves, e->cu_count);
  const size_t per_block = (size_t)waves * per_wave;
  blocks = clamp_blocks(blocks, per_block, e->d_rmx, e->max_M, Lc, what);
  if (blocks < 0) return WH_ENOMEM;
  if (e->d_rmx.ensure((size_t)blocks * waves * r.mx_stride * sizeof(double)) || e->d_bigsegs.ensure((size_t)blocks * waves * r.seg_stride * sizeof(int32_t))) {
    set_error("%s: %d workgroups x %zu bytes (queries of up to %d residues, lists of %d domains, %d segments, %d clusters) do not fit on the device", what, blocks, per_block, Lc, caps.dom, caps.seg, caps.clus);
    return WH_ENOMEM;
  }
  r.mx = (double *)e->d_rmx.p; r.segs = (int32_t *)e->d_bigsegs.p;
  // one segment of mixed models in the order of the list, one slot per workgroup
  std::vector<int32_t> plan((size_t)4 + blocks + 1, 0);
  plan[1] = n; plan[2] = -1;
  if (e->d_rchunks.ensure(sizeof(int32_t) * plan.size())) return WH_ENOMEM;
  int32_t *d_chunks = (int32_t *)e->d_rchunks.p;
  HIPCHK(hipMemcpyAsync(d_chunks, plan.data(), sizeof(int32_t) * plan.size(), hipMemcpyHostToDevice, c.s));
  r.chunks = d_chunks; r.n_chunks = 1; r.slots = d_chunks + 4; r.n_slots = blocks; r.cursors = d_chunks + 4 + blocks;
  r.order = src;
  HIPCHK(hipMemsetAsync(r.counter, 0, sizeof(int), c.s));
  if (int rc = reset_feedback(c, dst, dst ? q.n : 0)) return rc;
  HIPCHK(hipStreamSynchronize(c.s));     // <plan> is a local
  if (e->knobs.trace) fprintf(stderr, "[wh] %s: %d pairs, queries of up to %d residues, lists of %d domains per trace, %d segments, %d clusters: %d workgroups of %d wave(s), lds %zu, %zu KB of lists + %zu MB of matrix per wave\n",
                              what, n, Lc, caps.dom, caps.seg, caps.clus, blocks, waves, lds_total, r.seg_stride * 4 >> 10, r.mx_stride * 8 >> 20);
  const auto t0 = std::chrono::steady_clock::now();
  hipError_t err = launch_resolve(r, blocks, waves, lds_total, c.s);
  if (err != hipSuccess) { set_error("%s: resolve kernel launch failed: %s", what, hipGetErrorString(err)); return WH_EHIP; }
  (*rlaunches)++;
  if (int rc = read_feedback(c, fb)) return rc;
  note_big_counts(e, *fb);
  if (e->knobs.trace) fprintf(stderr, "[wh] %s: %.1f ms (host clock around launch + synchronize)%s\n", what,
                              std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), fb->big_pairs > 0 ? "; lists too short, once more" : "");
  return WH_OK;
}

// <fb>: what a launch over <q> reported, its big-region pairs listed in the first half of d_biglist.  They run again with lists
// sized from the counts, and once more if a list is still short; a launch reads one half of d_biglist and appends to the other.
static int big_region_pass(const ScoreCall &c, bool long_q, ResolveFeedback fb, const ListedQueue &q, int *rlaunches) {
  wh_ehmm *e = c.e;
  int32_t *src = (int32_t *)e->d_biglist.p, *dst = src + q.n;
  e->last_big[0] += std::min(fb.big_pairs, q.n);
  note_big_counts(e, fb);
  for (int again = 0; fb.big_pairs > 0; again++, std::swap(src, dst)) {
    if (again == 2) { set_error("wh_score_dev: a region's lists (%d domains, %d segments, %d clusters) were too short twice", fb.big_doms, fb.big_segs, fb.big_clus); return WH_ERANGE; }
    if (int rc = launch_listed(c, long_q, long_q ? c.Lc : c.Lmain, plan_big_regions(fb), src, std::min(fb.big_pairs, q.n), dst, q, rlaunches, &fb)) return rc;
  }
  return WH_OK;
}

// ---- the long-query pass.  The main resolver launches of a call are sized for the length cap c.Lmain; a launch lists the
// pairs of longer queries (<n_long> of them in d_longlist, the longest <longest> residues) instead of resolving them, and
// this pass runs them with the call's longest query as the cap and the per-residue arrays in HBM: first with lists of the
// default sizes (a long pair with a big region is counted and listed there like any other: under WH_NO_BIG_REGION it keeps
// WH_FLAG_TRUNC), then the big-region pass over what that launch listed, with the same kernel.
static int long_query_pass(const ScoreCall &c, int n_long, int longest, const ListedQueue &q, int *rlaunches) {
  wh_ehmm *e = c.e;
  const int n = std::min(n_long, q.n);
  e->last_long[0] += n;
  e->last_long[1] = std::max<int64_t>(e->last_long[1], longest);
  ResolveFeedback fb = {};
  if (int rc = launch_listed(c, true, c.Lc, plan_big_regions(fb), (const int32_t *)e->d_longlist.p, n, e->knobs.no_big_region ? nullptr : (int32_t *)e->d_biglist.p, q, rlaunches, &fb)) return rc;
  return big_region_pass(c, true, fb, q, rlaunches);
}

// what a launch over <q> left to the follow-up passes.  Its queue must still be in place.
static int follow_up(const ScoreCall &c, const ResolveFeedback &fb, const ListedQueue &q, int *rlaunches) {
  if (fb.big_pairs > 0 && !c.e->knobs.no_big_region) if (int rc = big_region_pass(c, false, fb, q, rlaunches)) return rc;
  if (fb.long_pairs > 0) if (int rc = long_query_pass(c, fb.long_pairs, fb.longest_query, q, rlaunches)) return rc;
  return WH_OK;
}

// one resolver launch (wh_resolve.hip, one wavefront per queued pair) over the first <n_multi> records of the queue;
// <rext>: the long-list pass, whose records keep their regions in HBM.  Pairs with a region beyond the launch's lists are
// counted in the feedback block and listed in d_biglist (unless WH_NO_BIG_REGION): the caller reads the count.
static int resolve_queue(const ScoreCall &c, int n_multi, const int32_t *rext, int64_t rext_stride, int *rlaunches) {
  wh_ehmm *e = c.e;
  hipStream_t s = c.s;
  const int Lc = c.Lmain;
  const size_t rlds = resolve_lds_bytes(Lc, e->max_M);
  ResolveArgs r = resolve_args(c, rext, rext_stride, Lc);
  const bool long_q = c.Lmain < c.Lc;      // pairs of queries beyond the cap are listed in d_longlist (long_query_pass)
  if (!e->knobs.no_big_region && e->d_biglist.ensure(2 * sizeof(int32_t) * (size_t)n_multi)) return WH_ENOMEM;
  if (long_q && e->d_longlist.ensure(sizeof(int32_t) * (size_t)n_multi)) return WH_ENOMEM;
  if (int rc = reset_feedback(c, e->knobs.no_big_region ? nullptr : (int32_t *)e->d_biglist.p, e->knobs.no_big_region ? 0 : n_multi,
                              long_q ? (int32_t *)e->d_longlist.p : nullptr, long_q ? n_multi : 0)) return rc;
  if (int rc = stats_begin(c, 256, 16, &r.stats)) return rc;
  if (r.stats) HIPCHK(hipStreamSynchronize(s));
  // ---- launch geometry: ONE workgroup of up to eight waves per CU.  Models of up to 16 cells per lane get their
  // eight float64 transition arrays staged in the workgroup's LDS (49 KB at 12 cells per lane) when that fits beside
  // the waves' blocks; the Forward sweeps of their pairs then read one array per cell from L2 instead of nine.
  int Qt = 0;
  for (auto &kv : e->by_q) if (kv.first <= 16 && (kv.first == 4 || kv.first == 8 || kv.first == 12 || kv.first == 16)) Qt = std::max(Qt, kv.first);
  const bool small_queue = n_multi < 64 * e->cu_count;        // fewer than eight pairs per wave (see order_queue)
  if (c.res_no_lds_tables || small_queue) Qt = 0;
  int waves = resolve_waves_per_cu();
  if (c.res_waves > 0) waves = std::min(waves, c.res_waves);
  if (Qt > 0 && resolve_lds_header_bytes(Qt) + (size_t)waves * rlds > kLdsBudget) {
    // fewer waves WITH the tables only while at least six fit; otherwise the tables stay in L2
    int w2 = waves;
    while (w2 > 0 && resolve_lds_header_bytes(Qt) + (size_t)w2 * rlds > kLdsBudget) w2--;
    if (w2 >= 6) waves = w2; else Qt = 0;
  }
  while (waves > 1 && resolve_lds_header_bytes(Qt) + (size_t)waves * rlds > kLdsBudget) waves--;
  const size_t lds_total = resolve_lds_header_bytes(Qt) + (size_t)waves * rlds;
  r.lds_tables = Qt;
  r.wave_lds_ints = (int)(rlds / 4);
  // ---- the order of the queue: cost keys and models from the device, sorted on the host (order_queue)
  if (e->d_rkeys.ensure(2 * sizeof(float) * (size_t)n_multi) || e->d_rorder.ensure(sizeof(int32_t) * (size_t)n_multi)) return WH_ENOMEM;
  int32_t *d_models = (int32_t *)e->d_rkeys.p + n_multi;
  hipError_t kerr = launch_resolve_keys(r.recs, n_multi, r.hmms, (float *)e->d_rkeys.p, d_models, s, rext, rext_stride);
  if (kerr != hipSuccess) { set_error("resolve key kernel launch failed: %s", hipGetErrorString(kerr)); return WH_EHIP; }
  std::vector<float> keys((size_t)n_multi);
  std::vector<int32_t> models((size_t)n_multi);
  HIPCHK(hipMemcpyAsync(keys.data(), e->d_rkeys.p, sizeof(float) * keys.size(), hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(models.data(), d_models, sizeof(int32_t) * models.size(), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const QueueOrder o = order_queue(keys, models, e->dev, small_queue, e->cu_count, waves);
  // one buffer: segments | slots | cursors
  const size_t n_seg = o.chunks.size() / 4, n_slot = o.slots.size();
  if (e->d_rchunks.ensure(sizeof(int32_t) * (4 * n_seg + n_slot + n_seg))) return WH_ENOMEM;
  int32_t *d_chunks = (int32_t *)e->d_rchunks.p, *d_slots = d_chunks + 4 * n_seg, *d_cursors = d_slots + n_slot;
  HIPCHK(hipMemcpyAsync(e->d_rorder.p, o.ord.data(), sizeof(int32_t) * o.ord.size(), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(d_chunks, o.chunks.data(), sizeof(int32_t) * o.chunks.size(), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(d_slots, o.slots.data(), sizeof(int32_t) * o.slots.size(), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(d_cursors, 0, sizeof(int32_t) * n_seg, s));
  HIPCHK(hipStreamSynchronize(s));     // the vectors of <o> are locals
  r.chunks = d_chunks; r.n_chunks = (int)n_seg;
  r.slots = d_slots; r.n_slots = (int)n_slot;
  r.cursors = d_cursors;
  r.order = (const int32_t *)e->d_rorder.p;
  int blocks = std::min(r.n_slots, e->cu_count);
  {
    // Every resident wavefront brings a slab of tens of MB, and hipMalloc costs ~40 ms per GB: a queue of a few thousand
    // pairs (the reference's example data: 8 412) spent 2.4 s allocating 55 GB for 0.12 s of work.  Unless the slabs exist
    // already, a wave gets at least four pairs.  (The cost is the driver scrubbing VRAM that another process used
    // before: on a fresh device the same allocation takes milliseconds.)
    const size_t have = std::min(e->d_rmx.cap / (r.mx_stride * sizeof(double)), e->d_rsegs.cap / std::max<size_t>(1, r.seg_stride * sizeof(int32_t))) / (size_t)waves;
    const int economy = std::max(32, n_multi / (4 * waves));
    if ((size_t)blocks > have) blocks = std::max((int)std::min<size_t>(have, (size_t)blocks), std::min(blocks, economy));
  }
  blocks = clamp_blocks(blocks, (size_t)waves * (r.mx_stride * sizeof(double) + r.seg_stride * sizeof(int32_t)), e->d_rmx, e->max_M, Lc, "resolver");
  if (blocks < 0) return WH_ENOMEM;
  if (e->d_rmx.ensure((size_t)blocks * waves * r.mx_stride * sizeof(double)) || e->d_rsegs.ensure((size_t)blocks * waves * r.seg_stride * sizeof(int32_t)))
    return WH_ENOMEM;
  r.mx = (double *)e->d_rmx.p; r.segs = (int32_t *)e->d_rsegs.p;
  if (e->knobs.trace) fprintf(stderr, "[wh] resolve: %d pairs with a multidomain region on %d models, %d workgroups of %d waves, lds %zu (float64 tables of up to %d cells per lane staged: %s), slab %zu MB per wave\n",
                              n_multi, r.n_chunks, blocks, waves, lds_total, Qt, Qt ? "yes" : "no", r.mx_stride * 8 >> 20);
  const auto t_rl0 = std::chrono::steady_clock::now();
  hipError_t err = launch_resolve(r, blocks, waves, lds_total, s);
  if (err != hipSuccess) { set_error("resolve kernel launch failed: %s", hipGetErrorString(err)); return WH_EHIP; }
  if (e->knobs.trace) {
    HIPCHK(hipStreamSynchronize(s));
    fprintf(stderr, "[wh] resolve kernel alone: %.1f ms (host clock around launch + synchronize)\n",
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_rl0).count());
  }
  (*rlaunches)++;
  e->last_resolved += n_multi;
  return r.stats ? print_resolver_stats(c, r, n_multi, blocks, waves) : WH_OK;
}

// Rounds of the float64 front end in its pair-list mode (wh_generic.hip) over the <n> pairs of <d_pairs>, each followed by a
// resolver launch of its own over the round's records, which reads the regions from the round's list in HBM and sums over
// all envelopes, and by that launch's follow-up passes.  <Lcap>: the longest query among the pairs - it sizes the slabs and
// the region lists, which hold every region a sequence of that length can have.  <first>: no kernel has scored the pairs
// (long-query scoring pass): their Forward log-odds are written too, and the residues-in-HBM instantiation serves a cap
// beyond the LDS block.  The main launch's queue is overwritten.
static int front_rounds(const ScoreCall &c, const int64_t *d_pairs, int n, int Lcap, bool first, const char *what, int *rlaunches, int64_t *done) {
  wh_ehmm *e = c.e;
  hipStream_t s = c.s;
  const bool longq = first && front_longq(e, Lcap);
  // a region is at least two rows long (the row that triggers it and a later one that ends it)
  const int ext_cap = Lcap / 2 + 2;
  const int64_t rext_stride = (int64_t)kRextInts * ext_cap;
  // rounds of as many pairs as 256 MB of region lists hold
  const int per_round = (int)std::max<int64_t>(1, std::min<int64_t>(n, ((int64_t)64 << 20) / rext_stride));
  if (e->d_rext.ensure(sizeof(int32_t) * (size_t)per_round * (size_t)rext_stride)) return WH_ENOMEM;
  if (e->d_rrecs.cap < sizeof(ResolveRec) * (size_t)per_round) {
    HIPCHK(hipStreamSynchronize(s));
    if (e->d_rrecs.ensure(sizeof(ResolveRec) * (size_t)per_round)) return WH_ENOMEM;
  }
  e->rq_cap = std::max<int64_t>(e->rq_cap, per_round);
  if (e->knobs.trace) fprintf(stderr, "[wh] %s: %d pairs, %d per round, queries of up to %d residues, up to %d regions each%s\n", what, n, per_round, Lcap, ext_cap, longq ? ", residues in HBM" : "");
  for (int t0 = 0; t0 < n; t0 += per_round) {
    const int n_round = std::min(per_round, n - t0);
    GenericArgs g = front_args(c, Lcap, longq);
    g.fwd_bits = nullptr;
    g.rcap = n_round;
    g.pair_list = d_pairs + t0; g.n_pairs = n_round;
    g.rext = (int32_t *)e->d_rext.p; g.rext_stride = rext_stride; g.ext_cap = ext_cap;
    int gblocks = 0;
    if (int rc = front_blocks(c, g, n_round, what, &gblocks)) return rc;
    HIPCHK(hipMemsetAsync(g.counter, 0, sizeof(int), s));
    hipError_t gerr = launch_generic_front(g, gblocks, generic_lds_bytes(longq ? 0 : Lcap), s, longq);
    if (gerr == hipSuccess && first) gerr = launch_long_fwd_bits((const ResolveRec *)e->d_rrecs.p, n_round, c.H, c.d_fwd_bits, c.d_detail, s);
    if (gerr != hipSuccess) { set_error("%s: front kernel launch failed: %s", what, hipGetErrorString(gerr)); return WH_EHIP; }
    // the resolver's queue is now this round's records: length and work-queue head
    const int two[2] = {n_round, 0};
    HIPCHK(hipMemcpyAsync(e->counter(kSlotResolveCount), two, sizeof two, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    if (int rc = resolve_queue(c, n_round, (const int32_t *)e->d_rext.p, rext_stride, rlaunches)) return rc;
    *done += n_round;
    if (!e->knobs.no_big_region || c.Lmain < c.Lc) {
      // (a pair with many regions can have a big one among them, or a query beyond the main launch's cap; this read-back is
      // paid by calls that have such pairs only)
      ResolveFeedback fb;
      if (int rc = read_feedback(c, &fb)) return rc;
      if (int rc = follow_up(c, fb, {(const int32_t *)e->d_rext.p, rext_stride, n_round}, rlaunches)) return rc;
    }
  }
  return WH_OK;
}

// ---- the long-list pass.  The scoring kernels keep the regions of a pair in a list of WH_MAX_ENVELOPES entries in LDS;
// HMMER has no such limit.  A pair with more regions comes out of them flagged WH_FLAG_TRUNC - and is scored
// AGAIN here: the any-size float64 front end (wh_generic.hip) with a region list in HBM that holds every region a
// sequence of this length can have, then a resolver launch of its own (front_rounds).  Costs one pass over the flags (a
// byte per pair) and one 4-byte read-back per call; the float64 kernels run only when a pair needs them.
// <n_multi>: length of the main launch's queue, whose big-region and long-query counts come back with this pass's own count
// (ONE read-back of the feedback block per call for all of them); <long_list> false: only that.
static int long_list_pass(const ScoreCall &c, int n_multi, bool long_list, int *rlaunches) {
  wh_ehmm *e = c.e;
  hipStream_t s = c.s;
  int *d_tcount = &e->d_feedback()->long_list_pairs;
  const int list_cap = (int)std::min<int64_t>(c.npairs_all, (int64_t)1 << 22);
  HIPCHK(hipMemsetAsync(d_tcount, 0, sizeof(int), s));
  if (long_list) {
    if (e->d_tlist.ensure(sizeof(int64_t) * (size_t)list_cap)) return WH_ENOMEM;
    // (a pair the resolver could not finish is not flagged: it is in the big-region list, so what is flagged here has
    // more regions than WH_MAX_ENVELOPES)
    hipError_t terr = launch_trunc_list(c.d_flags, c.npairs_all, d_tcount, (int64_t *)e->d_tlist.p, list_cap, s);
    if (terr != hipSuccess) { set_error("flag scan launch failed: %s", hipGetErrorString(terr)); return WH_EHIP; }
  }
  // the main launch's big regions and long queries first: its queue is still in place (the rounds below overwrite it)
  ResolveFeedback fb;
  if (int rc = read_feedback(c, &fb)) return rc;
  if (n_multi > 0) if (int rc = follow_up(c, fb, {nullptr, 0, n_multi}, rlaunches)) return rc;
  const int n_trunc = std::min(fb.long_list_pairs, list_cap);          // (beyond four million such pairs in one call the rest stay flagged)
  if (n_trunc <= 0) return WH_OK;
  // (the flagged pairs were scored by the main launches: none is longer than their cap)
  return front_rounds(c, (const int64_t *)e->d_tlist.p, n_trunc, c.Ls, false, "long-list pass", rlaunches, &e->last_long_list);
}

// ---- the long-query scoring pass.  The scoring launches of a call are sized for the length cap c.Ls and leave the pairs of
// longer queries alone (decibits 0, no flag); those pairs - every model of every such query - are listed on the device and
// scored here by the float64 front end and the resolver (front_rounds), one wavefront per pair: a correctness path, not a
// fast one.  Runs after every other pass of the call (it overwrites the resolver's queue).
static int long_score_pass(const ScoreCall &c, int *rlaunches) {
  wh_ehmm *e = c.e;
  hipStream_t s = c.s;
  int *d_count2 = e->counter(kSlotLongScore);
  if (e->d_lqlist.ensure(sizeof(int64_t) * (size_t)c.nq)) return WH_ENOMEM;
  HIPCHK(hipMemsetAsync(d_count2, 0, 2 * sizeof(int), s));
  hipError_t err = launch_long_queries(c.d_offsets, c.nq, c.Ls, d_count2, (int64_t *)e->d_lqlist.p, s);
  if (err != hipSuccess) { set_error("long-query scoring pass: query scan launch failed: %s", hipGetErrorString(err)); return WH_EHIP; }
  int count2[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(count2, d_count2, sizeof count2, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const int64_t n = (int64_t)count2[0] * c.H;
  if (n <= 0) return WH_OK;
  if (e->d_tlist.ensure(sizeof(int64_t) * (size_t)n)) return WH_ENOMEM;
  err = launch_long_pairs((const int64_t *)e->d_lqlist.p, count2[0], c.H, (int64_t *)e->d_tlist.p, s);
  if (err != hipSuccess) { set_error("long-query scoring pass: pair list launch failed: %s", hipGetErrorString(err)); return WH_EHIP; }
  e->last_long_score[1] = count2[1];
  const auto t0 = std::chrono::steady_clock::now();
  if (int rc = front_rounds(c, (const int64_t *)e->d_tlist.p, (int)n, std::min(c.Lc, std::max(count2[1], 1)), true, "long-query scoring pass", rlaunches, &e->last_long_score[0])) return rc;
  if (e->knobs.trace) {
    HIPCHK(hipStreamSynchronize(s));
    fprintf(stderr, "[wh] long-query scoring pass: %lld pairs of %d queries beyond %d residues (longest %d): %.1f ms (host clock, resolver rounds included)\n",
            (long long)n, count2[0], c.Ls, count2[1], std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
  return WH_OK;
}

// ---- multidomain regions: HMMER's stochastic resolver over the queue the scoring launches filled, then the long-list pass
int resolver_stage(const ScoreCall &c, bool *overflow, int *rlaunches) {
  wh_ehmm *e = c.e;
  hipStream_t s = c.s;
  int n_multi = 0;
  if (c.resolve) {
    int n_bad = 0;          // (the resolver launches of EARLIER calls: counted on the device, read at this call's first synchronisation)
    HIPCHK(hipMemcpyAsync(&n_multi, e->counter(kSlotResolveCount), sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&n_bad, &e->d_feedback()->wrong_model, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (n_bad != 0) {
      HIPCHK(hipMemsetAsync(&e->d_feedback()->wrong_model, 0, sizeof(int), s));
      set_error("resolver: %d queued pair(s) sat in a segment of another model and were NOT scored (internal error)", n_bad);
      return WH_EHIP;
    }
    e->rq_rate = std::max(e->rq_rate, (double)n_multi / (double)c.npairs_all);
    if ((int64_t)n_multi > e->rq_cap) {
      // more pairs asked for a slot than the estimate allowed: the caller repeats the scoring pass with room for all
      if (e->knobs.trace) fprintf(stderr, "[wh] resolver queue: %d pairs for %lld slots, scoring pass repeated\n", n_multi, (long long)e->rq_cap);
      e->rq_floor = n_multi;
      *overflow = true;
      return WH_OK;
    }
  }
  if (n_multi > 0) if (int rc = resolve_queue(c, n_multi, nullptr, 0, rlaunches)) return rc;
  reset_resolver_counts(e);
  const bool long_list = c.resolve && generic_lds_bytes(c.Ls) <= kLdsBudget && !e->knobs.no_long_list;
  if (long_list || (n_multi > 0 && (!e->knobs.no_big_region || c.Lmain < c.Lc))) if (int rc = long_list_pass(c, n_multi, long_list, rlaunches)) return rc;
  if (c.Ls < c.Lc) return long_score_pass(c, rlaunches);
  return WH_OK;
}
