// Host side of wh_score_dev: one call context, the plan of every launch of a scoring pass (LDS block, waves, work items,
// HBM workspace) made once before anything is launched, and the stages of a pass, each a function that returns a WH_* code.
#include "wh_host.h"

static const int kStagedMaxBatches = 1 << 15;   // staged launches: batches per scoring call (32 counters each: 4 MB)
static const int kStagedQB = 48;                // ... queries per work item

// the longest query of which the main resolver launch keeps all its waves per CU (no staged tables): the length cap of the
// main launches of a call that has a query beyond the resolver's LDS block
static int resolve_main_cap(int max_M) {
  const size_t per_wave = (kLdsBudget - resolve_lds_header_bytes(0)) / (size_t)resolve_waves_per_cu();
  int lo = 1, hi = 1 << 20;              // (resolve_lds_bytes grows with the length; the cap is a few thousand residues)
  while (lo < hi) {
    const int mid = lo + (hi - lo + 1) / 2;
    if (resolve_lds_bytes(mid, max_M) <= per_wave) lo = mid; else hi = mid - 1;
  }
  return lo;
}

static ScoreCall score_call(wh_ehmm *e, const uint8_t *d_residues, const int64_t *d_offsets, int64_t nq, int64_t total_residues, int32_t max_len,
                            int32_t *d_decibits, uint8_t *d_flags, float *d_fwd_bits, wh_pair_detail *d_detail, void *stream) {
  ScoreCall c = {e, (hipStream_t)stream, d_residues, d_offsets, nq, total_residues, max_len, d_decibits, d_flags, d_fwd_bits, d_detail};
  c.Lc = std::max(max_len, 1);
  c.H = (int)e->hmms.size();
  c.npairs_all = nq * (int64_t)c.H;
  // The resolver's LDS block holds the query and a state per residue.  A call whose longest query does not fit keeps the
  // resolver all the same: its main launches are sized for the lengths that keep their occupancy, longer queries' pairs go
  // through the long-query pass (WH_NO_LONG_QUERY: no resolver for the whole call, as it was).
  const bool fits = resolve_lds_bytes(c.Lc, e->max_M) <= kLdsBudget;
  c.Lmain = fits || e->knobs.no_long_query ? c.Lc : resolve_main_cap(e->max_M);
  c.resolve = !e->knobs.no_resolve && (fits || !e->knobs.no_long_query) && c.npairs_all < 0x7FFFFFFF;
  c.mixed = nq > 0 && total_residues > 0 && (double)max_len > 1.25 * (double)total_residues / (double)nq;
  c.wide_dense = getenv("WH_WIDE_DENSE"); c.wide_no_em_lds = getenv("WH_WIDE_NO_EM_LDS"); c.p2win_force = getenv("WH_P2WIN_FORCE");
  c.res_null2_gather = getenv("WH_RES_NULL2_GATHER"); c.res_no_lds_tables = getenv("WH_RES_NO_LDS_TABLES");
  if (const char *wv = getenv("WH_RES_WAVES")) c.res_waves = std::max(1, atoi(wv));
  // The scoring launches keep the query in LDS.  A call whose longest query a size class cannot plan sizes them for the
  // lengths every class accepts (wh_plan.h); the pairs of longer queries are scored by the long-query scoring pass, which
  // hands them to the resolver like the float64 front end does - so it needs the resolver.
  c.Ls = main_length_cap(e, c.Lc, false, c.resolve, c.p2win_force);
  return c;
}

// ------------------------------------------------------------------------------------ plans of the one-wave classes
struct StagedWaves { int wl, one, both, p2, p4; };    // floats per wave block; waves of the dense kernels (one / both orientations) and of the light ones
enum class ScoreFamily { PhaseCall, PhaseCallB, TwoQuery, FourEnvelope, PassSync, Staged, PhaseCallW };   // (W: sixteen waves, wh_score7w.o)
static const char *const kFamilyName[] = {"phase-call", "phase-call(B)", "two-queries-per-wave", "phase-call", "pass-synchronous", "staged", "phase-call(16 waves)"};

struct ScoreClassPlan {
  int Q, list_off, n_list;       // cells per lane; the class's models in d_lists
  ScoreFamily family;
  LdsPlan b;
  int Klds;                      // pass-synchronous kernel: emission rows in LDS (K) or read from L2 (0)
  bool specg;                    // special-state rows in the wave's HBM region
  int p2win;                     // multihit Backward on a node window: 0 no, 1 three more rows in LDS, 2 in place (P1's rows backed up in HBM)
  bool use_qorder;
  int QB, n_qblocks, n_items;
  size_t scratch_stride, spec_stride;
  int blocks;
  StagedWaves st;
};

static int cap_waves(const Knobs &kn, int w) { return cap_waves(kn.max_waves, w); }
static size_t score_table_bytes(const wh_ehmm *e, int Q) { return score_table_bytes(e->K, Q); }

// ---- staged launches (wh_staged.hip): a workgroup draws G work items of kStagedQB queries at a time and deals their
// candidates to its waves one by one
static const int G_all = 1, G_most = 4, G_few = 8, G_rare = 32;        // kernels that serve every pair / most / a few per cent / next to none
static int staged_cand_cap(int G, int per_pair) { return std::min(G * kStagedQB * per_pair, 2048); }
static size_t staged_lds(int Q, int wl, int arrays, int waves, int cand) {
  return lds_bytes(kLdsHeader + (size_t)cand * sizeof(int), (size_t)arrays * Q * kWave * sizeof(float), waves, wl);
}
// the LDS plans of the three kinds of staged kernel; false: the class's batch does not fit them (left to the fused kernel)
static bool plan_staged(const wh_ehmm *e, int Q, int Lc, StagedWaves *w) {
  const int K = e->K;
  const size_t tbl = (size_t)Q * kWave * sizeof(float);
  auto fit = [&](int arrays, int from, int cand, int per_cu) { return fit_waves(kLdsHeader + (size_t)cand * sizeof(int), arrays * tbl, from, w->wl, per_cu); };
  w->wl = kScoreSpecArrays * row_stride(Lc) + 32 + kRegsInts + residue_words(Lc);           // floats per wave block (plan_block1's, no extra rows)
  // dense kernels: twelve waves beside one orientation (+ the emission rows); the rare dense redo needs both
  w->one = fit(K + FW_NARR, 12, staged_cand_cap(G_few, WH_MAX_ENVELOPES), 1);
  w->both = fit(K + 2 * FW_NARR, 12, staged_cand_cap(G_rare, WH_MAX_ENVELOPES), 1);
  // light kernels: two workgroups per CU, the emission rows only
  w->p2 = fit(K, 12, staged_cand_cap(G_most, 1), 2);
  w->p4 = fit(K, 10, staged_cand_cap(G_most, WH_MAX_ENVELOPES), 2);
  return w->one >= 4 && w->both >= 4 && w->p2 >= 4 && w->p4 >= 4;
}

// The plan of one size class: kernel family, LDS block, work items, workspace per wave, resident workgroups.  Launches
// nothing and allocates nothing.  Three kernels serve a size class
// (wh_plan.h: plan_score_lds), and three opt-in schedules (WH_SCORE_KERNEL = 9, 10 / 11, 12) take the classes and batches they fit.
static int plan_score_class(const ScoreCall &c, int Q, int list_off, int n_list, ScoreClassPlan *out) {
  const wh_ehmm *e = c.e;
  const Knobs &kn = e->knobs;
  const int Lc = c.Ls;
  const int64_t nq = c.nq;
  const size_t table = score_table_bytes(e, Q);
  ScoreClassPlan p = {};
  p.Q = Q; p.list_off = list_off; p.n_list = n_list;
  ScoreLds l;
  if (!plan_score_lds(plan_knobs(e, c.p2win_force), e->K, Q, Lc, true, &l)) { set_error("query length %d with model class Q=%d does not fit in LDS", c.max_len, Q); return WH_ERANGE; }
  p.b = l.b; p.Klds = l.Klds;
  LdsPlan &b = p.b;
  const bool big = l.big, specg = l.specg, pairk = l.pairk, p2win = l.p2win, p2inpl = l.p2inpl;
  bool quadk = false;
  // ---- staged launches (wh_staged.hip): short-query batches of the one-wave classes, special states in LDS
  if ((kn.kernel == 10 || kn.kernel == 11) && !e->st_off && !big && !pairk && !specg && !kn.dbg && (Q == 8 || Q == 12 || Q == 16 || Q == 20 || Q == 24) &&
      plan_staged(e, Q, Lc, &p.st)) {
    p.family = ScoreFamily::Staged;
    b.SP = row_stride(Lc); b.wave_lds = p.st.wl;
    p.QB = kStagedQB; p.n_qblocks = (int)((nq + p.QB - 1) / p.QB); p.n_items = n_list * p.n_qblocks;
    p.scratch_stride = (size_t)(Lc + 1) * 2 * Q * kWave;          // the envelope kernel's per-wave Forward slab (as the fused kernel's)
    *out = p;
    return WH_OK;
  }
  // ---- four envelopes per Backward sweep (score_kernel7q, WH_SCORE_KERNEL=12): 16-cell models, special states in LDS
  if (kn.kernel == 12 && !big && !pairk && !specg && Q == 16) {
    const int wlq = kScoreSpecArrays * row_stride(Lc) + 128 + kRegsInts + 4 * 16 + 4 * 16 + 4 * residue_words(Lc);
    const int wq = fit_waves(kLdsHeader, table, cap_waves(kn, 12), wlq);
    if (wq >= 8) { quadk = true; b = {wq, row_stride(Lc), wlq, lds_bytes(kLdsHeader, table, wq, wlq)}; }
  }
  p.family = big ? ScoreFamily::PassSync : pairk ? ScoreFamily::TwoQuery : quadk ? ScoreFamily::FourEnvelope : kn.kernel == 8 ? ScoreFamily::PhaseCallB
             : l.four ? ScoreFamily::PhaseCallW : ScoreFamily::PhaseCall;
  p.p2win = (specg || big || pairk || quadk) ? 0 : p2win ? 1 : p2inpl ? 2 : 0;
  p.use_qorder = big || c.mixed;
  const int waves = b.waves;
  // (the phase-call kernels deal an item's queries to the waves one by one, so an item can be large - the wait at its
  // end is one pair's time whatever its size: 32 queries per wave; long models: a pair is milliseconds, smaller items
  // shorten the tail of the launch)
  p.QB = big ? waves * 2 : pairk ? waves * 4 : waves * (kn.item_g > 0 ? kn.item_g : 32);
  const int per_turn = pairk ? 2 : 1;   // queries a wave takes per turn
  // small batches (the reference's example as shipped: 500 fragments x 15 models): with the default item size there
  // are fewer than a handful of items per workgroup and the launch ends on its stragglers - one query per wave and
  // item then (the tables of a model are re-staged more often, which a small batch can afford)
  const int max_blocks = big ? e->cu_count : e->cu_count * std::max(1, 8 / waves);
  if ((int64_t)n_list * ((nq + p.QB - 1) / p.QB) < 4 * (int64_t)max_blocks) {
    // fewer items than that: smaller ones, down to one query per wave
    p.QB = waves * per_turn;
    if (!big && !pairk) for (int g_ = 16; g_ > 1; g_ /= 2)
      if ((int64_t)n_list * ((nq + waves * g_ - 1) / (waves * g_)) >= 4 * (int64_t)max_blocks) { p.QB = waves * g_; break; }
  }
  if (quadk) p.QB = std::max(p.QB, waves * 8);       // (items of two quads per wave)
  p.n_qblocks = (int)((nq + p.QB - 1) / p.QB);
  p.n_items = n_list * p.n_qblocks;
  p.scratch_stride = (size_t)(quadk ? 5 : per_turn) * (size_t)(Lc + 1) * 2 * Q * kWave;   // Forward slab(s) per wave
  p.spec_stride = specg ? (size_t)8 * b.SP : quadk ? (size_t)(5 * kScoreSpecArrays + 1) * b.SP : 0;
  p.specg = specg || quadk;                          // (the four-envelope kernel keeps an HBM region per wave too)
  p.blocks = clamp_blocks(std::min(p.n_items, max_blocks), (size_t)waves * (p.scratch_stride + p.spec_stride) * sizeof(float), e->d_scratch, e->max_M, Lc, "scoring");
  if (p.blocks < 0) return WH_ENOMEM;
  *out = p;
  return WH_OK;
}

// the kernel arguments of a planned class; <launches>: launches of this pass so far (the class's work-queue head)
static ScoreArgs class_args(const ScoreCall &c, const ScoreClassPlan &p, int launches) {
  const wh_ehmm *e = c.e;
  const Knobs &kn = e->knobs;
  ScoreArgs a;
  fill_common(a, c);
  a.tables = (const float *)e->d_tables.p;
  a.hmm_list = (const int32_t *)e->d_lists.p + p.list_off; a.n_list = p.n_list;
  a.counter = e->counter(kSlotLaunch0 + launches);
  a.dbg = kn.dbg;
  a.no_window = kn.no_window ? 1 : 0;
  a.keep_scale = kn.keep_scale;
  a.spill_band = kn.kernel != 9 ? kn.spill_band : 0;
  a.Klds = p.Klds; a.SP = p.b.SP; a.wave_lds = p.b.wave_lds; a.spec_arrays = kScoreSpecArrays;
  // (+ the layout of the block this build expects of the default scoring object, wh_score7.o: row records or arrays.  Its
  // launchers refuse the other one - an object left over from a build with other flags - as they refuse six against eight arrays)
  if (p.family == ScoreFamily::PhaseCall || p.family == ScoreFamily::PhaseCallW || p.family == ScoreFamily::FourEnvelope) a.spec_arrays |= kScoreSpecLayout << 8;
  a.paths = reinterpret_cast<unsigned long long *>(e->counter(kSlotScorePath));
  a.p2win = p.p2win;
  a.qorder = p.use_qorder ? c.d_qorder : nullptr;
  a.QB = p.QB; a.n_qblocks = p.n_qblocks; a.n_items = p.n_items;
  a.scratch_stride = p.scratch_stride; a.spec_stride = p.spec_stride;
  a.scratch = (float *)e->d_scratch.p;
  if (p.specg) a.spec_scratch = (float *)e->d_spec.p;
  return a;
}

static int print_class_stats(const ScoreCall &c, int Q, const unsigned long long *stats) {
  unsigned long long st[40];
  if (int rc = stats_read(c, stats, st)) return rc;
  const double tot = (double)(st[4] + st[5] + st[6] + st[7] + st[8] + st[9] + st[10] + st[11]);
  fprintf(stderr, "[wh] Q=%d wave cycles: P1 %.1f%%  P2 %.1f%%  regions %.1f%%  P3 %.1f%%  P4 %.1f%%  null2 %.1f%%  swaps+barriers %.1f%%  other %.1f%%  (total %.3g ticks)\n", Q, 100.0 * st[4] / tot,
          100.0 * st[5] / tot, 100.0 * st[6] / tot, 100.0 * st[7] / tot, 100.0 * st[8] / tot, 100.0 * st[9] / tot, 100.0 * st[10] / tot, 100.0 * st[11] / tot, tot);
  if (st[38]) fprintf(stderr, "[wh] Q=%d wave lifetimes %.3g cycles: %.1f%% in the phases above, %.1f%% fetching an item (two barriers)\n", Q, (double)st[38], 100.0 * tot / (double)st[38], 100.0 * (double)st[39] / (double)st[38]);
  if (st[37]) fprintf(stderr, "[wh] Q=%d four-envelope sweeps: %llu envelopes, %.0f wave cycles per envelope (slot 'null2' above)\n", Q, st[37], (double)st[9] / (double)st[37]);
  fprintf(stderr, "[wh] Q=%d envelope Backward sweeps: %llu on a 256-node window, %llu on a 512-node window, %llu windows failed the mass certificate, %llu full width; union of the stored lane blocks: span %.1f blocks (with margin), %.1f blocks set, of %llu envelopes\n", Q, st[0], st[1], st[2], st[3], (double)st[12] / (double)std::max(1ull, st[14]), (double)st[15] / (double)std::max(1ull, st[14]), st[14]);
  fprintf(stderr, "[wh] Q=%d multihit Backward on a window: %llu scans, of them in doubt at a threshold %llu, at the multidomain bound %llu; window loss out of range %llu; mean eps %.3g\n", Q,
          st[35], st[32], st[33], st[36], st[35] ? 1e-9 * (double)st[34] / (double)st[35] : 0.0);
  fprintf(stderr, "[wh] Q=%d |Ld - mass| / Ld  (<3e-7, <1e-6, <3e-6, <1e-5, <2e-5, more): window sweeps %llu %llu %llu %llu %llu %llu; full-width sweeps %llu %llu %llu %llu %llu %llu\n", Q,
          st[16], st[17], st[18], st[19], st[20], st[21], st[22], st[23], st[24], st[25], st[26], st[27]);
  return WH_OK;
}

static int launch_score_class(const ScoreCall &c, const ScoreClassPlan &p, int *launches) {
  wh_ehmm *e = c.e;
  hipStream_t s = c.s;
  const int Q = p.Q, waves = p.b.waves, threads = waves * kWave;
  const bool big = p.family == ScoreFamily::PassSync;
  ScoreArgs a = class_args(c, p, *launches);
  if (a.p2win == 2) {
    a.p2_backup_stride = (size_t)kScoreSpecArrays * a.SP;
    if (e->d_p2bak.ensure((size_t)p.blocks * waves * a.p2_backup_stride * sizeof(float))) return WH_ENOMEM;
    a.p2_backup = (float *)e->d_p2bak.p;
  }
  if (int rc = stats_begin(c, 320, 13, &a.stats)) return rc;
  if (e->knobs.trace) fprintf(stderr, "[wh] score Q=%d kernel=%s specg=%d waves=%d blocks=%d lds=%zu SP=%d wave_lds=%d items=%d Lcap=%d\n", Q,
                              kFamilyName[(int)p.family], (int)p.specg, waves, p.blocks, p.b.lds, a.SP, a.wave_lds, a.n_items, a.Lcap);
  HIPCHK(hipMemsetAsync(a.counter, 0, sizeof(int), s));
  e->last_shapes.push_back({Q, waves, a.p2win});
  if (class_mark(e, s, Q, big ? 1 : 0)) return WH_EHIP;
  hipError_t err = big ? launch_score_big(Q, a, p.blocks, threads, p.b.lds, s)
                   : p.family == ScoreFamily::TwoQuery ? launch_score9(Q, a, p.blocks, threads, p.b.lds, s)
                   : p.family == ScoreFamily::FourEnvelope ? launch_score7q(Q, a, p.blocks, threads, p.b.lds, s)
                   : p.family == ScoreFamily::PhaseCallB ? launch_score7b(Q, a, p.blocks, threads, p.b.lds, s)
                   : p.family == ScoreFamily::PhaseCallW ? launch_score7w(Q, a, p.blocks, threads, p.b.lds, s)
                                                         : launch_score7(Q, a, p.blocks, threads, p.b.lds, s);
  if (err != hipSuccess) { set_error("score kernel launch (Q=%d) failed: %s", Q, hipGetErrorString(err)); return WH_EHIP; }
  (*launches)++;
  return a.stats ? print_class_stats(c, Q, a.stats) : WH_OK;
}

static int print_staged_stats(const ScoreCall &c, int Q, const unsigned long long *stats) {
  unsigned long long st[64];
  if (int rc = stats_read(c, stats, st)) return rc;
  static const char *kind[9] = {"p1", "p2win 256", "p2win 512", "p2full", "p3", "p4win 256", "p4win 512", "p4full", "dense"};
  for (int k = 0; k < 9; k++)
    fprintf(stderr, "[wh] staged Q=%d %-10s sweeps %9llu  shader cycles per sweep %10.0f  real time per sweep %8.1f us  (clock %.2f GHz)  wave lifetimes %.3g cycles, in sweeps %.1f%%\n", Q, kind[k], st[4 * k + 3],
            st[4 * k + 3] ? (double)st[4 * k] / (double)st[4 * k + 3] : 0.0, st[4 * k + 3] ? 0.01 * (double)st[4 * k + 1] / (double)st[4 * k + 3] : 0.0,
            st[4 * k + 1] ? 0.1 * (double)st[4 * k] / (double)st[4 * k + 1] : 0.0, (double)st[4 * k + 2], st[4 * k + 2] ? 100.0 * (double)st[4 * k] / (double)st[4 * k + 2] : 0.0);
  return WH_OK;
}

// One planned size class through the staged launches (wh_staged.hip): sizes the batches from the free HBM and enqueues
// eight to ten launches per batch - nothing is read back in between: every kernel takes its work from device-side lists
// and counters.  Batches are ranges of the class's work items (model-major, a.QB queries each), so a batch holds one or
// two models' tables worth of pairs.
static int launch_staged_class(const ScoreCall &c, const ScoreClassPlan &p, int *launches) {
  wh_ehmm *e = c.e;
  hipStream_t s = c.s;
  const Knobs &kn = e->knobs;
  const bool split = kn.kernel == 11;           // 11: P3 and P4 as launches of their own too (one Forward slab per envelope of a batch)
  const int Q = p.Q, Lc = c.Ls, K = e->K, w_one = p.st.one, w_both = p.st.both, w_p2 = p.st.p2, w_p4 = p.st.p4;
  auto lds_of = [&](int arrays, int waves, int cand) { return staged_lds(Q, p.st.wl, arrays, waves, cand); };
  ScoreArgs a = class_args(c, p, *launches);
  StagedArgs g;
  memset(&g, 0, sizeof g);
  g.slab_stride = (size_t)(Lc + 1) * 2 * Q * kWave;
  g.p1stride = (size_t)kScoreSpecArrays * a.SP;
  g.p3stride = g.p1stride;
  // ---- batch size.  Full split: units (Forward slabs) from the free HBM, at most sixteen per resident dense wave; pairs =
  // units / (units per pair).  Otherwise a batch is bounded by its per-pair rows alone (3.6 KB per pair at L = 150).
  int64_t NS = split ? (int64_t)e->cu_count * w_one * 16 : (int64_t)1 << 20;
  size_t free_b = 0, total_b = 0;
  if (split && hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
    const size_t budget = (size_t)((double)(free_b + e->d_st_slabs.cap + e->d_st_p3spec.cap) * 0.45);
    NS = std::min<int64_t>(NS, (int64_t)(budget / ((g.slab_stride + g.p3stride) * sizeof(float))));
  }
  if (kn.st_units > 0) NS = kn.st_units;
  const int64_t total_pairs = (int64_t)a.n_items * a.QB;
  NS = std::min<int64_t>(NS, (int64_t)((double)total_pairs * e->st_upp) + a.QB * WH_MAX_ENVELOPES);
  if (NS < 16) { set_error("staged launches: no HBM for the Forward slabs (Q=%d, L=%d)", Q, Lc); return WH_ENOMEM; }
  const double upp = split ? e->st_upp : 1.0;
  int items_b = (int)std::max<int64_t>(1, (int64_t)((double)NS / upp) / a.QB);
  items_b = std::min(items_b, a.n_items);
  // (batches of equal size, each a multiple of the workgroup count where the class is large enough for that)
  {
    const int nb = (a.n_items + items_b - 1) / items_b;
    items_b = (a.n_items + nb - 1) / nb;
    if (items_b > 2 * e->cu_count) items_b = std::min((items_b + e->cu_count - 1) / e->cu_count * e->cu_count, (int)std::max<int64_t>(1, (int64_t)((double)NS / upp) / a.QB));
  }
  const int NB = items_b * a.QB;
  const int n_batches = (a.n_items + items_b - 1) / items_b;
  if (e->d_st_pairs.ensure(sizeof(StPair) * (size_t)NB) || e->d_st_p1spec.ensure(sizeof(float) * g.p1stride * (size_t)NB) ||
      e->d_st_cnt.ensure(sizeof(int) * 32 * (size_t)kStagedMaxBatches))
    return WH_ENOMEM;
  // (the counters of EVERY batch of the call are read back once, at its end: the block is allocated at its full size the
  // first time - growing it between two size classes of a call would drop the first class's counters)
  if (e->last_staged_batches + n_batches > kStagedMaxBatches) { set_error("staged launches: more than %d batches in one call", kStagedMaxBatches); return WH_ERANGE; }
  if (split && (e->d_st_units.ensure(sizeof(StUnit) * (size_t)NS) || e->d_st_p3spec.ensure(sizeof(float) * g.p3stride * (size_t)NS) ||
                e->d_st_slabs.ensure(sizeof(float) * g.slab_stride * (size_t)NS)))
    return WH_ENOMEM;
  g.NB = NB; g.NS = (int)NS;
  if (split) e->st_last_NB = NB;
  g.pairs = (StPair *)e->d_st_pairs.p; g.p1spec = (float *)e->d_st_p1spec.p;
  g.units = (StUnit *)e->d_st_units.p; g.p3spec = (float *)e->d_st_p3spec.p; g.slabs = (float *)e->d_st_slabs.p;
  g.pair_paths = e->path_buf; g.pair_paths16 = e->path_buf16;
  int *cnt0 = (int *)e->d_st_cnt.p + 32 * (size_t)e->last_staged_batches;
  HIPCHK(hipMemsetAsync(cnt0, 0, sizeof(int) * 32 * (size_t)n_batches, s));
  const bool w512 = Q == 16 || Q == 24;
  if (kn.trace) fprintf(stderr, "[wh] staged Q=%d: %d items of %d queries in %d batches of %d pairs, %lld units (%.1f GB of slabs), waves dense %d / both %d / p2win %d / p4win %d\n",
                        Q, a.n_items, a.QB, n_batches, NB, (long long)NS, (double)NS * g.slab_stride * 4e-9, w_one, w_both, w_p2, w_p4);
  if (class_mark(e, s, Q, 4)) return WH_EHIP;
  if (int rc = stats_begin(c, 512, -1, &a.stats)) return rc;
  const int cu = e->cu_count;
  for (int b = 0; b < n_batches; b++) {
    g.a = a;
    g.item0 = b * items_b;
    g.n_items_b = std::min(items_b, a.n_items - g.item0);
    g.cnt = cnt0 + 32 * (size_t)b;
    auto groups = [&](int G) { return (g.n_items_b + G - 1) / G; };
    hipError_t err = hipSuccess;
    auto go = [&](int G, int per_pair) { g.G = G; g.cand_cap = staged_cand_cap(G, per_pair); return err == hipSuccess; };
    if (go(G_all, 1)) err = launch_staged_p1(Q, g, std::min(groups(g.G), cu), w_one * kWave, lds_of(K + FW_NARR, w_one, g.cand_cap), s);
    if (go(G_most, 1)) err = launch_staged_p2win(Q, 4, g, std::min(groups(g.G), 2 * cu), w_p2 * kWave, lds_of(K, w_p2, g.cand_cap), s);
    if (w512 && go(G_few, 1)) err = launch_staged_p2win(Q, 8, g, std::min(groups(g.G), 2 * cu), w_p2 * kWave, lds_of(K, w_p2, g.cand_cap), s);
    if (go(G_few, 1)) err = launch_staged_p2full(Q, g, std::min(groups(g.G), cu), w_one * kWave, lds_of(K + BW_NARR, w_one, g.cand_cap), s);
    if (!split) {
      if (go(G_all, 1)) err = launch_staged_env(Q, g, std::min(groups(g.G), cu), w_both * kWave, lds_of(K + 2 * FW_NARR, w_both, g.cand_cap), s);
      if (err != hipSuccess) { set_error("staged launch (Q=%d, batch %d) failed: %s", Q, b, hipGetErrorString(err)); return WH_EHIP; }
      continue;
    }
    if (go(G_all, WH_MAX_ENVELOPES)) err = launch_staged_p3(Q, g, std::min(groups(g.G), cu), w_one * kWave, lds_of(K + FW_NARR, w_one, g.cand_cap), s);
    if (go(G_most, WH_MAX_ENVELOPES)) err = launch_staged_p4win(Q, 4, g, std::min(groups(g.G), 2 * cu), w_p4 * kWave, lds_of(K, w_p4, g.cand_cap), s);
    if (w512 && go(G_few, WH_MAX_ENVELOPES)) err = launch_staged_p4win(Q, 8, g, std::min(groups(g.G), 2 * cu), w_p4 * kWave, lds_of(K, w_p4, g.cand_cap), s);
    if (go(G_few, WH_MAX_ENVELOPES)) err = launch_staged_p4full(Q, g, std::min(groups(g.G), cu), w_one * kWave, lds_of(K + BW_NARR, w_one, g.cand_cap), s);
    if (go(G_rare, WH_MAX_ENVELOPES)) err = launch_staged_dense(Q, g, std::min(groups(g.G), cu), w_both * kWave, lds_of(K + 2 * FW_NARR, w_both, g.cand_cap), s);
    if (err == hipSuccess) err = launch_staged_assemble(g, s);
    if (err != hipSuccess) { set_error("staged launch (Q=%d, batch %d) failed: %s", Q, b, hipGetErrorString(err)); return WH_EHIP; }
  }
  e->last_staged_batches += n_batches;
  (*launches)++;
  return a.stats ? print_staged_stats(c, Q, a.stats) : WH_OK;
}

// ------------------------------------------------------------------------------------ stages of a scoring pass
// The queue of pairs with a multidomain region (finished by resolve_kernel after the scoring launches): sized by estimate
// and reset.
static int size_resolver_queue(const ScoreCall &c) {
  wh_ehmm *e = c.e;
  e->last_resolved = 0;
  if (!c.resolve) return WH_OK;
  // estimate: 5 % of the pairs (at least 65 536) or 1.25 x the largest share an earlier call on this handle queued,
  // plus every pair of the any-size float64 front end, which hands each pair with a region to the resolver; never
  // more than one record per pair.  (Synthetic family fragments queue 0.005 % of their pairs, the reference's rRNA
  // fragments 28 %: a first call on such data repeats its scoring pass once, later calls are sized by what it saw.)
  int64_t cap = std::max<int64_t>(65536, std::max<int64_t>(c.npairs_all / 20, (int64_t)(1.25 * e->rq_rate * (double)c.npairs_all) + 1024)) +
                c.nq * (int64_t)e->generic_front.size();
  cap = std::max<int64_t>(cap, (int64_t)(e->d_rrecs.cap / sizeof(ResolveRec)));   // what an earlier call allocated is free to use
  if (e->knobs.rqueue_cap > 0) cap = e->knobs.rqueue_cap;                          // test hook
  cap = std::min<int64_t>(std::max(cap, e->rq_floor), c.npairs_all);
  if (e->d_rrecs.ensure(sizeof(ResolveRec) * (size_t)cap)) return WH_ENOMEM;
  e->rq_cap = cap;
  HIPCHK(hipMemsetAsync(e->counter(kSlotResolveCount), 0, 2 * sizeof(int), c.s));    // queue length and the resolver's work-queue head
  return WH_OK;
}

// Long models run four waves in lockstep per workgroup (wh_score_big.hip): hand them the queries in
// descending length order, so that the waves of a workgroup finish their sweeps together and the longest
// pairs start first.  (One D2H copy of the offsets and a host sort; only when such a class exists.)
// ... and the phase-call kernel deals the queries of a work item to its waves in fixed turns: with lengths of
// 50-2 000 residues in one batch a wave that drew long queries keeps the eleven others waiting at the item's
// end (about 30 % of the launch on the protein workload) - same cure.  Batches of near-equal lengths (the
// headline: all 150 nt) skip the copy and the sort.
static int order_queries(ScoreCall &c) {
  wh_ehmm *e = c.e;
  const int64_t nq = c.nq;
  bool any_long = !e->wide_by_w.empty();
  for (auto &kv : e->by_q) any_long = any_long || kv.first >= 20;
  c.d_qorder = nullptr;
  if (!(any_long || c.mixed) || nq <= 4 || nq >= 0x7FFFFFFF) return WH_OK;
  std::vector<int64_t> offs((size_t)nq + 1);
  HIPCHK(hipMemcpyAsync(offs.data(), c.d_offsets, sizeof(int64_t) * offs.size(), hipMemcpyDeviceToHost, c.s));
  HIPCHK(hipStreamSynchronize(c.s));
  std::vector<int32_t> ord((size_t)nq);
  for (int64_t q = 0; q < nq; q++) ord[(size_t)q] = (int32_t)q;
  std::stable_sort(ord.begin(), ord.end(), [&](int32_t x, int32_t y) { return offs[x + 1] - offs[x] > offs[y + 1] - offs[y]; });
  if (e->d_qorder.ensure(sizeof(int32_t) * ord.size())) return WH_ENOMEM;
  HIPCHK(hipMemcpyAsync(e->d_qorder.p, ord.data(), sizeof(int32_t) * ord.size(), hipMemcpyHostToDevice, c.s));
  HIPCHK(hipStreamSynchronize(c.s));   // ord is a local
  c.d_qorder = (const int32_t *)e->d_qorder.p;
  return WH_OK;
}

// The one-wave size classes: every class is planned first, the per-wave workspace is sized from the plans and allocated
// ONCE (growing a DevBuf class by class meant a hipFree + hipMalloc of tens of GB per class: ~25 ms per GB), then the
// launches go out from the stored plans - with the workgroup counts the workspace was sized for.
static int score_size_classes(const ScoreCall &c, int *launches) {
  wh_ehmm *e = c.e;
  std::vector<ScoreClassPlan> plans;
  size_t need_scratch = 0, need_spec = 0;
  int list_off = 0;
  for (auto &kv : e->by_q) {
    const int n_list = (int)kv.second.size();
    list_off += n_list;
    if (e->force_wide && e->dev[(size_t)kv.second[0]].wideW > 0) continue;   // test hook: these models go through the wide kernel
    ScoreClassPlan p;
    if (int rc = plan_score_class(c, kv.first, list_off - n_list, n_list, &p)) return rc;
    const size_t waves = p.family == ScoreFamily::Staged ? (size_t)p.st.both : (size_t)p.b.waves;
    const size_t blocks = p.family == ScoreFamily::Staged ? (e->knobs.kernel == 11 ? 0 : (size_t)e->cu_count) : (size_t)p.blocks;   // (full split: slabs per envelope unit, not per wave)
    need_scratch = std::max(need_scratch, blocks * waves * p.scratch_stride * sizeof(float));
    if (p.specg) need_spec = std::max(need_spec, blocks * waves * p.spec_stride * sizeof(float));
    plans.push_back(p);
  }
  if (e->d_scratch.ensure(need_scratch) || (need_spec && e->d_spec.ensure(need_spec))) return WH_ENOMEM;
  for (const ScoreClassPlan &p : plans)
    if (int rc = p.family == ScoreFamily::Staged ? launch_staged_class(c, p, launches) : launch_score_class(c, p, launches)) return rc;
  return WH_OK;
}

static int print_wide_stats(const ScoreCall &c, int W, int wq, const unsigned long long *stats) {
  unsigned long long st[24];
  if (int rc = stats_read(c, stats, st)) return rc;
  for (int wv = 0; wv < 2; wv++) {
    const unsigned long long *g = st + 8 + 8 * wv;
    double rt = 0; for (int k = 0; k < 7; k++) rt += (double)g[k];
    if (rt > 0) fprintf(stderr, "[wh] wide P1 row, %s wave: cells %.1f%%  barrier0 %.1f%%  local D %.1f%%  barrier1 %.1f%%  fix-up+sum %.1f%%  barrier2 %.1f%%  specials+tail %.1f%%\n", wv ? "last" : "first",
                        100 * g[0] / rt, 100 * g[1] / rt, 100 * g[2] / rt, 100 * g[3] / rt, 100 * g[4] / rt, 100 * g[5] / rt, 100 * g[6] / rt);
  }
  const double tot = (double)st[5] > 0 ? (double)st[5] : 1.0;
  fprintf(stderr, "[wh] wide %d x %d cells per lane, cycles of the first wave: P1 %.1f%%  P2 %.1f%%  regions %.1f%%  P3 %.1f%%  P4 %.1f%%  (of %.3g)\n", W, wq,
          100.0 * st[0] / tot, 100.0 * st[1] / tot, 100.0 * st[2] / tot, 100.0 * st[3] / tot, 100.0 * st[4] / tot, tot);
  return WH_OK;
}

// floats of one workgroup's slab of the wide scoring kernel: Forward rows [row][2][Q4][NL] (+ per-row lane masks)
static size_t wide_score_stride(int Lc, int wq, int W, bool sparse) {
  const size_t st = (size_t)(Lc + 1) * 2 * wq * W * kWave + (sparse ? (size_t)(Lc + 1) * W * 2 + 4 : 0);
  return (st + 3) & ~(size_t)3;
}

// ---- models of 3 073 - 24 576 nodes: several wavefronts per pair, float32 (wh_score_wide.hip); one launch per
// waves-per-pair class.  A query batch too long for the kernel's LDS block (<wide_done> false) falls to the float64 front end.
static int score_wide_classes(const ScoreCall &c, int *launches, bool *wide_done) {
  wh_ehmm *e = c.e;
  hipStream_t s = c.s;
  const int Lc = c.Ls;
  const size_t wlds0 = wide_lds_bytes(Lc);
  *wide_done = wlds0 <= kLdsBudget;
  if (!*wide_done && e->force_wide) { set_error("WH_FORCE_WIDE: query length %d does not fit the wide kernel's LDS block", c.max_len); return WH_ERANGE; }
  if (!*wide_done) return WH_OK;
  size_t woff = e->generic_front.size();            // (the queue of the resolver was sized and reset before the one-wave launches)
  for (auto &kv : e->by_q) woff += kv.second.size();
  int wclass = 0;
  for (auto &kv : e->wide_by_w) {
    const int W = kv.first & 15, wq = kv.first >> 4;
    // 12-cell classes: the emission rows of the canonical residues go to LDS where they fit behind the block
    const size_t em_floats = (size_t)e->K * wq * W * kWave;
    const bool em_lds = (wq == kWideQReg || wq == kWideQReg2) && !c.wide_no_em_lds && wide_lds_bytes(Lc, em_floats) <= kLdsBudget;
    const size_t wlds = em_lds ? wide_lds_bytes(Lc, em_floats) : wlds0;
    WideArgs a;
    fill_common(a, c);
    a.tables = (const float *)e->d_tables.p;
    a.hmm_list = (const int32_t *)e->d_lists.p + woff; a.n_list = (int)kv.second.size();
    woff += kv.second.size();
    if (wclass >= kWideScoreClasses) { set_error("too many classes of long models"); return WH_ERANGE; }
    a.counter = e->counter(kSlotWideScore + wclass++);
    a.em_lds = em_lds ? 1 : 0;
    a.SP = row_stride(Lc);
    a.qorder = c.d_qorder;
    a.sparse = c.wide_dense ? 0 : 1;
    a.paths16 = e->path_buf16;
    a.scratch_stride = wide_score_stride(Lc, wq, W, a.sparse != 0);
    const int64_t n_items = c.nq * (int64_t)a.n_list;
    const int per_cu = (W <= 4 && 2 * wlds <= kLdsBudget) ? 2 : 1;
    int blocks = (int)std::min<int64_t>(n_items, (int64_t)e->cu_count * per_cu);
    blocks = clamp_blocks(blocks, a.scratch_stride * sizeof(float), e->d_wscratch, e->max_M, Lc, "wide scoring");
    if (blocks < 0) return WH_ENOMEM;
    if (e->d_wscratch.ensure((size_t)blocks * a.scratch_stride * sizeof(float))) return WH_ENOMEM;
    a.scratch = (float *)e->d_wscratch.p;
    HIPCHK(hipMemsetAsync(a.counter, 0, sizeof(int), s));
    if (e->knobs.trace) fprintf(stderr, "[wh] wide scoring: %lld pairs on %d models, %d waves per pair x %d cells per lane, %d workgroups, lds %zu, slab %zu MB per workgroup\n",
                                (long long)n_items, a.n_list, W, wq, blocks, wlds, a.scratch_stride * 4 >> 20);
    if (class_mark(e, s, wq * W, 3)) return WH_EHIP;
    if (int rc = stats_begin(c, 320, -1, &a.stats)) return rc;
    hipError_t werr = launch_score_wide(wq, a, blocks, W, wlds, s);
    if (werr != hipSuccess) { set_error("wide score kernel launch failed: %s", hipGetErrorString(werr)); return WH_EHIP; }
    if (a.stats) if (int rc = print_wide_stats(c, W, wq, a.stats)) return rc;
    (*launches)++;
  }
  return WH_OK;
}

// ---- models of more than 3072 nodes without wide tables (or all of them, when the wide kernel did not take the batch):
// every pair with a region goes through the resolver's queue, which also assembles its score
static int score_front_end(const ScoreCall &c, bool wide_done, int *launches) {
  wh_ehmm *e = c.e;
  if (!c.resolve || c.nq * (int64_t)e->generic.size() >= 0x7FFFFFFF) {
    set_error("models of more than %d nodes need the resolver stage (query length %d, %lld pairs)", kMaxQ * kWave, c.max_len, (long long)c.npairs_all);
    return WH_ERANGE;
  }
  GenericArgs g = front_args(c, c.Ls);
  size_t goff = 0;
  for (auto &kv : e->by_q) goff += kv.second.size();
  const size_t n_gen = wide_done ? e->generic_front.size() : e->generic.size();     // (front list and wide lists are adjacent)
  g.hmm_list = (const int32_t *)e->d_lists.p + goff; g.n_list = (int)n_gen;
  const size_t glds = generic_lds_bytes(c.Ls);
  if (glds > kLdsBudget) { set_error("query length %d does not fit the any-size kernel's LDS", c.max_len); return WH_ERANGE; }
  const int64_t n_items = c.nq * (int64_t)n_gen;
  int blocks = 0;
  if (int rc = front_blocks(c, g, n_items, "any-size front end", &blocks)) return rc;
  HIPCHK(hipMemsetAsync(g.counter, 0, sizeof(int), c.s));
  if (e->knobs.trace) fprintf(stderr, "[wh] any-size front end: %lld pairs on %zu models (up to %d nodes), %d wavefronts, slab %zu MB per wave\n",
                              (long long)n_items, n_gen, e->max_M, blocks, g.slab_stride * 8 >> 20);
  if (class_mark(e, c.s, e->max_Q, 2)) return WH_EHIP;
  hipError_t gerr = launch_generic_front(g, blocks, glds, c.s);
  if (gerr != hipSuccess) { set_error("any-size front kernel launch failed: %s", hipGetErrorString(gerr)); return WH_EHIP; }
  (*launches)++;
  return WH_OK;
}

// the staged batches' counters, once per call: units per pair (sizes the next call's batches) and the overflow flag
static int read_staged_counters(const ScoreCall &c, bool *over) {
  wh_ehmm *e = c.e;
  e->st_cnt_host.resize((size_t)32 * e->last_staged_batches);
  HIPCHK(hipMemcpyAsync(e->st_cnt_host.data(), e->d_st_cnt.p, sizeof(int) * e->st_cnt_host.size(), hipMemcpyDeviceToHost, c.s));
  HIPCHK(hipStreamSynchronize(c.s));
  int most_units = 0;
  for (int b = 0; b < e->last_staged_batches; b++) {
    *over = *over || e->st_cnt_host[(size_t)32 * b + ST_OVERFLOW] != 0;
    most_units = std::max(most_units, e->st_cnt_host[(size_t)32 * b + ST_N_UNITS]);
  }
  // (full split: the next call's batches are sized for 1.25 x the densest batch seen, never below 1.05 units per pair)
  if (!*over && most_units > 0 && e->st_last_NB > 0) e->st_upp = std::max(1.05, 1.25 * (double)most_units / (double)e->st_last_NB);
  if (!*over) return WH_OK;
  // a batch held more envelopes than it had slabs for (sixteen regions per pair are possible, batches are sized for the
  // rate seen so far): this call runs again with the fused kernel, the next ones with batches sized for what was seen
  if (e->knobs.trace) fprintf(stderr, "[wh] staged launches: a batch ran out of envelope units, the scoring pass is repeated with the fused kernel\n");
  e->st_upp = std::min<double>(WH_MAX_ENVELOPES, e->st_upp * 2.0);
  e->st_off = true;
  return WH_OK;
}

// While the scoring kernels run, the host sets up what the NEXT stage needs: the alignment kernels' per-wave slabs
// ((L+1) x 5 x Q x 64 floats per resident wave: 6 GB at L = 150, Q = 16 - a first-call hipMalloc of 0.3 s that used to
// sit between the two stages).  Bounded: skipped when it would take more than a tenth of the free HBM.
static void prefetch_align_workspace(const ScoreCall &c) {
  wh_ehmm *e = c.e;
  const size_t need = (size_t)8 * (size_t)e->cu_count * (size_t)(c.Ls + 1) * 5 * (size_t)e->by_q.rbegin()->first * kWave * sizeof(float);
  size_t free_b = 0, total_b = 0;
  if (need > e->d_ascratch.cap && hipMemGetInfo(&free_b, &total_b) == hipSuccess && need < free_b / 10) (void)e->d_ascratch.ensure(need);
}

// One scoring pass: every pair is scored.  <overflow>: the caller repeats the pass (the resolver's queue was too small,
// or a staged batch ran out of envelope units).
static int score_dev_pass(ScoreCall &c, bool *overflow) {
  wh_ehmm *e = c.e;
  hipStream_t s = c.s;
  HIPCHK(hipSetDevice(e->device));
  if (timer_begin(e, 0, s)) return WH_EHIP;
  e->cls_n = 0;
  e->last_shapes.clear();
  e->last_staged_batches = 0;
  int launches = 0;
  bool wide_done = false;
  if (c.nq > 0) {
    if ((int)e->by_q.size() > kMaxLaunches) { set_error("too many model size classes (%zu)", e->by_q.size()); return WH_ERANGE; }
    if (int rc = size_resolver_queue(c)) return rc;
    HIPCHK(hipMemsetAsync(e->counter(kSlotScorePath), 0, kScorePathInts * sizeof(int), s));
    // the 16-bit per-pair record: its address goes where the ScoreArgs kernels look for it (wh_launch.h: path_record)
    static_assert(2 * kPathRecSlot + 2 == kScorePathInts, "the record's address takes the last of the eight path counters");
    if (e->path_buf16) HIPCHK(hipMemcpyAsync(e->counter(kSlotScorePath) + 2 * kPathRecSlot, &e->path_buf16, sizeof e->path_buf16, hipMemcpyHostToDevice, s));
    if (int rc = order_queries(c)) return rc;
    if (int rc = score_size_classes(c, &launches)) return rc;
    if (!e->wide_by_w.empty()) if (int rc = score_wide_classes(c, &launches, &wide_done)) return rc;
    if (!e->generic_front.empty() || (!wide_done && !e->wide_by_w.empty() && !e->force_wide))
      if (int rc = score_front_end(c, wide_done, &launches)) return rc;
  }
  if (class_mark(e, s, 0, -1)) return WH_EHIP;        // closes the last launch's interval
  if (timer_end(e, 0, s, launches)) return WH_EHIP;
  if (e->last_staged_batches > 0) {
    bool over = false;
    if (int rc = read_staged_counters(c, &over)) return rc;
    if (over) {
      *overflow = true;
      if (timer_begin(e, 4, s) || timer_end(e, 4, s, 0)) return WH_EHIP;
      return WH_OK;
    }
  }
  if (c.nq > 0 && !e->by_q.empty()) prefetch_align_workspace(c);
  if (timer_begin(e, 4, s)) return WH_EHIP;
  int rlaunches = 0;
  if (c.nq > 0 && !e->knobs.no_resolve && e->d_rrecs.p) {
    if (int rc = resolver_stage(c, overflow, &rlaunches)) return rc;
  }
  if (timer_end(e, 4, s, rlaunches)) return WH_EHIP;
  return WH_OK;
}

extern "C" int wh_score_dev(wh_ehmm *e, const uint8_t *d_residues, const int64_t *d_offsets, int64_t nq,
                            int64_t total_residues, int32_t max_len, int32_t *d_decibits, uint8_t *d_flags,
                            float *d_fwd_bits, wh_pair_detail *d_detail, void *stream) {
  if (!e || !d_residues || !d_offsets || !d_decibits || !d_flags || nq < 0 || max_len < 0) {
    set_error("wh_score_dev: bad argument");
    return WH_EINVAL;
  }
  // One call serves fewer than 2^31 pairs (pair numbers and the resolver's queue are 32-bit).  Until round 4 a larger call
  // ran WITHOUT the multidomain resolver and said nothing - a different reported set; now it is refused: the caller feeds
  // the queries in chunks (QueryAlignmentEngine.run: 20 000 at a time, the reference's own hmmsearch chunk).
  if (nq * (int64_t)e->hmms.size() >= 0x7FFFFFFF) {
    set_error("wh_score_dev: %lld queries x %zu models is 2^31 pairs or more; score the queries in chunks", (long long)nq, e->hmms.size());
    return WH_ERANGE;
  }
  ScoreCall c = score_call(e, d_residues, d_offsets, nq, total_residues, max_len, d_decibits, d_flags, d_fwd_bits, d_detail, stream);
  // The float64 front end's slab of one wave and the wide kernel's slab of one workgroup must fit on the device (models
  // beyond the one-wave float32 kernels, long queries): otherwise the call is refused before anything is launched.  (The
  // resolver's and the long-list pass's slabs depend on what the scoring launches queue: they are checked when planned.)
  if (nq > 0 && !e->generic.empty() &&
      !one_block_fits(((generic_front_doubles(c.Ls, e->max_Q) + 1) & ~(size_t)1) * sizeof(double), e->d_rmx, e->max_M, c.Ls, "any-size front end"))
    return WH_ENOMEM;
  if (nq > 0 && !e->wide_by_w.empty()) {
    if ((int)e->wide_by_w.size() > kWideScoreClasses) { set_error("too many classes of long models (%zu)", e->wide_by_w.size()); return WH_ERANGE; }
    for (auto &kv : e->wide_by_w)
      if (wide_lds_bytes(c.Ls) <= kLdsBudget &&
          !one_block_fits(wide_score_stride(c.Ls, kv.first >> 4, kv.first & 15, !c.wide_dense) * sizeof(float), e->d_wscratch, e->max_M, c.Ls, "wide scoring"))
        return WH_ENOMEM;
  }
  // ... and one wave's float64 slab of the long-query scoring pass (gigabytes at 100 000 residues x 1 000 nodes)
  if (c.Ls < c.Lc && !one_block_fits(front_args(c, c.Lc, front_longq(e, c.Lc)).slab_stride * sizeof(double), e->d_rmx, e->max_M, c.Lc, "long-query scoring pass"))
    return WH_ENOMEM;
  // The queue of pairs with a multidomain region is sized by ESTIMATE (a per-pair record is 296 bytes; the worst case,
  // one record per pair, was 3.4 GB at the headline for a class that is 0.005 % of its pairs).  The kernels count every
  // pair that wants a slot; when the count exceeds the capacity, the queue is grown to the count and the scoring pass
  // runs once more (every pair is scored again, so the queue then holds exactly what the first pass counted).
  e->last_queue_reruns = 0;
  reset_resolver_counts(e);
  e->rq_floor = 0;
  e->st_off = false;
  // (diagnostics only: a pair the kernels leave early - an empty query, one beyond the length cap - has a record of zeros)
  if (d_detail && nq > 0) HIPCHK(hipMemsetAsync(d_detail, 0, sizeof(wh_pair_detail) * (size_t)nq * e->hmms.size(), c.s));
  bool overflow = false;
  int rc = score_dev_pass(c, &overflow);
  // (two independent reasons to repeat a pass: the resolver's queue, and a staged batch that ran out of envelope units)
  for (int again = 0; rc == WH_OK && overflow; again++) {
    if (again == 2) { set_error("wh_score_dev: the resolver's queue overflowed twice"); rc = WH_ERANGE; break; }
    e->last_queue_reruns++;
    overflow = false;
    rc = score_dev_pass(c, &overflow);
  }
  e->rq_floor = 0;
  e->st_off = false;
  return rc;
}
