// Internal header of the host side of libwitch_hip.so: what wh_api.hip (handles, options, getters, host-pointer entry
// points), wh_host_score.hip (wh_score_dev), wh_host_resolve.hip (its resolver stage), wh_host_align.hip (wh_align_dev),
// wh_host_domains.hip (wh_domains_dev), wh_host_msa.hip (wh_msa_dev), wh_host_hits.hip (wh_hits_msa_dev), wh_host_display.hip (wh_domain_display_dev), wh_host_seqtab.hip (wh_seq_table_dev) and wh_host_filter.hip (the filters) share: the handle, the d_counter slots, the
// staging of the host-pointer entry points.  No kernel file includes it.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <vector>

#include "wh_devbuf.h"
#include "wh_knobs.h"
#include "wh_launch.h"
#include "wh_plan.h"

namespace wh {
const char *last_error();
}

using namespace wh;

struct KernelTimer {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  double ms = 0.0;
  int launches = 0;
  bool pending = false;
};

// ---- d_counter: 256 ints in HBM, zeroed at load.  Every owner of a slot or range, in one place: the kernels and the
// wh_last_* getters depend on these numbers.  [60..62], [68..79], [89..95], [124..127], [144..159], [192..255]
// are free.
enum CounterSlot {
  kSlotLaunch0 = 0,         // [0..59] work-queue heads of the launches of ONE call, in launch order: the one-wave scoring
  kMaxLaunches = 60,        //   classes (wh_score_dev) or the alignment launches (wh_align_dev: both passes)
  kSlotConsensus = 63,      // work-queue head of the consensus kernel
  kSlotResolveCount = 64,   // resolver: length of the queue of pairs with a multidomain region ...
  kSlotResolveWork = 65,    // ... and the work-queue head of the resolver launch (reset together)
  kSlotGenericFront = 66,   // work-queue head of the float64 front end (main launch and long-list pass)
  kSlotGenericAlign = 67,   // ... of the float64 alignment kernel
  kSlotWideAlign = 80,      // [80..88] ... of the wide alignment launches, one per (cells per lane, waves) class
  kWideAlignClasses = 9,
  kSlotAlignStat = 96,      // [96..123] wh_align_dev: window statistics of the last call (AlignArgs::wstat), among them
  kAlignStatInts = 28,
  kSlotAlignCycles = 100,   //   [100..107] four 64-bit cycle counters (AlignArgs::wcyc)
  kSlotScorePath = 128,     // [128..143] eight 64-bit counters of the last scoring call: six paths (wh_last_score_paths),
  kScorePathInts = 16,      //   bytes of Forward rows stored, and the ADDRESS of the 16-bit per-pair record (kPathRecSlot; 0: none)
  kSlotWideScore = 160,     // [160..175] work-queue heads of the wide scoring launches, one per (cells per lane, waves) class
  kWideScoreClasses = 16,   //   (13 exist: 12 x 5..8, 16 x 7..8, 24 x 6..8, 48 x 5..8; WH_FORCE_WIDE adds smaller workgroups of one of them)
  kSlotLongScore = 176,     // [176..177] long-query scoring pass: queries beyond the main length cap, the longest of them (long_queries_kernel)
  kSlotResolveFeedback = 178, // [178..191] what the resolver launches report and the lists they append to (wh_launch.h: ResolveFeedback)
  kResolveFeedbackInts = 14,
  kCounterInts = 256
};
static_assert(kSlotLaunch0 + kMaxLaunches <= kSlotConsensus && kSlotConsensus < kSlotResolveCount && kSlotResolveWork == kSlotResolveCount + 1 &&
              kSlotResolveWork < kSlotGenericFront && kSlotGenericFront < kSlotGenericAlign && kSlotGenericAlign < kSlotWideAlign, "d_counter slots overlap");
static_assert(kSlotWideAlign + kWideAlignClasses <= kSlotAlignStat && kSlotAlignCycles >= kSlotAlignStat && kSlotAlignCycles + 8 <= kSlotAlignStat + kAlignStatInts &&
              kSlotAlignCycles % 2 == 0 && kSlotAlignStat + kAlignStatInts <= kSlotScorePath && kSlotScorePath % 2 == 0, "d_counter slots overlap");
static_assert(kSlotScorePath + kScorePathInts <= kSlotWideScore && kSlotWideScore + kWideScoreClasses <= kSlotLongScore && kSlotLongScore + 2 <= kSlotResolveFeedback &&
              kSlotResolveFeedback + kResolveFeedbackInts <= kCounterInts && kResolveFeedbackInts * sizeof(int) == sizeof(ResolveFeedback) &&
              (kSlotResolveFeedback * sizeof(int) + offsetof(ResolveFeedback, big_list)) % 8 == 0 && (kSlotResolveFeedback * sizeof(int) + offsetof(ResolveFeedback, long_list)) % 8 == 0,
              "d_counter slots overlap or leave the buffer, the resolver's feedback does not fill its range, or a list's address is not 8-byte aligned");

struct FilterState;      // private to wh_host_filter.hip
struct SeqTabState;      // private to wh_host_seqtab.hip
struct DisplayState;     // private to wh_host_display.hip

struct wh_ehmm {
  Knobs knobs;
  int device = 0;
  int alphabet = 0, K = 0, Kp = 0;
  int cu_count = 256;
  std::vector<HostHMM> hmms;
  std::vector<DevHMM> dev;          // host copy of the descriptors
  std::map<int, std::vector<int32_t>> by_q;   // Q class -> model positions
  std::vector<int32_t> generic;               // models beyond the register-resident classes (wh_generic.hip)
  std::vector<int32_t> generic_front;         // ... of them, those SCORED by the float64 front end (the others: wide_by_w)
  std::map<int, std::vector<int32_t>> wide_by_w;   // cells per lane * 16 + waves per pair -> models scored by wh_score_wide.hip (3 073 - 24 576 nodes)
  unsigned resolver_launches = 0;             // see ResolveArgs::launch_id
  int force_wide_q = 0;                       // WH_FORCE_WIDE=<4|12|16|24|48>: cells per lane of every model's wide tables (tests)
  bool force_wide = false;                    // WH_FORCE_WIDE: EVERY model is scored by the wide kernel (test hook)
  DevBuf d_wscratch;                          // Forward slabs of the wide kernel's workgroups
  DevBuf d_hmms, d_tables, d_nseq, d_index, d_lists, d_counter, d_scratch;
  DevBuf d_ascratch;                        // per-wave slabs of the alignment kernels (allocated while the scoring kernels run)
  DevBuf d_gtab, d_rrecs, d_rmx, d_rsegs;   // multidomain resolver: float64 tables, pair queue, matrix slabs, segment arrays
  int last_resolved = 0;                    // pairs the resolver finished in the last wh_score call
  int64_t last_long_list = 0;               // ... of them, pairs of the long-list pass (more than WH_MAX_ENVELOPES regions)
  DevBuf d_tlist, d_rext;                   // long-list pass: pair positions, their region lists
  int64_t last_big[4] = {0, 0, 0, 0};       // big-region pass of the last wh_score call: pairs redone, most domains of a trace, segments, clusters of a region
  ResolveFeedback feedback = {};            // host copy of the resolver's feedback as uploaded in front of a launch (here: the async copy needs no synchronisation)
  DevBuf d_biglist, d_bigsegs;              // ... queue positions of its pairs (two halves: read / written by a launch), its waves' list blocks
  int64_t last_long[2] = {0, 0};            // long-query pass of the last wh_score call: pairs redone, the longest query among them
  DevBuf d_longlist;                        // ... queue positions of its pairs
  int64_t last_long_score[2] = {0, 0};      // long-query scoring pass of the last wh_score call: pairs scored by it, the longest query among them
  int64_t last_long_align[2] = {0, 0};      // ... and the same of the last wh_align call's long-query alignment pass
  DevBuf d_lqlist;                          // long-query scoring pass: the queries beyond the main length cap (their pairs: d_tlist)
  // wh_domains_dev: Forward tau / lambda per model (NaN without the STATS line), per-domain pair and envelope length, the
  // packed envelopes with their CSR, the alignment's pair lists, columns and posteriors
  std::vector<int64_t> h_env_off;           // ... host sources of asynchronous uploads: they outlive the call
  std::vector<float> h_evp;
  DevBuf d_evp, d_dom_pair, d_dom_len, d_env_res, d_env_off, d_dom_q, d_dom_h, d_dom_cols, d_dom_pp;
  int dom_lenmodel = 0;                     // wh_set_domain_length_model: WH_LENMODEL_ENVELOPE | WH_LENMODEL_SEQUENCE
  DevBuf d_dom_seqlen;                      // ... under the latter: each domain's sequence length, the alignment's d_cfg_len
  // wh_msa_dev: widths / layout / matmap / PP_cons sums, per-residue cells, RF and PP_cons, the rows, the posterior chunk;
  // wh_msa: the alignment's columns, posteriors and pair lists
  DevBuf d_msa_lay, d_msa_res, d_msa_gc, d_msa_rows, d_msa_pprows, d_msa_ppm, d_msa_cols, d_msa_pp;
  DevBuf d_map_rows, d_map_code, d_map_cnt, d_map_off, d_map_alloff, d_map_cols, d_map_text;     // wh_msa_mapali[_dev]
  DevBuf d_hits_work, d_hits_text, d_hits_cols, d_hits_pp, d_hits_dom;     // wh_hits_msa[_dev]: scan workspace and row records, the sliced batch, wh_hits_msa's domain records
  int64_t rq_cap = 0;                       // records the queue of the current scoring call holds
  double rq_rate = 0.0;                     // largest share of queued pairs any call on this handle has seen (sizes the next queue)
  int64_t rq_floor = 0;                     // ... at least this many (set when a call overflowed its estimate; the call then runs again)
  int last_queue_reruns = 0;                // scoring passes the last wh_score call repeated because its queue overflowed (0 to 2: the resolver's queue overflowed, or a staged batch ran out of envelope units)
  // staged launches (wh_staged.hip): per-batch state in HBM
  DevBuf d_p2bak;                           // 20- / 24-cell classes: P1's per-row arrays of every resident wave while its P2 window sweep works in place
  DevBuf d_st_pairs, d_st_p1spec, d_st_units, d_st_p3spec, d_st_slabs, d_st_cnt;
  double st_upp = 1.25;                     // envelope units per pair the next call's batches are sized for (learned: 1.25 x the largest seen)
  int st_last_NB = 0;                       // pairs per batch of the last full-split class launch
  bool st_off = false;                      // a batch of the current call ran out of units: the call is repeated with the fused kernel
  int last_staged_batches = 0;              // batches the staged launches of the last scoring call went through
  std::vector<int> st_cnt_host;             // the batches' counters of the last call (read back once, at the end of the scoring pass)
  uint8_t *path_buf = nullptr;              // wh_set_path_buffer: device array [nq x H] the next scoring calls fill with WH_PATH_* bits
  uint16_t *path_buf16 = nullptr;           // wh_set_path_buffer16: the 16-bit record (its address reaches the ScoreArgs kernels that write it
                                            // through the spare slot of the path counters: kPathRecSlot, wh_launch.h)
  // staging of the host-pointer entry points: the arrays of ONE call take these in call order (Staging, below); no two
  // entry points run at once on a handle and no *_dev function reads them, so they are as many as the call with the most
  // arrays needs (wh_consensus)
  static const int kStagingSlots = 11;
  DevBuf staging[kStagingSlots];
  DevBuf d_rkeys, d_rorder, d_rchunks, d_qorder, d_order, d_items, d_recs, d_spec, d_back, d_cwj, d_cwv, d_cwn, d_crow;
  uint32_t degen[32];
  // acceleration filters (wh_host_filter.hip, which alone knows the type): tables, per-length settings, last counts; made by the first wh_filter call
  struct FilterStateDelete { void operator()(FilterState *f) const; };
  std::unique_ptr<FilterState, FilterStateDelete> filter;
  // hmmsearch --tblout (wh_host_seqtab.hip, which alone knows the type): work lists, workspaces, last status; made by the first wh_seq_expect / wh_seq_table call
  struct SeqTabStateDelete { void operator()(SeqTabState *f) const; };
  std::unique_ptr<SeqTabState, SeqTabStateDelete> seqtab;
  // hmmsearch's alignment display (wh_host_display.hip, which alone knows the type): the models' display tables, scan workspace, the host-pointer call's outputs; made by the first wh_domain_display call
  struct DisplayStateDelete { void operator()(DisplayState *f) const; };
  std::unique_ptr<DisplayState, DisplayStateDelete> display;
  bool timing = false;
  static const int kTimers = 10;
  KernelTimer timers[kTimers];              // wh_last_kernel_ms: 0 scoring, 1 topk, 2 align, 3 consensus, 4 resolver, 5 domain stage, 6 alignment assembly (wh_msa_dev), 7 --mapali mapping (wh_msa_mapali_dev), 8 hit selection (wh_hits_msa_dev), 9 alignment display (wh_domain_display_dev)
  int max_M = 0;
  int max_Q = 4;                              // largest cells-per-lane of any model (sizes the float64 slabs)
  int last_align_redo = 0;          // pairs of the last wh_align call that went through the log-space pass
  int last_align_unaligned = 0;     // ... that the any-size kernel could not align (float64 range)
  int64_t last_align_paths[4] = {0, 0, 0, 0};   // pairs of the last wh_align call: 256-node window, window rejected, no window, 512-node window
  std::vector<int64_t> last_unaligned_pairs;   // their pair numbers (wh_last_align_status)
  // timing only: one event in front of every scoring launch of the last call (+ one behind the last), its cells-per-lane class
  // and kernel family (0 phase-call, 1 pass-synchronous, 2 any-size front end): wh_last_score_launches
  std::vector<hipEvent_t> cls_ev;
  std::vector<int> cls_q, cls_kind;
  int cls_n = 0;
  // the launches of the one-wave size classes of the last scoring pass, in launch order (timing mode or not): cells per lane,
  // waves per workgroup, ScoreArgs::p2win - wh_last_score_shapes
  struct ScoreShape { int q, waves, p2win; };
  std::vector<ScoreShape> last_shapes;
  int *counter(int slot) const { return (int *)d_counter.p + slot; }      // a slot of the table above
  ResolveFeedback *d_feedback() const { return (ResolveFeedback *)counter(kSlotResolveFeedback); }
};

// ---- the host-pointer entry points (wh_score, wh_align_pp, ...): what they check and how they stage their arrays
static inline int max_query_len(const int64_t *offsets, int64_t nq) {
  int64_t m = 0;
  for (int64_t i = 0; i < nq; i++) m = std::max(m, offsets[i + 1] - offsets[i]);
  return (int)m;
}
// every residue code is below the alphabet's Kp
static inline int check_residues(int Kp, const uint8_t *residues, int64_t total) {
  for (int64_t i = 0; i < total; i++)
    if (residues[i] >= Kp) { set_error("residue code %d at position %lld is not in the alphabet", residues[i], (long long)i); return WH_EINVAL; }
  return WH_OK;
}

// The staging of one call, made on the entry point's stack: every array takes the handle's next slot (an optional array
// that is absent takes its slot too, so that an array's slot does not depend on the options, and gives null); finish()
// waits for the device and copies the outputs back.  The first failure is latched in <rc>: the arrays after it are null,
// and the entry point returns it before it launches anything.  <pad>: bytes a kernel may read beyond the array's end.
struct Staging {
  wh_ehmm *e;
  int rc = WH_OK, next = 0, nback = 0;
  struct { void *host; const void *dev; size_t bytes; } back[wh_ehmm::kStagingSlots];
  explicit Staging(wh_ehmm *handle) : e(handle) {}
  template <class T> const T *in(const T *host, size_t bytes, size_t pad = 0) { return (const T *)take((void *)host, bytes, pad, true, false); }
  template <class T> T *out(T *host, size_t bytes, size_t pad = 0) { return (T *)take(host, bytes, pad, false, true); }
  template <class T> T *inout(T *host, size_t bytes, size_t pad = 0) { return (T *)take(host, bytes, pad, true, true); }
  // <dev_rc>: what the *_dev function returned (a failure goes back as it is, without waiting for the device)
  int finish(int dev_rc) {
    if (dev_rc || rc) return dev_rc ? dev_rc : rc;
    HIPCHK(hipDeviceSynchronize());
    for (int t = 0; t < nback; t++)
      if (back[t].bytes) HIPCHK(hipMemcpy(back[t].host, back[t].dev, back[t].bytes, hipMemcpyDeviceToHost));
    return WH_OK;
  }
 private:
  void *take(void *host, size_t bytes, size_t pad, bool upload, bool download) {
    if (next >= wh_ehmm::kStagingSlots) { if (!rc) { set_error("internal error: a call stages more than %d arrays", wh_ehmm::kStagingSlots); rc = WH_EINVAL; } return nullptr; }
    DevBuf &b = e->staging[next++];
    if (!host || rc) return nullptr;
    if ((rc = b.ensure(bytes + pad))) return nullptr;
    if (upload && bytes) {
      const hipError_t err = hipMemcpy(b.p, host, bytes, hipMemcpyHostToDevice);
      if (err != hipSuccess) { set_error("hipMemcpy of %zu bytes to the device failed: %s", bytes, hipGetErrorString(err)); rc = WH_EHIP; return nullptr; }
    }
    if (download) { back[nback].host = host; back[nback].dev = b.p; back[nback].bytes = bytes; nback++; }
    return b.p;
  }
};

// one event per scoring launch (timing mode only); events are created once and reused
static inline int class_mark(wh_ehmm *e, hipStream_t s, int Q, int kind) {
  if (!e->timing) return WH_OK;
  if ((int)e->cls_ev.size() <= e->cls_n) { hipEvent_t ev; HIPCHK(hipEventCreate(&ev)); e->cls_ev.push_back(ev); e->cls_q.push_back(0); e->cls_kind.push_back(0); }
  HIPCHK(hipEventRecord(e->cls_ev[(size_t)e->cls_n], s));
  e->cls_q[(size_t)e->cls_n] = Q; e->cls_kind[(size_t)e->cls_n] = kind;
  e->cls_n++;
  return WH_OK;
}

static inline int timer_begin(wh_ehmm *e, int which, hipStream_t s) {
  KernelTimer &t = e->timers[which];
  t.pending = false; t.ms = 0.0; t.launches = 0;
  if (!e->timing) return WH_OK;
  if (!t.e0) { HIPCHK(hipEventCreate(&t.e0)); HIPCHK(hipEventCreate(&t.e1)); }
  HIPCHK(hipEventRecord(t.e0, s));
  return WH_OK;
}
static inline int timer_end(wh_ehmm *e, int which, hipStream_t s, int launches) {
  KernelTimer &t = e->timers[which];
  t.launches = launches;
  if (!e->timing) return WH_OK;
  HIPCHK(hipEventRecord(t.e1, s));
  t.pending = true;
  return WH_OK;
}

static_assert(kAlignSpecRows == kAlignSpecArrays, "wh_plan.h sizes the alignment kernel's special-state rows");

// Resident workgroups are capped so that <per_block> bytes of per-wave workspace each fit in
// about 70 % of the free HBM (the work-item counter loops tolerate fewer workgroups than CUs).
// -1 when not even ONE workgroup's workspace fits (the buffer <have> counts as free: it is given
// back first): the error names the model length, the query length cap and the figures, and the
// caller refuses the call with WH_ENOMEM before it launches anything more.
// (<M> is the longest model's node count, or for the consensus kernel (<backbone>) the backbone's column count)
static inline bool one_block_fits(size_t per_block, const DevBuf &have, int M, int Lcap, const char *what, bool backbone = false) {
  if (per_block <= have.cap) return true;
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return true;     // (the allocation itself will say)
  if (per_block <= free_b + have.cap) return true;
  set_error("%s: the workspace of one workgroup does not fit on the device (%s %d %s, queries of up to %d residues: "
            "%zu bytes per workgroup, %zu bytes free)", what, backbone ? "a backbone of" : "models of up to", M, backbone ? "columns" : "nodes",
            Lcap, per_block, free_b + have.cap);
  return false;
}
static inline int clamp_blocks(int blocks, size_t per_block, const DevBuf &have, int M, int Lcap, const char *what, bool backbone = false) {
  if (blocks < 1 || per_block == 0) return blocks;
  if ((size_t)blocks * per_block <= have.cap) return blocks;
  if (!one_block_fits(per_block, have, M, Lcap, what, backbone)) return -1;
  if (blocks == 1) return blocks;
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return blocks;
  const size_t budget = (size_t)((double)(free_b + have.cap) * 0.7);
  const size_t fit = budget / per_block;
  return (int)std::max<size_t>(1, std::min<size_t>((size_t)blocks, fit));
}

// ---- wh_score_dev: what wh_host_score.hip and wh_host_resolve.hip share
// One scoring call: what the stages of a pass share.  The environment switches are per CALL, not per handle (tests flip
// them between two calls on one handle), and read once, so that the admission check and the launches cannot disagree.
struct ScoreCall {
  wh_ehmm *e;
  hipStream_t s;
  const uint8_t *d_residues; const int64_t *d_offsets; int64_t nq, total_residues; int32_t max_len;
  int32_t *d_decibits; uint8_t *d_flags; float *d_fwd_bits; wh_pair_detail *d_detail;
  int Lc, H;
  int Ls;                        // length cap of the scoring launches (= Lc unless a class cannot plan the call's longest query: long_score_pass scores the longer queries' pairs)
  int Lmain;                     // length cap of the main resolver launches (= Lc unless the longest query exceeds the resolver's LDS block: long_query_pass)
  int64_t npairs_all;
  bool resolve;                  // multidomain regions go through the resolver's queue (else: one envelope per region)
  bool mixed;                    // query lengths differ enough for the length order to pay in the one-wave classes too
  const int32_t *d_qorder;       // queries in descending length order, when the pass formed it
  bool wide_dense, wide_no_em_lds, p2win_force, res_null2_gather, res_no_lds_tables;   // WH_WIDE_DENSE ... WH_RES_NO_LDS_TABLES
  int res_waves;                 // WH_RES_WAVES (experiments: waves per resolver workgroup), 0 = not set
};

// multidomain regions: HMMER's stochastic resolver over the queue the scoring launches filled, then its follow-up passes
// (wh_host_resolve.hip).  <overflow>: the queue was too small, the caller repeats the scoring pass
int resolver_stage(const ScoreCall &c, bool *overflow, int *rlaunches);
// the follow-up passes' counters of the last call: reset when a call starts and when a pass starts over
static inline void reset_resolver_counts(wh_ehmm *e) {
  e->last_long_list = 0;
  for (int64_t &v : e->last_big) v = 0;
  e->last_long[0] = e->last_long[1] = 0;
  e->last_long_score[0] = e->last_long_score[1] = 0;
}

// what of the handle decides the LDS plans (wh_plan.h)
static inline PlanKnobs plan_knobs(const wh_ehmm *e, bool p2win_force = false) {
  const Knobs &k = e->knobs;
  PlanKnobs pk;
  pk.kernel = k.kernel; pk.max_waves = k.max_waves; pk.force_specg = k.force_specg; pk.no_window = k.no_window; pk.no_p2win = k.no_p2win; pk.p2win_force = p2win_force;
  return pk;
}
static inline PlanClasses plan_classes(const wh_ehmm *e) {
  PlanClasses cl;
  cl.K = e->K;
  for (auto &kv : e->by_q) {
    cl.align_q.push_back(kv.first);
    if (!(e->force_wide && e->dev[(size_t)kv.second[0]].wideW > 0)) cl.score_q.push_back(kv.first);   // (test hook: these models go through the wide kernel)
  }
  cl.wide = !e->wide_by_w.empty(); cl.force_wide = e->force_wide; cl.front = !e->generic_front.empty();
  return cl;
}
// the main length cap of a scoring (alignment) call with the longest query <Lc>; <can_pass>: the call has what the long-query
// pass needs, else - and under WH_NO_LONG_SCORE - the cap is Lc and the planner refuses what does not fit
static inline int main_length_cap(const wh_ehmm *e, int Lc, bool align, bool can_pass, bool p2win_force = false) {
  if (!can_pass || e->knobs.no_long_score) return Lc;
  const PlanKnobs pk = plan_knobs(e, p2win_force);
  const PlanClasses cl = plan_classes(e);
  const int cap = align ? align_main_cap(pk, cl, Lc) : score_main_cap(pk, cl, Lc);
  return e->knobs.score_lmain > 0 ? std::max(1, std::min(cap, e->knobs.score_lmain)) : cap;
}

// the fields ScoreArgs, WideArgs and GenericArgs have in common: models, queries, outputs, alphabet, resolver queue
template <class Args> static void fill_common(Args &a, const ScoreCall &c) {
  const wh_ehmm *e = c.e;
  memset(&a, 0, sizeof a);
  a.hmms = (const DevHMM *)e->d_hmms.p;
  a.residues = c.d_residues; a.offsets = c.d_offsets; a.nq = c.nq;
  a.Lcap = c.Ls;
  a.decibits = c.d_decibits; a.flags = c.d_flags; a.fwd_bits = c.d_fwd_bits; a.detail = c.d_detail;
  a.H = c.H; a.K = e->K; a.Kp = e->Kp;
  memcpy(a.degen, e->degen, sizeof a.degen);
  if (c.resolve) { a.rrecs = (ResolveRec *)e->d_rrecs.p; a.rcount = e->counter(kSlotResolveCount); a.rcap = (int)e->rq_cap; }
}

// WH_STATS: a kernel's counter block (in d_recs), zeroed before its launch; <min_slot>: a 64-bit slot that starts at ~0
static inline int stats_begin(const ScoreCall &c, size_t bytes, int min_slot, unsigned long long **stats) {
  if (!c.e->knobs.stats) return WH_OK;
  if (c.e->d_recs.ensure(bytes)) return WH_ENOMEM;
  HIPCHK(hipMemsetAsync(c.e->d_recs.p, 0, bytes, c.s));
  if (min_slot >= 0) { unsigned long long bigv = ~0ull; HIPCHK(hipMemcpyAsync((char *)c.e->d_recs.p + min_slot * 8, &bigv, 8, hipMemcpyHostToDevice, c.s)); }
  *stats = (unsigned long long *)c.e->d_recs.p;
  return WH_OK;
}
template <int N> static int stats_read(const ScoreCall &c, const unsigned long long *stats, unsigned long long (&st)[N]) {
  HIPCHK(hipMemcpyAsync(st, stats, sizeof st, hipMemcpyDeviceToHost, c.s));
  HIPCHK(hipStreamSynchronize(c.s));
  return WH_OK;
}

// The float64 front end (wh_generic.hip), one wavefront per pair: its arguments but for the work list (models of the
// main launch, pairs of the long-list pass), and the wavefronts of a launch over <n_items> with their slabs in d_rmx.
// <Lcap>: the launch's length cap, which sizes the slab; <longq>: the residues behind it (generic_front_long_kernel)
static inline bool front_longq(const wh_ehmm *e, int Lcap) { return e->knobs.longq_force || generic_lds_bytes(Lcap) > kLdsBudget; }
static inline GenericArgs front_args(const ScoreCall &c, int Lcap, bool longq = false) {
  GenericArgs g;
  fill_common(g, c);
  g.Lcap = Lcap;
  g.gtab = (const double *)c.e->d_gtab.p;
  g.counter = c.e->counter(kSlotGenericFront);
  g.Qmax = c.e->max_Q;
  g.paths16 = c.e->path_buf16;
  g.slab_stride = (generic_front_doubles(Lcap, c.e->max_Q) + 1) & ~(size_t)1;
  if (longq) g.slab_stride += generic_seq_doubles(Lcap);
  return g;
}
static inline int front_blocks(const ScoreCall &c, GenericArgs &g, int64_t n_items, const char *what, int *blocks) {
  wh_ehmm *e = c.e;
  *blocks = (int)std::min<int64_t>(n_items, (int64_t)e->cu_count * std::min<size_t>(12, kLdsBudget / std::min(generic_lds_bytes(g.Lcap), kLdsBudget)));
  *blocks = clamp_blocks(*blocks, g.slab_stride * sizeof(double), e->d_rmx, e->max_M, g.Lcap, what);
  if (*blocks < 0) return WH_ENOMEM;
  if (e->d_rmx.ensure((size_t)*blocks * g.slab_stride * sizeof(double))) return WH_ENOMEM;
  g.slab = (double *)e->d_rmx.p;
  return WH_OK;
}
