// Kernel argument blocks and launcher prototypes (host <-> device glue).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "wh_common.h"

namespace wh {

// A pair with a multidomain region, handed from the scoring kernels to resolve_kernel (wh_resolve.hip)
struct ResolveRec {
  int64_t q;
  int32_t h;
  float fwdsc;                 // float32 multihit Forward score of the whole sequence (nats)
  float fwd_bits;
  int32_t nreg;                // regions found; the first nenv are stored
  int32_t nenv;
  int32_t flags;               // WH_FLAG_* collected so far
  int32_t multi_mask;          // bit e: stored region e is multidomain
  int32_t ri[WH_MAX_ENVELOPES], rj[WH_MAX_ENVELOPES];
  float envsc[WH_MAX_ENVELOPES], domcorr[WH_MAX_ENVELOPES];   // single-domain regions: scored by the scoring kernel
};

struct ScoreArgs {
  const DevHMM *hmms;          // all models of the eHMM
  const float *tables;         // table buffer (fw / bw / em arrays of every model)
  const int32_t *hmm_list;     // model positions of this size class
  int n_list;
  const uint8_t *residues;
  const int64_t *offsets;
  int64_t nq;
  int QB;                      // queries per work item
  int n_qblocks;
  int n_items;                 // n_list * n_qblocks
  int *counter;                // work-queue head (zeroed by a memset node before the launch)
  int Lcap;                    // longest query of the batch
  int SP;                      // stride of the per-row special-state arrays (>= Lcap+1)
  int wave_lds;                // floats of LDS per wave
  int spec_arrays;             // per-row special-state arrays in that block the PLANNER assumed (the launcher refuses a mismatch with its build)
  float *scratch;              // per-wave Forward slabs
  size_t scratch_stride;       // floats per wave
  int32_t *decibits;
  uint8_t *flags;
  float *fwd_bits;
  wh_pair_detail *detail;
  float *spec_scratch;         // long-query mode: per-wave special-state rows in HBM (else NULL -> LDS)
  size_t spec_stride;          // floats per wave
  int H;
  int K, Kp;
  uint32_t degen[32];
  int Klds;                    // emission rows staged in LDS (= K, or 0: read from L2)
  int no_window;               // 1: envelope Backward sweeps at full width only (WH_NO_WINDOW)
  int p2win;                   // 1: the wave blocks hold three more per-row arrays and the multihit Backward sweep tries a node window first;
                               // 2: no room for them (20- / 24-cell models): the window sweep works IN PLACE on the block, after P1's rows
                               //    were copied to <p2_backup> (a doubtful scan brings them back for the full-width sweep)
  float *p2_backup;            // p2win == 2: per resident wave spec_arrays x SP floats
  size_t p2_backup_stride;     // floats per wave
  int dbg;                     // timing experiments only: 1 = skip Forward-row stores, 2 = skip Forward-row loads
  float keep_scale;            // Forward-row spill threshold relative to E(row); 0 = the kernel's default (2^-24)
  int spill_band;              // 1: an envelope's Forward sweep stores only the lane blocks around P1's dominant path (spill_band, wh_score7.hip)
  ResolveRec *rrecs;           // queue of pairs with a multidomain region (NULL: such regions become one envelope)
  int *rcount;                 // queue length (device counter)
  int rcap;
  unsigned long long *stats;   // WH_STATS: [4..11] wave cycles per phase (or NULL)
  unsigned long long *paths;   // 6 counters (always counted, one atomic per wave and counter at the end of the launch): envelope Backward
                               // sweeps on a 256-node window, on a 512-node window, windows that failed the certificate, full-width sweeps;
                               // multihit Backward sweeps kept from a node window, windows whose region scan was in doubt (redone at full width);
                               // [6] bytes of Forward rows stored; [kPathRecSlot] the ADDRESS of the 16-bit per-pair record (path_record below)
  const int32_t *qorder;       // long-model kernel: queries in descending length order (or NULL: input order)
};

// The 16-bit per-pair record (wh_set_path_buffer16: [nq x H] WH_PATH_* bits, or none): a kernel that takes ScoreArgs finds its
// address in the last of the eight path counters, which the host writes after zeroing them (score_dev_pass) - memory the
// kernel addresses anyway.  As one more kernel argument the pointer would cost the main launch scratch, like the
// resolver's feedback fields did (ResolveArgs::fb).  Wave-uniform: NULL = branch around the record.  (score_kernel7 reads it
// where a pair's result is stored and the pass-synchronous kernel once per wave.)
constexpr int kPathRecSlot = 7;
__device__ __forceinline__ uint16_t *path_record(const ScoreArgs &a) {
  if (!a.paths) return nullptr;
  const unsigned long long v = a.paths[kPathRecSlot];
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
  return reinterpret_cast<uint16_t *>(((unsigned long long)hi << 32) | lo);
}

// ---- staged scoring launches (wh_staged.hip): the five sweeps of a pair as kernels of their own, each at the
// occupancy it can use, over batches of pairs whose intermediate results live in HBM.
enum { ST_CLS_NONE = 0, ST_CLS_FULL = 1, ST_CLS_DENSE = 2, ST_CLS_W256 = 4, ST_CLS_W512 = 8 };   // what an envelope still needs
// Per pair of a batch:
struct StPair {
  float xC; int32_t ef;              // P1: C(L) and its scale exponent (the multihit Forward score)
  uint32_t um_lo, um_hi;             // P1: lane blocks the dominant alignment runs through (places the window of P2)
  uint32_t um_steady;                // P1: range of the steady blocks among them (the envelopes' band; forward_sweep, wh_device.h)
  int32_t state;                     // 0 nothing to do (empty / too long / no Forward mass: result written by P1), 1 P1 done,
                                     // 2 regions known, 3 the windowed region scan was in doubt (full-width P2 follows),
                                     // 4 the window of P2 needs 512 nodes
  int32_t nenv, nreg, flags;         // regions: flags = WH_FLAG_* | multidomain mask << 8
  int32_t path;                      // WH_PATH_* bits of the pair (wh_set_path_buffer, wh_set_path_buffer16); kStWantedWindow: internal
  int32_t pad[3];
  int32_t regs[2 * WH_MAX_ENVELOPES];
  float envsc[WH_MAX_ENVELOPES], domcorr[WH_MAX_ENVELOPES];
  int32_t uid[WH_MAX_ENVELOPES];     // per envelope: its unit (Forward slab) in the batch
  uint8_t cls[WH_MAX_ENVELOPES];     // per envelope: ST_CLS_* - the Backward sweep it still needs
};
// Per envelope unit of a batch (one Forward slab each):
struct StUnit {
  float xC; int32_t ef;              // P3: unihit Forward of the envelope
  int32_t m0, pad;                   // first reversed node of the window P4 runs on
};
enum { ST_C_P1 = 0, ST_C_P2, ST_C_P2W8, ST_C_P2B, ST_C_P3, ST_N_UNITS, ST_C_256, ST_C_512, ST_C_FULL, ST_C_DENSE, ST_OVERFLOW, ST_NCOUNT };
struct StagedArgs {
  ScoreArgs a;                       // the class launch (tables, queries, outputs, items) as the fused kernel gets it
  int item0, n_items_b;              // this batch: work items [item0, item0 + n_items_b) of the class launch
  int NB;                            // pairs per batch = n_items_b * QB (per-pair arrays are indexed inside the batch)
  int NS;                            // envelope units (Forward slabs) a batch may use
  int G;                             // work items a workgroup draws at a time in THIS launch
  int cand_cap;                      // entries of the workgroup's candidate list in LDS (behind the wave blocks)
  StPair *pairs;
  float *p1spec; size_t p1stride;    // per pair: P1's six per-row arrays (floats per pair)
  StUnit *units;
  float *p3spec; size_t p3stride;    // per unit: P3's six per-row arrays
  float *slabs; size_t slab_stride;  // per unit: Forward rows (floats per unit)
  int *cnt;                          // ST_NCOUNT counters of the batch (zeroed before its first launch)
  uint8_t *pair_paths;               // optional [nq x H]: WH_PATH_* bits per pair (or NULL)
  uint16_t *pair_paths16;            // optional [nq x H]: the 16-bit record (or NULL); each buffer is written where it is set
};
constexpr int kStWantedWindow = 1 << 16;   // StPair::path: P2 wanted a window and none fitted (counted as the fused kernel counts it; never stored)
// <threads> = 64 x waves; <lds> covers the header, the tables of the kind, the wave blocks and the candidate list
hipError_t launch_staged_p1(int Q, const StagedArgs &a, int blocks, int threads, size_t lds, hipStream_t s);
hipError_t launch_staged_p2win(int Q, int QB, const StagedArgs &a, int blocks, int threads, size_t lds, hipStream_t s);
hipError_t launch_staged_p2full(int Q, const StagedArgs &a, int blocks, int threads, size_t lds, hipStream_t s);
hipError_t launch_staged_p3(int Q, const StagedArgs &a, int blocks, int threads, size_t lds, hipStream_t s);
hipError_t launch_staged_p4win(int Q, int QB, const StagedArgs &a, int blocks, int threads, size_t lds, hipStream_t s);
hipError_t launch_staged_p4full(int Q, const StagedArgs &a, int blocks, int threads, size_t lds, hipStream_t s);
hipError_t launch_staged_dense(int Q, const StagedArgs &a, int blocks, int threads, size_t lds, hipStream_t s);
hipError_t launch_staged_env(int Q, const StagedArgs &a, int blocks, int threads, size_t lds, hipStream_t s);
hipError_t launch_staged_assemble(const StagedArgs &a, hipStream_t s);

hipError_t launch_score_big(int Q, const ScoreArgs &a, int blocks, int threads, size_t lds, hipStream_t s);
hipError_t launch_score7(int Q, const ScoreArgs &a, int blocks, int threads, size_t lds, hipStream_t s);
hipError_t launch_score7b(int Q, const ScoreArgs &a, int blocks, int threads, size_t lds, hipStream_t s);   // A/B slot
// sixteen waves per workgroup (wh_score7w.o): threads == 1024, Q = 8 / 12 / 16, rows in LDS; ScoreArgs::p2win is 0 or 2
hipError_t launch_score7w(int Q, const ScoreArgs &a, int blocks, int threads, size_t lds, hipStream_t s);
hipError_t launch_score7q(int Q, const ScoreArgs &a, int blocks, int threads, size_t lds, hipStream_t s);   // four envelopes per Backward sweep (Q = 16)
// two queries per wavefront (wh_score9.hip): ScoreArgs::wave_lds = 2 x score9_block_floats(SP, Lcap), scratch_stride = two slabs
hipError_t launch_score9(int Q, const ScoreArgs &a, int blocks, int threads, size_t lds, hipStream_t s);
int score9_block_floats(int SP, int Lcap);

// What the resolver kernels report back to the host and what the host tells a launch about its lists: one block of the
// handle's counters (wh_host.h: kSlotResolveFeedback), reached through ResolveArgs::fb.
struct ResolveFeedback {
  int wrong_model;             // queue records found in a segment of another model (never, for a well-formed segment list): NOT reset by an upload
  int long_list_pairs;         // pairs flagged WH_FLAG_TRUNC after the resolver (trunc_list_kernel)
  // ---- from here on the host uploads the block in front of every launch: counts zeroed, the launch's lists
  // Regions whose lists do not fit the wave's blocks (wh_resolve.hip):
  int big_pairs, big_doms, big_segs, big_clus;   // pairs that have one; the most domains of a trace, segments and significant clusters such a region needs (0: that list was long enough)
  // Pairs whose query is longer than ResolveArgs::Lcap:
  int long_pairs, longest_query;
  int big_cap;                 // capacity of the list of the big-region pairs' queue positions (0: none - the pair keeps WH_FLAG_TRUNC, WH_NO_BIG_REGION)
  int long_cap;                // ... of the long-query pairs' (0: none - the pair keeps WH_FLAG_TRUNC)
  int32_t *big_list, *long_list;
};
constexpr size_t kFeedbackUploadFrom = offsetof(ResolveFeedback, big_pairs);

struct ResolveArgs {
  const DevHMM *hmms;
  const double *gtab;          // float64 tables of every model (DevHMM::gfw_off / gem_off)
  const float *ftab;           // float32 table buffer (DevHMM::emn_off: node-major emission odds)
  const uint8_t *residues;
  const int64_t *offsets;
  const ResolveRec *recs;
  const int32_t *order;        // queue positions in processing order (model by model, longest pairs first inside a model), or NULL
  const int32_t *chunks;       // the queue's segments, one per model: (first entry of <order>, entries, model position, cells per lane) x n_chunks
  int n_chunks;
  const int32_t *slots;        // what a workgroup draws: segment numbers, a model's in proportion to its share of the work
  int n_slots;
  int *cursors;                // per segment: next entry to hand out (zeroed before the launch)
  int lds_tables;              // > 0: a chunk's model of up to this many cells per lane has its float64 transition arrays staged in LDS
  int wave_lds_ints;           // 4-byte units of LDS per wave
  const int *count;            // number of queued pairs (device)
  int rec_cap;
  int *counter;                // work-queue head (chunks)
  int Lcap, Mmax;
  double *mx;                  // per-wave matrix slabs
  size_t mx_stride;            // doubles per wave
  size_t dc_off;               // offset (doubles, even) of the walk's threshold-line cache inside a wave's slab
  unsigned launch_id;          // differs from launch to launch of a handle: part of the cache's validation bits (the slabs persist)
  int null2_gather;            // WH_RES_NULL2_GATHER (environment, per call): null2 by trace from one table row per residue (the pre-round-4 path)
  int32_t *segs;               // per-wave segment arrays
  size_t seg_stride;           // ints per wave
  int seg_cap;
  int32_t *decibits;
  uint8_t *flags;
  wh_pair_detail *detail;
  int H, K, Kp;
  uint32_t degen[32];
  unsigned long long *stats;   // WH_STATS: wave cycles per phase [0] region Forward [1] traces [2] clustering [3] cluster statistics [4] envelope Forward
  int dbg;                     // WH_RDBG > 0: print the first <dbg> sampled segments and the cluster statistics of every region
  ResolveFeedback *fb;         // device: what the launch reports (wrong_model: the host turns it into WH_EHIP) and the lists it appends to.  ONE
                               // pointer, read from memory where a pair needs it: as kernel arguments of their own the fields cost the main launch scratch
  const int32_t *rext;         // long-list pass (wh_api.hip): record t's regions are NOT in the record but here, at rext + t * rext_stride:
  int64_t rext_stride;         // kRextInts ints per region (first row, last row, envsc bits, domcorr bits, multidomain), ResolveRec::nenv of them
  int dom_cap, clus_cap;       // > 0: the big-region pass (resolve_big_kernel) - every list of a region in the wave's HBM block, seg_cap segments,
                               // seg_stride >= resolve_big_seg_ints(...)
  int long_query;              // 1 (with dom_cap > 0): the long-query pass (resolve_long_kernel) - residues and emitting states in the wave's HBM
                               // block as well, seg_stride >= resolve_long_seg_ints(...), wave_lds_ints = resolve_long_lds_bytes(Mmax) / 4
};
constexpr int kRextInts = 5;
hipError_t launch_resolve(const ResolveArgs &a, int blocks, int waves, size_t lds, hipStream_t s);
size_t resolve_lds_header_bytes(int Qt);
// cost estimate of every queued pair (cells of its multidomain regions) for the longest-first order
hipError_t launch_resolve_keys(const ResolveRec *recs, int n, const DevHMM *hmms, float *keys, int32_t *models, hipStream_t s,
                               const int32_t *rext = nullptr, int64_t rext_stride = 0);
size_t resolve_lds_bytes(int Lcap, int Mmax);
int resolve_seg_cap();
int resolve_waves_per_cu();
size_t resolve_seg_ints(int Lcap, int Mmax);
size_t resolve_big_seg_ints(int Lcap, int Mmax, int dom_cap, int seg_cap, int clus_cap);
size_t resolve_long_seg_ints(int Lcap, int Mmax, int dom_cap, int seg_cap, int clus_cap);
size_t resolve_long_lds_bytes(int Mmax);
int resolve_dom_max();
int resolve_clus_max();
size_t resolve_dcache_doubles();
size_t resolve_tail_row_doubles();

// models of any size (wh_generic.hip)
// several wavefronts per pair (wh_score_wide.hip): models of 3 073 - 24 576 nodes (scoring), 3 073 - 12 288 (alignment)
struct WideArgs {
  const DevHMM *hmms;
  const float *tables;
  const int32_t *hmm_list;     // model positions of this launch (all with the same wideW)
  int n_list;
  const uint8_t *residues;
  const int64_t *offsets;
  int64_t nq;
  int *counter;
  int Lcap, SP;
  float *scratch;              // per-workgroup Forward slabs
  size_t scratch_stride;       // floats per workgroup
  int32_t *decibits;
  uint8_t *flags;
  float *fwd_bits;
  wh_pair_detail *detail;
  int H, K, Kp;
  uint32_t degen[32];
  ResolveRec *rrecs;
  int *rcount;
  int rcap;
  const int32_t *qorder;
  int em_lds;                  // 12-cell kernels: the emission rows of the canonical residues are staged in LDS (behind the block)
  unsigned long long *stats;   // WH_STATS: [0..4] cycles of the first wave in P1, P2, region scan, P3, P4; [5] whole items (or NULL)
  int sparse;                  // envelope Forward rows: only the lanes above 2^-24 of the row's E are stored (+ masks behind the slab)
  uint16_t *paths16;           // optional [nq x H]: the 16-bit per-pair record (wh_set_path_buffer16), or NULL
};
// The PP output inside the PP kernels: a float array or a double array (wh_align_pp64) behind one word, bit 0 = "doubles".
// A type of its own: nothing but put() can index it.
struct PPOut {
  uintptr_t u = 0;
  PPOut() = default;
#if defined(__HIPCC__)
  __device__ __forceinline__ PPOut(float *p32, double *p64, int64_t off)
      : u(p64 ? (reinterpret_cast<uintptr_t>(p64 + off) | 1) : reinterpret_cast<uintptr_t>(p32 + off)) {}
  template <class T>
  __device__ __forceinline__ void put(int64_t i, T v) const {
    if (u & 1) reinterpret_cast<double *>(u & ~(uintptr_t)1)[i] = (double)v;
    else reinterpret_cast<float *>(u)[i] = (float)v;
  }
#endif
};
struct WideAlignArgs {
  const DevHMM *hmms;
  const float *tables;
  const uint8_t *residues;
  const int64_t *offsets;
  const int32_t *items;        // pair indices served by this launch (models with the same wideW)
  int n_items;
  const int64_t *pair_q;
  const int32_t *pair_h;
  const int64_t *col_off;
  int32_t *cols;
  int32_t *status;             // per pair: set to 1 when the pair left float32 range (the float64 kernel then redoes it)
  int *counter;
  int Lcap, SP;
  float *scratch;              // per workgroup: Forward/posterior rows, then OA rows
  size_t scratch_stride;       // floats per workgroup
  int K, Kp;
  // (last: the fields above keep the offsets they have without it)
  float *pp;                   // optional, CSR like <cols>: posterior probability of each residue's state on the path (wh_align_pp), or NULL
  double *pp64;                // ... or the same as doubles (wh_align_pp64); at most one of the two is set
  const int32_t *cfg_len;      // optional, per query: the length the pair's length model is configured for (wh_align_pp_len); NULL: the query's own
};
size_t wide_align_lds_bytes(int Lcap);
hipError_t launch_align_wide(int Q, const WideAlignArgs &a, int blocks, int waves, size_t lds, hipStream_t s);
size_t wide_lds_bytes(int Lcap, size_t em_floats = 0);
hipError_t launch_score_wide(int Q, const WideArgs &a, int blocks, int waves, size_t lds, hipStream_t s);

struct GenericArgs {
  const DevHMM *hmms;
  const double *gtab;
  const int32_t *hmm_list;     // model positions served by the generic kernels
  int n_list;
  const uint8_t *residues;
  const int64_t *offsets;
  int64_t nq;
  int *counter;                // work-queue head
  int Lcap, Qmax;
  double *slab;                // per-wave workspace
  size_t slab_stride;          // doubles per wave
  int32_t *decibits;
  uint8_t *flags;
  float *fwd_bits;
  wh_pair_detail *detail;
  int H, K, Kp;
  uint32_t degen[32];
  ResolveRec *rrecs;           // EVERY pair with a region is finished by resolve_kernel
  int *rcount;
  int rcap;
  // long-list pass: the pairs whose region list did not fit WH_MAX_ENVELOPES in the kernel that scored them (WH_FLAG_TRUNC)
  // are scored again here with a region list in HBM.  Work item t = pair_list[t] (q * H + h), its record is rrecs[t] and its
  // regions are rext + t * rext_stride (kRextInts ints each, up to ext_cap of them).  NULL: the hmm_list x nq mode above.
  const int64_t *pair_list;
  int64_t n_pairs;
  int32_t *rext;
  int64_t rext_stride;
  int ext_cap;
  uint16_t *paths16;           // optional [nq x H]: the 16-bit per-pair record (wh_set_path_buffer16), or NULL
};
// pairs flagged WH_FLAG_TRUNC, appended to <list> (up to <cap>; <count> keeps counting)
hipError_t launch_trunc_list(const uint8_t *flags, int64_t npairs, int *count, int64_t *list, int cap, hipStream_t s);
struct GenericAlignArgs {
  const DevHMM *hmms;
  const double *gtab;
  const uint8_t *residues;
  const int64_t *offsets;
  const int32_t *items;        // pair indices served by this launch
  int n_items;
  const int64_t *pair_q;
  const int32_t *pair_h;
  const int64_t *col_off;
  int32_t *cols;
  int32_t *status;             // per pair: 0 ok, 1 no path has probability, 2 traceback found no cell (or NULL)
  int *counter;
  int Lcap, Qmax, Kp;
  double *slab;
  size_t slab_stride;
  // (last: the fields above keep the offsets they have without them)
  float *pp;                   // optional, CSR like <cols>: posterior probability of each residue's state on the path (wh_align_pp), or NULL
  double *pp64;                // ... or the same as doubles (wh_align_pp64); at most one of the two is set
  size_t pp_off;               // with <pp>: where in the wave's slab the unrounded ppM / ppI rows are kept (generic_align_pp_doubles of them)
  const int32_t *cfg_len;      // optional, per query: the length the pair's length model is configured for (wh_align_pp_len); NULL: the query's own
};
// <longq>: the instantiations that read the residues from the wave's slab in HBM, for queries beyond generic_lds_bytes: the
// copy takes the last generic_seq_doubles(Lcap) doubles of the slab (slab_stride covers them), the LDS block is
// generic_lds_bytes(0) / any size
hipError_t launch_generic_front(const GenericArgs &a, int blocks, size_t lds, hipStream_t s, bool longq = false);
hipError_t launch_generic_align(const GenericAlignArgs &a, int blocks, size_t lds, hipStream_t s, bool longq = false);
size_t generic_front_doubles(int Lcap, int Qmax);
size_t generic_align_doubles(int Lcap, int Qmax);
size_t generic_align_pp_doubles(int Lcap, int Qmax);   // the extra rows of a call that asks for PP
size_t generic_lds_bytes(int Lcap);
size_t generic_seq_doubles(int Lcap);
// the long-query scoring pass: queries longer than <Lmain> (count2: their number, the longest), their pairs on every model,
// and the Forward log-odds of those pairs from the records the front end wrote
hipError_t launch_long_queries(const int64_t *offsets, int64_t nq, int Lmain, int *count2, int64_t *qlist, hipStream_t s);
hipError_t launch_long_pairs(const int64_t *qlist, int n_long, int H, int64_t *pair_list, hipStream_t s);
hipError_t launch_long_fwd_bits(const ResolveRec *recs, int n, int H, float *fwd_bits, wh_pair_detail *detail, hipStream_t s);

// final transitive merge (wh_merge.hip)
struct MergeArgs {
  const uint8_t *q_text;       // query characters as given (ASCII), concatenated
  const int64_t *q_off;        // [nq+1]
  const int32_t *codes;        // consensus kernel output per residue
  const int32_t *q_row;        // per query: >= 0 the query gets a row; -1 widens the gaps only; -2 no alignment
  const int64_t *row_q;        // per query row (in output order after the backbone rows): its query
  int64_t nq;
  const uint8_t *bb;           // backbone rows [nb][B], upper case
  int32_t nb, B;
  int32_t *W;                  // [B+1] widest insertion run per gap (zeroed before merge_runs)
  int32_t *res_gap, *res_k;    // per residue: gap of an insertion (or -1) and position inside its run
  long long *gap_start, *col_pos, *width;   // [B+1], [B], [1]
  uint8_t *out_full, *out_masked;
};
hipError_t launch_merge_runs(const MergeArgs &a, hipStream_t s);
hipError_t launch_merge_layout(const MergeArgs &a, hipStream_t s);
hipError_t launch_merge_render(const MergeArgs &a, int64_t nrows, hipStream_t s);

// wh_msa_dev (wh_msa.hip): hmmalign's alignment of nq sequences to ONE model, assembled from the alignment's per-residue
// columns and posteriors (CSR by the sequences' offsets).  Block k (0..M) is the insert block behind node k (0: the N flank,
// M: the C flank); layout[0..M] its first alignment column, layout[M + 1] the alignment's width W.
struct MsaArgs {
  const int32_t *cols;         // per residue: 0-based node; -1: an insert of the block behind the last match residue (a flank
                               //   at the sequence's ends), as wh_align writes it; -(k + 2): an insert of block k whatever
                               //   surrounds it (the rows of a --mapali alignment: wh_mapali.hip)
  const float *pp;             // per residue r >= pp_shift: pp[r - pp_shift], the posterior of its state on the path
  const uint8_t *text;         // the sequences' characters as given
  const int64_t *off;          // [nq + 1]
  int64_t nq, total;           // total: residues the per-residue arrays hold (no kernel goes beyond it)
  int64_t n_nopp, pp_shift;    // the first n_nopp sequences (residues 0 .. pp_shift - 1) carry no posteriors: no PP row, no part
                               //   in PP_cons, never counted as pathless (0, 0: every sequence has them)
  int32_t M;
  int32_t trim;                // --trim: flank residues are dropped, blocks 0 and M stay empty
  int32_t *width;              // [M + 1] widest insert run per block (zeroed before the widths kernel)
  int32_t *res_blk, *res_k;    // per insert residue: its block (-1: not rendered) and its cell in it: k >= 0 from the
                               //   block's left end, k < 0 from its right end (width + k)
  int *pathless;               // [1] sequences without a match state
  long long *layout;           // [M + 2]
  int32_t *matmap;             // [M] alignment column of node k + 1
  uint8_t *rf, *pp_cons;       // [W] (allocated for the largest possible W)
  uint8_t *rows, *pp_rows;     // [nq][W], [nq - n_nopp][W]
  float *ppm;                  // [chunk rows][M] posterior of the residue at a node, -1: none (a chunk of sequences)
  int64_t q0, q1;              // ... the chunk
  float *cons_sum;             // [M] running float32 sums, in sequence order ...
  int32_t *cons_cnt;           // [M] ... and counts over the chunks so far
  double *cons_sum64;          // WH_MSA_CONS_HMMER: [M] the sums as doubles, HMMER's PP_cons arithmetic (else NULL)
  int32_t last;                // the chunk ends the file: PP_cons is written
};
hipError_t launch_msa_widths(const MsaArgs &a, hipStream_t s);
hipError_t launch_msa_layout(const MsaArgs &a, hipStream_t s);
hipError_t launch_msa_render(const MsaArgs &a, long long W, bool lds, hipStream_t s);
hipError_t launch_msa_cons(const MsaArgs &a, hipStream_t s);
size_t msa_render_lds_bytes(long long W);

// wh_msa_mapali_dev (wh_mapali.hip): the rows of the alignment a model was built from, as sequences for the kernels above.
// colcode[alen]: per alignment column node - 1, or -(k + 2) for an insert column of block k (made from MAP on the host).
struct MapaliArgs {
  const uint8_t *rows;         // [n_map][alen] the alignment's characters (a letter is a residue, anything else a gap)
  int64_t n_map, alen;
  const int32_t *colcode;      // [alen]
  int32_t *count;              // [n_map] residues per row (count kernel)
  const int64_t *off;          // [n_map + 1] their CSR (formed on the host from count), read by the map kernel
  uint8_t *text;               // packed residues' characters ...
  int32_t *cols;               // ... and codes
  const int64_t *seq_off;      // [nq + 1] the new sequences' offsets ...
  int64_t nq, shift;
  int64_t *all_off;            // ... [n_map + nq + 1]: off, then seq_off + shift
};
hipError_t launch_mapali_count(const MapaliArgs &a, hipStream_t s);
hipError_t launch_mapali_map(const MapaliArgs &a, hipStream_t s);
constexpr size_t kMsaLdsBudget = 64 * 1024;   // the two rows of a sequence in LDS: up to 32 K columns, two workgroups per CU stay resident

// wh_hits_msa_dev (wh_hits.hip): the included domains of model h as the sequences of an alignment.  <npairs> = nq x H; the
// domain records, the envelope CSR and the per-residue columns / posteriors are wh_domain_paths_dev's.
struct HitsArgs {
  const uint8_t *flags;        // [npairs]
  const wh_pair_detail *detail;
  const int64_t *dom_off;      // [npairs + 1]
  const wh_domain *dom;        // [ndom]
  int64_t npairs, ndom, nq;
  int H, h;
  const int64_t *env_off;      // [ndom + 1]
  const int32_t *cols;         // per envelope residue: 0-based node or -1 ...
  const float *pp;             // ... and the posterior of its state
  const uint8_t *text;         // the sequences' characters as given ...
  const int64_t *offsets;      // ... [nq + 1]
  const int32_t *order;        // [nq] the queries in output order, or NULL: query order
  float tau, lambda;           // model h's Forward E-value parameters (NaN: no STATS line)
  double ln_inc_seq, ln_inc_dom;   // ln(incE / Z), ln(incdomE / domZ)
  int32_t *len;                // mark kernel: [ndom] residues ali_i..ali_j of an included domain, 0: not included
  int *bad;                    // ... set when a record does not fit dom_off, its envelope or its query, or order[] leaves 0..nq-1
  int64_t nblk;                // workgroups of the scan
  int32_t *pos_row;            // scan: [nq] per output position the rows in front of it inside its workgroup ...
  long long *pos_res;          // ... and their residues
  long long *blk_row, *blk_res;   // [nblk] the workgroups' sums, then their exclusive scan
  long long *totals;           // [2] rows, residues
  int64_t nrows, nres;         // ... as the host read them back
  int64_t *row_dom;            // place kernel: [nrows] the row's domain ...
  int64_t *row_off;            // ... [nrows + 1] the CSR of the batch ...
  wh_hit_row *row_rec;         // ... and the record the caller names the row from
  uint8_t *out_text;           // slice kernel: the batch wh_msa_dev assembles
  int32_t *out_cols;
  float *out_pp;
};
hipError_t launch_hits_mark(const HitsArgs &a, hipStream_t s);
hipError_t launch_hits_scan(const HitsArgs &a, hipStream_t s);
hipError_t launch_hits_place(const HitsArgs &a, hipStream_t s);
hipError_t launch_hits_slice(const HitsArgs &a, hipStream_t s);
int64_t hits_scan_blocks(int64_t nq);

// wh_domain_display_dev (wh_display.hip): the four text lines of hmmsearch's alignment display for the reportable domains of
// model h.  The domain records, the envelope CSR and the per-residue columns / posteriors are wh_domain_paths_dev's; <tab_*>:
// the model's display table (wh_host_display.hip builds it at the first call).
struct DisplayArgs {
  const uint8_t *flags;        // [npairs]
  const int64_t *dom_off;      // [npairs + 1]
  const wh_domain *dom;        // [ndom]
  int64_t npairs, ndom, nq;
  int H, h, M, Kp;
  const uint8_t *residues;     // the residue codes of the scoring call ...
  const int64_t *offsets;      // ... [nq + 1]
  const int64_t *env_off;      // [ndom + 1]
  const int32_t *cols;         // per envelope residue: 0-based node or -1 ...
  const float *pp;             // ... and the posterior of its state
  const float *tab_odds;       // [(M + 1) x Kp] float32 match odds of (node, residue code), degenerate codes included
  const uint8_t *tab_cons;     // [M + 1] consensus letter of the node as the file prints it ...
  const uint8_t *tab_code;     // ... and its digital code
  const uint8_t *tab_sym;      // [32] the alphabet's symbol of every code (upper case)
  double ln_rep_dom;           // ln(domE / domZ)
  int32_t *len;                // count kernel: [ndom] columns of a selected domain, 0: not selected
  int *bad;                    // ... set when a record does not fit dom_off, its envelope, its query or its own path
  int64_t nblk;                // workgroups of the scan
  int32_t *pos_sel;            // scan: [ndom] the selected domains in front of the domain inside its workgroup ...
  long long *pos_len;          // ... and their columns
  long long *blk_sel, *blk_len;   // [nblk] the workgroups' sums, then their exclusive scan
  long long *totals;           // [2] selected domains, columns
  int64_t nsel, total;         // ... as the host read them back
  int64_t *disp_off;           // render kernel: [nsel + 1] the CSR of the lines ...
  wh_display_rec *recs;        // ... [nsel] the domain of each ...
  uint8_t *model, *match, *target, *ppline;   // ... and the four lines, total bytes each
};
hipError_t launch_display_count(const DisplayArgs &a, hipStream_t s);
hipError_t launch_display_scan(const DisplayArgs &a, hipStream_t s);
hipError_t launch_display_render(const DisplayArgs &a, hipStream_t s);
int64_t display_scan_blocks(int64_t ndom);

struct TopkArgs {
  const int32_t *decibits;
  const uint8_t *flags;
  const int32_t *nseq;         // [H]
  const int32_t *hmm_index;    // [H]
  int64_t nq;
  int H, k;
  int32_t *idx;
  double *w;
  int32_t *n_kept;
  int32_t *n_used;
};
hipError_t launch_topk(const TopkArgs &a, hipStream_t s);

// wh_domains_dev (wh_domains.hip): the kernels around the alignment of the packed envelopes.  Each launcher reads the
// fields its kernel needs; <npairs> = nq x H.
struct DomainArgs {
  const uint8_t *flags;        // [npairs]
  const wh_pair_detail *detail;
  int64_t npairs;
  int H;
  int32_t *counts;             // count kernel: [npairs] domains a pair lists ...
  int32_t *n_unlisted;         // ... and (optional) its envelopes beyond them
  const int64_t *dom_off;      // [npairs + 1]
  int64_t ndom;
  int64_t *dom_pair;           // [ndom] list kernel: the domain's pair ...
  int32_t *dom_len;            // ... and its envelope's length; -1: an envelope outside its query
  int32_t *dom_seqlen;         // ... and (optional, WH_LENMODEL_SEQUENCE) its sequence's length
  int *bad;                   // ... set when dom_off does not match the records
  const uint8_t *residues;
  const int64_t *offsets;      // [nq + 1]
  const int64_t *env_off;      // [ndom + 1] CSR of the packed envelopes (and of their columns and posteriors)
  uint8_t *env_res;            // gather kernel: the packed envelopes ...
  int64_t *dom_q;              // ... and the alignment's pair lists: envelope d against model dom_h[d]
  int32_t *dom_h;
  const int32_t *cols;         // summary kernel: the alignment's columns and posteriors
  const float *pp;
  const float *evp;            // [H][2] Forward tau, lambda (NaN: no STATS line)
  wh_domain *out;
};
hipError_t launch_domain_count(const DomainArgs &a, hipStream_t s);
hipError_t launch_domain_list(const DomainArgs &a, hipStream_t s);
hipError_t launch_envelope_gather(const DomainArgs &a, hipStream_t s);
hipError_t launch_domain_summary(const DomainArgs &a, hipStream_t s);

constexpr int kAlignSpecArrays = 14;   // special-state rows per wave of the alignment kernel (AL_NARR)
struct AlignArgs {
  const DevHMM *hmms;
  const float *tables;
  const uint8_t *residues;
  const int64_t *offsets;
  const int64_t *pair_q;
  const int32_t *order;        // pair indices grouped by model
  const int32_t *item_h;       // work items: model position, first entry of <order>, entry count
  const int32_t *item_start;
  const int32_t *item_count;
  int n_items;
  const int64_t *col_offsets;
  int32_t *cols;
  int *counter;
  int Lcap, SP, wave_lds;
  float *scratch;              // per-wave slabs: Forward/posterior rows, then OA rows
  size_t scratch_stride;       // floats per wave
  float *spec_scratch;         // long-query mode: per-wave special-state rows in HBM (else NULL -> LDS)
  size_t spec_stride;
  int Klds;                    // emission rows staged in LDS (= K, or 0: read from L2)
  int K, Kp;
  int *redo_count;             // pairs whose Backward sweep saturated (float32 range) are appended to
  int32_t *redo_list;          // redo_list for the log-space pass (NULL in that pass)
  int logsp;                   // 1: this launch is the log-space pass
  int swap;                    // 1: pass-synchronous variant (one table orientation resident in LDS)
  int no_window;               // 1: Backward / OA / traceback at full width only (WH_NO_WINDOW)
  int *wstat;                  // NULL or 4 counters: pairs aligned on a 256-node window, window rejected, window not tried, 512-node window
  unsigned long long *wcyc;    // NULL or 4 wave-cycle sums of the window pairs: Forward, Backward + posteriors, OA fill, traceback
  const int32_t *cfg_len;      // optional, per query: the length the pair's length model is configured for (wh_align_pp_len); NULL: the query's own
};
// what the host fills in; the kernels without the PP output take the core alone (the kernel arguments a build without the
// feature has), the ones with it the whole
struct AlignArgsPP : AlignArgs {
  float *pp;                   // optional, CSR like <cols>: posterior probability of each residue's state on the path (wh_align_pp), or NULL
  double *pp64;                // ... or the same as doubles (wh_align_pp64); at most one of the two is set
};
hipError_t launch_align(int Q, const AlignArgsPP &a, int blocks, int threads, size_t lds, hipStream_t s);

struct ConsArgs {
  const int64_t *offsets;
  int64_t nq;
  const int64_t *qpair_off;
  const int32_t *pair_h;
  const double *pair_w;
  const int64_t *col_offsets;
  const int32_t *cols;
  const int64_t *ret_off;
  const int32_t *retained;
  const int32_t *nongaps;
  int backbone_length;
  int32_t *out;
  int32_t *minmax;
  int *counter;
  int Lcap, Wcap, KMAX;
  uint8_t *back;               // per wave (Lcap+1) x (Wcap+2) back-pointers
  int32_t *cwj;                // per wave Lcap x KMAX edge columns
  double *cwv;                 // per wave Lcap x KMAX edge weights
  int32_t *cwn;                // per wave Lcap edge counts
  double *rowg;                // per wave Wcap+2 doubles: the DP row when it does not fit in LDS (else NULL)
};
hipError_t launch_consensus(const ConsArgs &a, int blocks, int threads, size_t lds, hipStream_t s);

}  // namespace wh
