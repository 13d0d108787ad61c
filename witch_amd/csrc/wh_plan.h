// LDS planning of the scoring and alignment launches: which kernel family a size class takes at a query length, the waves
// and the block of a workgroup - and from the same functions the main length cap of a call (Lmain): the longest query every
// class of a handle can plan.  Host code without a HIP call (tools/plan_check.cpp runs it under the sanitizers); the three
// formulas below live beside their kernels.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

#include "wh_common.h"

namespace wh {

size_t wide_lds_bytes(int Lcap, size_t em_floats);      // wh_score_wide.hip
size_t generic_lds_bytes(int Lcap);                     // wh_generic.hip
int score9_block_floats(int SP, int Lcap);              // wh_score9.hip

constexpr size_t kLdsBudget = 160 * 1024 - 512;
constexpr size_t kLdsHeader = 16;   // work-item slot in front of the tables (keeps them 16-byte aligned)
// per-row special-state arrays of a wave's LDS block in the phase-call scoring kernel (wh_score7.hip is built with
// WH_SLIM_SPEC: N, B, E, J, C, scale; an envelope's mask words share the B / E slots), and of the alignment kernel (AL_NARR)
constexpr int kScoreSpecArrays = 6;
// ... and how the default scoring object lays that block out: 0 six arrays, 1 one 6-word record per row (SpecAt, wh_device.h; the
// Makefile hands the same K7_LAYOUT to the object and to the host).  The sizes are the same either way.
#ifndef WH_K7_LAYOUT
#define WH_K7_LAYOUT 1
#endif
constexpr int kScoreSpecLayout = WH_K7_LAYOUT;
constexpr int kAlignSpecRows = 14;
constexpr int kMaxPlanLength = 1 << 24;                                    // the length searches below end here

inline int row_stride(int Lc) { return (Lc + 1 + 3) / 4 * 4; }        // floats of one per-row array: rows 0..Lc, 16-byte multiple
inline int residue_words(int Lc) { return (Lc + 3) / 4 + 4; }         // words of a wave's residue buffer
// LDS of a workgroup: <header> bytes, the model's tables, <w> wave blocks of <wave_words> words; and the most waves (from
// <w> down, 0 = none) of which <per_cu> such workgroups fit a CU.  (The alignment planner tests without the header.)
inline size_t lds_bytes(size_t header, size_t table, int w, int wave_words) { return header + table + (size_t)w * (size_t)wave_words * sizeof(float); }
inline int fit_waves(size_t header, size_t table, int w, int wave_words, int per_cu = 1) {
  while (w >= 1 && per_cu * lds_bytes(header, table, w, wave_words) > kLdsBudget) w--;
  return w;
}
// Long models (pass-synchronous scoring and alignment): ONE orientation resident, four waves - one per SIMD, the kernel
// uses the whole register file; the emission rows beside it where they fit (Klds = K), else read from L2 (Klds = 0).
inline bool plan_long_model(int Q, int K, int wave_words, int *Klds, size_t *lds) {
  *Klds = K;
  size_t table = (size_t)(K + 8) * Q * kWave * sizeof(float);
  if (lds_bytes(kLdsHeader, table, 4, wave_words) > kLdsBudget) { *Klds = 0; table = (size_t)8 * Q * kWave * sizeof(float); }
  *lds = lds_bytes(kLdsHeader, table, 4, wave_words);
  return *lds <= kLdsBudget;
}

// what of a handle's knobs and a call's switches decides an LDS plan
struct PlanKnobs { int kernel = 7, max_waves = 0; bool force_specg = false, no_window = false, no_p2win = false, p2win_force = false; };
struct LdsPlan { int waves, SP, wave_lds; size_t lds; };
inline int cap_waves(int max_waves, int w) { return max_waves > 0 ? std::max(1, std::min(w, max_waves)) : w; }
inline size_t score_table_bytes(int K, int Q) { return (size_t)(K + 2 * FW_NARR) * Q * kWave * sizeof(float); }   // K emission rows + both transition orientations

// LDS plan of the phase-call scoring kernel: tables + per wave one block (special-state arrays, null2 table, region
// list, residues), up to <top> waves (twelve; sixteen for the four-waves-per-SIMD launch below).  <b> is left alone when not
// even one wave fits.
inline bool plan_block1(int max_waves, int K, int Q, int Lcap, int extra_arrays, LdsPlan *b, int top = 12) {
  const int sp = row_stride(Lcap);
  const int wl = (kScoreSpecArrays + extra_arrays) * sp + 32 + kRegsInts + residue_words(Lcap);
  const int w = fit_waves(kLdsHeader, score_table_bytes(K, Q), cap_waves(max_waves, top), wl);
  if (w < 1) return false;
  *b = {w, sp, wl, lds_bytes(kLdsHeader, score_table_bytes(K, Q), w, wl)};
  return true;
}

// Four waves per SIMD (wh_score7w.o: workgroups of 1 024 threads at 128 vector registers): the classes
// that take sixteen waves where sixteen six-array blocks fit beside their tables.  Bit Q / 4 of kFourWaveClasses: the classes
// that take it by default, each only where its own A/B run on the headline's shape showed a gain; WH_MAX_WAVES=16 asks for it
// in every class the object serves (8, 12 and 16 cells per lane), any other cap (WH_MAX_WAVES=12: the launch as it was) for none.
// Never thirteen to fifteen waves: they pay the 128-register budget for less than a full fourth wave.
constexpr int kFourWaveClasses = 1 << 4;      // the 16-cell class (the headline); the 8- and 12-cell classes have no such run yet
inline bool four_wave_class(int max_waves, int Q) {
  if (Q != 8 && Q != 12 && Q != 16) return false;
  return max_waves == 16 || (max_waves == 0 && ((kFourWaveClasses >> (Q / 4)) & 1));
}

// The kernel family and the LDS block of one scoring size class (Q cells per lane, K canonical residues) at the length cap
// Lc.  Three kernels serve a size class:
//  * phase-call kernel, special states in LDS: models of up to 24 cells per lane, short queries
//  * the same kernel with the special-state rows in HBM (specg): long queries
//  * pass-synchronous kernel (big; wh_score_big.hip): 28+ cells per lane, 20/24-cell models whose
//    emission rows do not fit in LDS beside both orientations (protein), and 16-cell models with a query for which
//    not one wave fits beside their tables
// and the two-queries-per-wave kernel takes the classes it fits when asked for (pairk; <with9> false: not considered).
// false: a query of Lc residues does not fit the class.
struct ScoreLds { LdsPlan b; bool big, specg, pairk, p2win, p2inpl; int Klds; bool four; };   // <four>: sixteen waves, the 1 024-thread object
inline bool plan_score_lds(const PlanKnobs &kn, int K, int Q, int Lc, bool with9, ScoreLds *out) {
  const size_t table = score_table_bytes(K, Q);
  ScoreLds r = {};
  LdsPlan &b = r.b;
  r.big = Q > kMaxQFast;
  if (with9 && !r.big && kn.kernel == 9 && !kn.force_specg && (Q == 8 || Q == 12 || Q == 16)) {
    // two queries per wavefront (wh_score9.hip): eight waves, each with two blocks of per-row arrays
    const int wl9 = 2 * score9_block_floats(row_stride(Lc), Lc), w9 = cap_waves(kn.max_waves, 8);
    if (lds_bytes(kLdsHeader, table, w9, wl9) <= kLdsBudget) { r.pairk = true; b = {w9, row_stride(Lc), wl9, lds_bytes(kLdsHeader, table, w9, wl9)}; }
  }
  if (!r.big && !r.pairk) {
    // (twelve waves = three per SIMD at 168 registers; 20-cell models keep that since the six-array block, 24-cell
    // models get the nine or ten waves that fit beside their 120 KB of tables)
    bool ok = plan_block1(kn.max_waves, K, Q, Lc, 0, &b);
    // ... and, where the waves still fit with them, three more per-row arrays per wave: the multihit Backward sweep then
    // tries a node window first (wh_score7.hip, "P2 on a node window")
    if (ok && b.waves >= 4 && !kn.force_specg && !kn.no_window && !kn.no_p2win && Q >= 8) {
      LdsPlan b2 = {};
      if (plan_block1(kn.max_waves, K, Q, Lc, 3, &b2) && (b2.waves >= b.waves || (kn.p2win_force && b2.waves >= 8))) { r.p2win = true; b = b2; }
      else if (Q >= 20 && kn.kernel != 9) r.p2inpl = true;      // round 5: the window sweep in place, P1's rows backed up in HBM (ScoreArgs::p2win == 2)
    }
    // ... and sixteen waves, four per SIMD, where sixteen six-array blocks fit (short queries on DNA models of up to 16 cells
    // per lane): the default kernel's own launch only, and the window sweep in place - the three more rows would leave room for
    // thirteen blocks at most.  A length at which the sixteen do not fit keeps the plan above unchanged.
    if (ok && b.waves >= 4 && !kn.force_specg && !kn.no_window && !kn.no_p2win && kn.kernel == 7 && four_wave_class(kn.max_waves, Q)) {
      LdsPlan b4 = {};
      if (plan_block1(kn.max_waves, K, Q, Lc, 0, &b4, 16) && b4.waves == 16) { r.four = true; r.p2win = false; r.p2inpl = true; b = b4; }
    }
    if (!ok || b.waves < 4 || kn.force_specg) {
      r.specg = true;
      b.SP = row_stride(Lc);
      b.wave_lds = 32 + kRegsInts + residue_words(Lc);
      b.waves = fit_waves(kLdsHeader, table, cap_waves(kn.max_waves, Q <= 16 ? 12 : 8), b.wave_lds);
      ok = b.waves >= 1;
      b.lds = lds_bytes(kLdsHeader, table, b.waves, b.wave_lds);
      if (Q >= 20 && (!ok || b.waves < 4)) r.big = true;
      // 16-cell models whose tables (protein: 92 KB) leave not even one wave's residues: the pass-synchronous kernel, as the
      // 20-cell models take it - otherwise the class would accept HALF the query length of the next larger one
      if (Q == 16 && !ok) r.big = true;
    }
    if (!r.big && !ok) return false;
  }
  if (r.big) {
    b.waves = 4; b.SP = row_stride(Lc); b.wave_lds = 32 + kRegsInts + residue_words(Lc);
    if (!plan_long_model(Q, K, b.wave_lds, &r.Klds, &b.lds)) return false;
    r.specg = true;
  }
  *out = r;
  return true;
}

// LDS plan of the alignment kernel for one size class (waves, block, tables).  0: planned; 1: a query of Lc residues does
// not fit the class; 2: the class's tables do not fit whatever the query.
struct AlignLds { int waves, SP, wave_lds, Klds; size_t lds; bool spec_in_hbm, swap; };
inline int plan_align_lds(bool force_specg, int K, int Q, int Lc, AlignLds *out) {
  const size_t table = (size_t)(K + 2 * FW_NARR) * Q * kWave * sizeof(float);
  AlignLds p = {};
  p.Klds = K; p.SP = row_stride(Lc);
  if (Q <= kMaxQFast) {      // special states in LDS, up to eight waves
    p.wave_lds = kAlignSpecRows * p.SP + residue_words(Lc);
    p.waves = std::max(0, fit_waves(0, table, 8, p.wave_lds));
    p.lds = lds_bytes(kLdsHeader, table, p.waves, p.wave_lds);
  }
  p.swap = Q > kMaxQFast;
  // 20/24-cell models whose emission rows (protein: 20) do not fit beside BOTH orientations even
  // with the special states in HBM: pass-synchronous variant
  if (!p.swap && Q >= 20 && (p.waves < 4 || force_specg) && lds_bytes(kLdsHeader, table, 4, residue_words(Lc)) > kLdsBudget) p.swap = true;
  // ... and 16-cell models with a query for which not one wave fits beside them (what used to be refused)
  if (!p.swap && Q == 16 && fit_waves(kLdsHeader, table, 8, residue_words(Lc)) < 1) p.swap = true;
  if (p.swap) {   // long models: one orientation resident, 4 waves, special states in HBM
    p.spec_in_hbm = true; p.wave_lds = residue_words(Lc); p.waves = 4;
    if (!plan_long_model(Q, K, p.wave_lds, &p.Klds, &p.lds)) return 1;
  } else if (p.waves < 4 || force_specg) {   // long queries: special-state rows in HBM
    p.spec_in_hbm = true; p.wave_lds = residue_words(Lc);
    p.waves = fit_waves(kLdsHeader, table, 8, p.wave_lds);
    if (p.waves < 1) return lds_bytes(kLdsHeader, table, 1, residue_words(1)) > kLdsBudget ? 2 : 1;
    p.lds = lds_bytes(kLdsHeader, table, p.waves, p.wave_lds);
  }
  *out = p;
  return 0;
}

// ---- the main length cap of a call.  The classes of a handle that decide it:
struct PlanClasses {
  int K = 4;
  std::vector<int> score_q, align_q;   // cells per lane of the one-wave classes the scoring / the alignment launches plan
  bool wide = false;                   // models scored by the several-waves-per-pair kernel ...
  bool force_wide = false;             // ... which must take them (WH_FORCE_WIDE), else a batch too long for it falls to the float64 front end
  bool front = false;                  // models scored by the float64 front end in every call
};
// Every scoring launch of a call with the length cap L can be planned.  <as_today> false: the wide kernel must fit as well
// (the cap of the main launches); true: what a call needs to run at all - a batch too long for the wide kernel is the
// front end's.
inline bool score_fits(const PlanKnobs &kn, const PlanClasses &cl, int L, bool as_today) {
  ScoreLds s;
  for (int Q : cl.score_q) if (!plan_score_lds(kn, cl.K, Q, L, false, &s)) return false;
  const bool wide_ok = !cl.wide || wide_lds_bytes(L, 0) <= kLdsBudget;
  if (!wide_ok && (cl.force_wide || !as_today)) return false;
  if ((cl.front || (cl.wide && !wide_ok)) && generic_lds_bytes(L) > kLdsBudget) return false;
  return true;
}
inline bool align_fits(const PlanKnobs &kn, const PlanClasses &cl, int L) {
  AlignLds a;
  for (int Q : cl.align_q) if (plan_align_lds(kn.force_specg, cl.K, Q, L, &a) != 0) return false;
  return true;
}
// the largest length of 1 .. kMaxPlanLength that <fits> accepts (it accepts every shorter one then); 0: none
template <class Fits> int largest_length(Fits fits) {
  if (!fits(1)) return 0;
  int lo = 1, hi = kMaxPlanLength;
  while (lo < hi) {
    const int mid = lo + (hi - lo + 1) / 2;
    if (fits(mid)) lo = mid; else hi = mid - 1;
  }
  return lo;
}
// Lmain of a call whose longest query has Lc residues: Lc itself when the call can be planned as it is, else the largest
// length every class accepts; queries beyond it are the long-query pass's.  (0 classes accept nothing: Lc, and the planner
// says why.)
inline int score_main_cap(const PlanKnobs &kn, const PlanClasses &cl, int Lc) {
  if (score_fits(kn, cl, Lc, true)) return Lc;
  const int cap = largest_length([&](int L) { return score_fits(kn, cl, L, false); });
  return cap > 0 ? std::min(cap, Lc) : Lc;
}
inline int align_main_cap(const PlanKnobs &kn, const PlanClasses &cl, int Lc) {
  if (align_fits(kn, cl, Lc)) return Lc;
  const int cap = largest_length([&](int L) { return align_fits(kn, cl, L); });
  return cap > 0 ? std::min(cap, Lc) : Lc;
}
// the length up to which queries stay on the float32 kernels in scoring AND alignment, however long the call's longest
inline int query_len_cap(const PlanKnobs &kn, const PlanClasses &cl) {
  const int s = largest_length([&](int L) { return score_fits(kn, cl, L, false); });
  const int a = largest_length([&](int L) { return align_fits(kn, cl, L); });
  return std::min(s, a);
}

}  // namespace wh
