// hmmsearch's acceleration pipeline in front of the scoring kernels: MSV filter -> (bias filter) -> Viterbi filter ->
// Forward, as HMMER 3.1b2's p7_Pipeline runs it per (model, sequence of length L).  Restated from HMMER's published
// behaviour and pinned on the stage outcomes of the reference's bundled hmmsearch (tests/golden/filters).
//
// The two integer dynamic programmes are wh_calibrate.h's (calib_msv_core, calib_viterbi_core), unchanged.  What this
// header adds is what calibration does not need because it fixes L and draws canonical residues only:
//  * the settings that depend on the query's length: the MSV filter's tjb and the Viterbi filter's N/C/J move cost
//    (both from logf(3 / (L + 3))) and null1 - one FilterLen record per length, made on the host, so that no
//    transcendental is ever evaluated on the device;
//  * table columns for degenerate residues (Kp columns instead of K): the expected score over the residue set on the
//    float profile, in float32 like esl_abc_FExpectScVec, then quantised like any other column;
//  * raw score -> nats -> decision.  HMMER rejects where P > F with P = gumbel_surv(bits; mu, lambda) in double.  The
//    survival functions fall monotonically, so "P > F" is "bits < x(F)" with x(F) the smallest float32 whose P is <= F:
//    surv_threshold finds it with the host's libm, once per model and call.  Host and device then make every decision
//    by comparing float32 scores that both compute with correctly rounded operations alone (integer -> float, add,
//    subtract, a float64 division): the same bits on both sides, and HMMER's own arithmetic.
// The bias filter is an OPT-IN (wh_filter_opts.nobias = WH_BIAS_FILTER_ON; the default later): a
// pair past the MSV stage is scored by the scaled float32 Forward of a two-state composition HMM ("the bias filter" below),
// pinned on the stage outcomes of the binary run without --nobias (tests/golden/filters_bias).  Its score, filtersc, then
// stands where null1 stands otherwise: in stage 2, in the "run the Viterbi filter" test, and in stages 3 and 4.  Host and
// device evaluate the same statements - no fused operation, divisions through float64, a logarithm made of float64
// + - x / alone - so they agree bit for bit here too.  With nobias = 1 the pipeline runs as hmmsearch --nobias does: the
// reference score of every stage is null1, and the bias stage counts as passed wherever the MSV stage is.
#pragma once

#include <cstring>

#include "wh_calibrate.h"
#include "wh_common.h"

namespace whf {

using namespace whc;

constexpr double kLog2 = 0.69314718055994529;

// wh_filter_opts with HMMER's defaults
struct FilterOpts {
  double F1 = 0.02, F2 = 1e-3, F3 = 1e-5;
  int nobias = 0;      // wh_filter_opts.nobias: 1, or WH_BIAS_FILTER_ON
  bool bias() const { return nobias == WH_BIAS_FILTER_ON; }
};

// bits of the stage byte
enum { kStageMSV = 1, kStageBias = 2, kStageVit = 4, kStageVitRan = 8, kStageFwd = 16, kStageBadLen = 128 };

// ---- per query length ------------------------------------------------------------------------------------------
struct FilterLen {
  float nullsc;        // p7_bg_NullOne
  int16_t xmove;       // Viterbi filter: N->B, J->B, C->T
  uint8_t tjb;         // MSV filter: the same move, in its units
  uint8_t pad;
};

inline FilterLen filter_len(int L) {
  FilterLen f;
  CalibMSV m; m.scale = (float)(3.0 / kLog2); m.bias = 0;
  CalibVit v; v.scale = (float)(500.0 / kLog2);
  const float mv = logf(3.0f / ((float)L + 3.0f));
  f.nullsc = L > 0 ? calib_nullone(L) : 0.f;
  f.tjb = m.unbiased(mv);
  f.xmove = v.wordify(mv);
  f.pad = 0;
  return f;
}

// ---- P-values (Easel's esl_gumbel_surv, esl_exp_surv) -------------------------------------------------------------
inline double gumbel_surv(double x, double mu, double lambda) {
  const double y = lambda * (x - mu);
  const double ey = -std::exp(-y);
  if (std::fabs(ey) < 5e-9) return -ey;
  return 1.0 - std::exp(ey);
}
inline double exp_surv(double x, double mu, double lambda) {
  if (x < mu) return 1.0;
  return std::exp(-lambda * (x - mu));
}

// the smallest float32 x with surv(x) <= F (surv falls with x): "P > F" <=> "score < x".  F >= 1 never rejects
// (-infinity), F <= 0 rejects every finite score (+infinity: an overflowed filter still passes, as in HMMER)
template <class Surv> inline float surv_threshold(Surv surv, double guess, double F) {
  if (!(F < 1.0)) return -INFINITY;
  if (!(F > 0.0)) return INFINITY;
  float x = (float)guess;
  if (!std::isfinite(x)) x = 0.f;
  // walk to the boundary: first in growing strides, then float by float
  float step = std::max(1e-3f, std::fabs(x) * 1e-6f);
  for (int it = 0; it < 200 && surv((double)x) > F; it++) { x += step; step *= 2.f; }
  step = std::max(1e-3f, std::fabs(x) * 1e-6f);
  for (int it = 0; it < 200 && surv((double)(x - step)) <= F; it++) { x -= step; step *= 2.f; }
  // now surv(x) <= F < surv(x - step): bisect on floats
  float lo = x - step, hi = x;
  for (int it = 0; it < 200; it++) {
    const float mid = lo + (hi - lo) * 0.5f;
    if (!(mid > lo && mid < hi)) break;
    if (surv((double)mid) <= F) hi = mid; else lo = mid;
  }
  return hi;
}

struct FilterThr {
  float x1;       // MSV (and bias) stage: rejected below, in bits against the MSV Gumbel at F1
  float x2m;      // the Viterbi filter runs where the last MSV-stage score is below this (its P > F2)
  float x2v;      // Viterbi stage, against the Viterbi Gumbel at F2
  float x3;       // Forward stage, against the exponential tail at F3
};

// evp: MSV mu, lambda; Viterbi mu, lambda; Forward tau, lambda (the STATS LOCAL lines, float32 as HMMER holds them)
inline FilterThr filter_thresholds(const float evp[6], const FilterOpts &o) {
  FilterThr t;
  const double mmu = evp[0], mlam = evp[1], vmu = evp[2], vlam = evp[3], tau = evp[4], flam = evp[5];
  auto gm = [&](double x) { return gumbel_surv(x, mmu, mlam); };
  auto gv = [&](double x) { return gumbel_surv(x, vmu, vlam); };
  auto ef = [&](double x) { return exp_surv(x, tau, flam); };
  auto ginv = [](double mu, double lam, double F) { return F > 0. && F < 1. ? mu - std::log(-std::log1p(-F)) / lam : 0.; };
  t.x1 = surv_threshold(gm, ginv(mmu, mlam, o.F1), o.F1);
  t.x2m = surv_threshold(gm, ginv(mmu, mlam, o.F2), o.F2);
  t.x2v = surv_threshold(gv, ginv(vmu, vlam, o.F2), o.F2);
  t.x3 = surv_threshold(ef, o.F3 > 0. && o.F3 < 1. ? tau - std::log(o.F3) / flam : 0., o.F3);
  return t;
}

// ---- the bias filter's settings (its arithmetic: below, "the bias filter") ------------------------------------------------
struct FilterBias {      // per model
  float t10, t11;        // composition state -> background state, -> itself: 1 / (L1 + 1), L1 / (L1 + 1), L1 = M / 8
  float eo1[30];         // [Kp] odds ratios of the composition state
};
struct FilterBiasLen {   // per query length (host, libm - as FilterLen)
  float t00, t01;        // p7_bg_SetLength overwrites the background state's own transitions: p1, 1 - p1
  float lp1, lq1;        // (float) L * logf(p1), logf(1 - p1)
};

inline FilterBiasLen filter_bias_len(int L) {
  FilterBiasLen b;
  const float p1 = (float)L / (float)(L + 1);
  b.t00 = p1;
  b.t01 = 1.0f - p1;
  b.lp1 = (float)L * logf(p1);
  b.lq1 = logf((float)(1.0 - (double)p1));
  return b;
}

// compo [K] (float32 as parsed), bg [K]
inline void filter_bias_prepare(int M, int K, int Kp, const uint32_t *degen, const float *compo, const float *bg, FilterBias &fb) {
  const float L1 = (float)M / 8.0f;
  fb.t10 = 1.0f / (L1 + 1.0f);
  fb.t11 = L1 / (L1 + 1.0f);
  for (int x = 0; x < 30; x++) fb.eo1[x] = 1.0f;
  for (int x = 0; x < K; x++) fb.eo1[x] = compo[x] / bg[x];
  for (int x = K + 1; x <= Kp - 3; x++) {
    if (!degen[x]) continue;
    float num = 0.f, den = 0.f;
    for (int a = 0; a < K; a++)
      if (degen[x] & (1u << a)) { num += compo[a]; den += bg[a]; }
    fb.eo1[x] = num / den;
  }
}

// ---- one model ---------------------------------------------------------------------------------------------------
struct FilterModel {
  int M = 0, K = 0, Kp = 0;
  CalibMSV msv;        // rb [Kp][M+1]; tjb is per query (FilterLen)
  CalibVit vit;        // rw [Kp][M+1], tw [M+1][8]; xNCJ_move is per query
  float evp[6] = {0, 0, 0, 0, 0, 0};
  FilterBias bias;     // the bias filter's per-model settings (filter_model_of)
};

// h: the model's probabilities in float32 (K canonical residues); degen[x]: bit a set where code x stands for residue a
// (0: gap, nonresidue, missing data - impossible in a match state)
inline void filter_prepare(const CalibModel &h, int Kp, const uint32_t *degen, FilterModel &fm) {
  CalibProfile gm, gx;
  calib_profile(h, gm);
  const int M = h.M, K = h.K;
  gx.M = M; gx.K = Kp;
  gx.tsc = gm.tsc; gx.bm = gm.bm;
  gx.msc.assign((size_t)(M + 1) * Kp, -INFINITY);
  for (int k = 1; k <= M; k++) {
    const float *sc = &gm.msc[(size_t)k * K];
    float *out = &gx.msc[(size_t)k * Kp];
    for (int x = 0; x < K; x++) out[x] = sc[x];
    for (int x = K + 1; x <= Kp - 3; x++) {      // esl_abc_FExpectScore: float32 sums in residue order
      if (!degen[x]) continue;
      float result = 0.f, denom = 0.f;
      for (int a = 0; a < K; a++)
        if (degen[x] & (1u << a)) { result += sc[a] * h.bg[a]; denom += h.bg[a]; }
      out[x] = result / denom;
    }
  }
  fm.M = M; fm.K = K; fm.Kp = Kp;
  calib_msv_convert(gx, fm.msv);      // (bias: the maximum over all columns is the maximum over the canonical ones)
  calib_vit_convert(gx, fm.vit);
}

// a parsed model file -> its filter tables (degen: wh::degen_masks of its alphabet).  Returns nullptr, or the name of the
// STATS LOCAL line the file lacks: a model without E-value statistics cannot be filtered
inline const char *filter_model_of(const wh::HostHMM &h, const uint32_t *degen, FilterModel &fm) {
  if (!h.has_mstats) return "MSV";
  if (!h.has_vstats) return "VITERBI";
  if (!h.has_fstats) return "FORWARD";
  float bg[20];
  for (int a = 0; a < h.K; a++) bg[a] = h.alphabet == WH_ALPH_AMINO ? (float)wh::kAminoBg[a] : 0.25f;
  const CalibModel cm{h.M, h.K, h.tf.data(), h.matf.data(), bg};
  filter_prepare(cm, h.Kp, degen, fm);
  filter_bias_prepare(h.M, h.K, h.Kp, degen, h.compo.data(), bg, fm.bias);
  fm.evp[0] = h.mmu; fm.evp[1] = h.mlambda; fm.evp[2] = h.vmu; fm.evp[3] = h.vlambda; fm.evp[4] = h.ftau; fm.evp[5] = h.flambda;
  return nullptr;
}

// ---- raw integer -> nats -> bits: float32 steps that are correctly rounded on the host and on the device alike ------
WH_HD inline float filter_div(float a, double b) { return (float)((double)a / b); }

WH_HD inline float filter_msv_nats(int raw, int tjb, int base, float scale) {
  if (raw < 0) return INFINITY;                // overflow: passes
  float sc = (float)(raw - tjb) - (float)base;
  sc = filter_div(sc, (double)scale);
  return sc - 3.0f;
}
WH_HD inline float filter_vit_nats(int raw, int xmove, int base, float scale) {
  if (raw == kCalibVitOverflow) return INFINITY;
  if (raw <= -32768) return -INFINITY;
  float sc = (float)raw + (float)xmove - (float)base;
  sc = filter_div(sc, (double)scale);
  return sc - 3.0f;
}
// (sc - ref) / ln 2 as p7_Pipeline computes it: float32 difference, float64 division, stored as float32
WH_HD inline float filter_bits(float sc, float ref) { return filter_div(sc - ref, kLog2); }

// stages 1 and 2 from the MSV filter's raw score (no bias filter: stage 2 passes with stage 1); *run_vit: the Viterbi filter
// has to run (else it counts as passed)
WH_HD inline int filter_stage12(int msv_raw, FilterLen fl, int base, float scale, FilterThr t, bool *run_vit) {
  *run_vit = false;
  const float usc = filter_msv_nats(msv_raw, fl.tjb, base, scale);
  const float s = filter_bits(usc, fl.nullsc);
  if (s < t.x1) return 0;
  int st = kStageMSV | kStageBias;
  *run_vit = s < t.x2m;
  if (!*run_vit) st |= kStageVit;
  return st;
}
// ---- the bias filter (p7_bg_SetFilter, p7_bg_SetLength, p7_bg_FilterScore) ----------------------
// A two-state HMM scores the query: state 0 emits the background (odds ratio exactly 1 for every code), state 1 the
// model's composition (odds eo1[x] = compo[x] / f[x]; a degenerate code: float32 sums over its residues in residue order;
// gap, nonresidue, missing: 1).  Easel's scaled Forward runs on it in float32, each product and sum rounded (no FMA),
// the logarithm of every row's maximum in float64.  Host and device run THIS code: float32 + and x, divisions through
// float64 (rounding a float64 quotient of two float32 to float32 is the correctly rounded float32 quotient: 53 >= 2 x 24
// + 2 bits), and filter_log, which uses + - x / on float64 alone - no libm on either side, the same bits on both.
// (float) log((double) x) for a finite x > 0, from + - x / on float64: x = 2^e m with m in [sqrt(1/2), sqrt(2)),
// s = (m - 1) / (m + 1), ln m = 2 s + 2 s z P(z), z = s^2, P = 1/3 + z/5 + ... + z^12/27 (|s| < 0.1716: the first term
// left out is below 2^-70), + e ln 2 in two parts.  Equal to the host libm's value on every float32 in [1/4, 4)
// (tests/test_filters_bias_host.py); what matters to the pipeline is that host and device evaluate the same operations.
WH_HD inline float filter_log(float x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double xd = (double)x;
  unsigned long long u;
  memcpy(&u, &xd, 8);
  int e = (int)((u >> 52) & 0x7FFull) - 1023;
  u = (u & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull;
  double m;
  memcpy(&m, &u, 8);
  if (m > 1.4142135623730951) { m = m * 0.5; e++; }
  const double s = (m - 1.0) / (m + 1.0), z = s * s;
  double P = 1.0 / 27.0;
  P = P * z + 1.0 / 25.0; P = P * z + 1.0 / 23.0; P = P * z + 1.0 / 21.0; P = P * z + 1.0 / 19.0; P = P * z + 1.0 / 17.0;
  P = P * z + 1.0 / 15.0; P = P * z + 1.0 / 13.0; P = P * z + 1.0 / 11.0; P = P * z + 1.0 / 9.0; P = P * z + 1.0 / 7.0;
  P = P * z + 1.0 / 5.0; P = P * z + 1.0 / 3.0;
  const double s2 = 2.0 * s, de = (double)e;
  const double r = de * 6.93147180369123816490e-01 + (s2 + (s2 * z * P + de * 1.90821492927058770002e-10));
  return (float)r;
}

// the scaled Forward's state between rows: (a, b) = the two states' values of the last row, divided by their maximum
struct FilterBiasRow { float a, b; };
// one row (first: row 1, from the start probabilities 0.999, 0.001); eo: the composition state's odds of the row's residue.
// Returns the row's maximum, whose logarithm is the row's term.  The maximum is never 0: row 1's background value is
// 0.999, and later rows' is a t00 + b t10 with a or b = 1 and t00, t10 > 0.  An odds ratio of 0 (a COMPO entry of '*')
// only empties the composition state for that row: b = 0, and the next row enters it again through a t01.
WH_HD inline float filter_bias_row(FilterBiasRow &s, bool first, float eo, float t10, float t11, FilterBiasLen bl) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float na, nb;
  if (first) { na = 1.0f * 0.999f; nb = eo * 0.001f; }
  else {
    const float a0 = s.a * bl.t00, b0 = s.b * t10, a1 = s.a * bl.t01, b1 = s.b * t11;
    na = a0 + b0;
    const float n1 = a1 + b1;
    nb = n1 * eo;
  }
  const float mx = na > nb ? na : nb;
  s.a = filter_div(na, (double)mx);
  s.b = filter_div(nb, (double)mx);
  return mx;
}
// the end state's term and p7_bg_FilterScore's length terms
WH_HD inline float filter_bias_end(float nullsc, FilterBiasRow s, FilterBiasLen bl) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float ab = s.a + s.b;
  nullsc = nullsc + filter_log(ab);
  const float f = nullsc + bl.lp1;
  return f + bl.lq1;
}
// filtersc of one query: seq.get(i), i = 1 .. L (L >= 1), codes below Kp
template <class Seq> WH_HD inline float filter_bias_score(const float *eo1, float t10, float t11, FilterBiasLen bl, const Seq &seq, int L) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  FilterBiasRow s{0.f, 0.f};
  float nullsc = 0.f;
  for (int i = 1; i <= L; i++) {
    const float mx = filter_bias_row(s, i == 1, eo1[seq.get(i)], t10, t11, bl);
    nullsc = nullsc + filter_log(mx);
  }
  return filter_bias_end(nullsc, s, bl);
}

// stage 1 alone: the MSV filter's score in nats (*usc), true where the pair is past the MSV stage
WH_HD inline bool filter_stage1(int msv_raw, FilterLen fl, int base, float scale, FilterThr t, float *usc) {
  *usc = filter_msv_nats(msv_raw, fl.tjb, base, scale);
  return !(filter_bits(*usc, fl.nullsc) < t.x1);
}
// stage 2 of a pair past stage 1, with the bias filter: the MSV score against filtersc, at F1; *run_vit from the same
// score at F2.  (An overflowed MSV score, +infinity, passes both.)
WH_HD inline int filter_stage2_bias(float usc, float filtersc, FilterThr t, bool *run_vit) {
  *run_vit = false;
  const float s = filter_bits(usc, filtersc);
  if (s < t.x1) return kStageMSV;
  int st = kStageMSV | kStageBias;
  *run_vit = s < t.x2m;
  if (!*run_vit) st |= kStageVit;
  return st;
}

// stage 3 from the Viterbi filter's raw score (with the bias filter: fl.nullsc replaced by filtersc)
WH_HD inline int filter_stage3(int vit_raw, FilterLen fl, int base, float scale, FilterThr t) {
  const float vfsc = filter_vit_nats(vit_raw, fl.xmove, base, scale);
  const float s = filter_bits(vfsc, fl.nullsc);
  return kStageVitRan | (s < t.x2v ? 0 : kStageVit);
}
// stage 4 from the scoring kernels' fwd_bits = (Forward - null1) / ln 2 and filtersc - null1 in nats
WH_HD inline bool filter_stage4(float fwd_bits, float bias_nats, FilterThr t) {
  const float s = bias_nats == 0.f ? fwd_bits : fwd_bits - filter_div(bias_nats, kLog2);
  return !(s < t.x3);
}

// what ran unfiltered: a placeholder raw score for a sweep that did not run
enum { kVitNotRun = -32769 };

// ---- the scalar pipeline of one pair (host) ------------------------------------------------------------------------
// dsq: the query's residues, 0-based; rows: 14 (M + 1) bytes of scratch, 2-byte aligned
struct FilterPairOut { int stage; float bias_nats; int msv_raw, vit_raw; };

inline FilterPairOut filter_pair_host(const FilterModel &fm, const FilterThr &t, const uint8_t *dsq, int L, int16_t *rows, bool bias = false) {
  FilterPairOut r{0, 0.f, 0, kVitNotRun};
  if (L <= 0) return r;
  const int M = fm.M;
  const size_t W = (size_t)M + 1;
  FilterLen fl = filter_len(L);
  const CalibRow<const uint8_t> seq{dsq - 1, 1};
  CalibMSVPar mp = calib_msv_par(fm.msv);
  mp.tjb = fl.tjb;
  uint8_t *brow = reinterpret_cast<uint8_t *>(rows);
  r.msv_raw = calib_msv_core(M, mp, fm.msv.rb.data(), seq, L, CalibRow<uint8_t>{brow, 1}, CalibRow<uint8_t>{brow + W, 1});
  bool run_vit = false;
  if (!bias) r.stage = filter_stage12(r.msv_raw, fl, fm.msv.base, fm.msv.scale, t, &run_vit);
  else {
    float usc;
    if (filter_stage1(r.msv_raw, fl, fm.msv.base, fm.msv.scale, t, &usc)) {
      const float filtersc = filter_bias_score(fm.bias.eo1, fm.bias.t10, fm.bias.t11, filter_bias_len(L), seq, L);
      r.stage = filter_stage2_bias(usc, filtersc, t, &run_vit);
      r.bias_nats = filtersc - fl.nullsc;
      fl.nullsc = filtersc;              // the Viterbi stage scores against it
    }
  }
  if (run_vit) {
    CalibVitPar vp = calib_vit_par(fm.vit);
    vp.xNCJ_move = fl.xmove;
    r.vit_raw = calib_viterbi_core(M, vp, fm.vit.rw.data(), fm.vit.tw.data(), seq, L, CalibRow<int16_t>{rows + W, 1}, CalibRow<int16_t>{rows + 4 * W, 1});
    r.stage |= filter_stage3(r.vit_raw, fl, fm.vit.base, fm.vit.scale, t);
  }
  return r;
}

// ---- the device path (wh_filter.hip), as wh_host_filter.hip drives it ----------------------------------------------------
// Register classes: a model of up to 64 Q nodes runs with Q cells per lane; beyond the last class (3 072 nodes, the
// scoring kernels' own limit) a pair runs the scalar cores, one lane per pair, rows in HBM.
constexpr int kFilterQ[] = {2, 4, 8, 16, 32, 48};
constexpr int kFilterClasses = 6;
constexpr int kFilterMaxReg = 64 * 48;
inline int filter_class(int M) {
  for (int c = 0; c < kFilterClasses; c++) if (M <= 64 * kFilterQ[c]) return c;
  return -1;
}

// one model as the kernels read it.  Register classes: rb [Kp][Mpad] bytes (node k at k - 1; 255 behind M), rw [Kp][Mpad]
// and tw [8][Mpad] words (-32768 behind M), Mpad = 64 Q, all 16-byte aligned.  HBM class (Q = 0): the host's layouts,
// rb / rw [Kp][M + 1], tw [M + 1][8].
struct FilterDevModel {
  int M, Kp;
  int base_b, bias_b, tbm, tec;
  int base_w, xE_loop, xE_move;
  float scale_b, scale_w;
  FilterThr thr;
  unsigned long long rb, rw, tw;       // byte offsets into the table block
};

struct FilterArgs {
  const FilterDevModel *models;        // [H]
  const unsigned char *tables;
  const FilterLen *lens;               // [lmax + 1]
  int lmax;
  const uint8_t *residues;
  const long long *offsets;
  long long nq;
  int H;
  const int *list;                     // the launch's models (positions 0 .. H-1): pair p of the launch is query p % nq on model list[p / nq]
  uint8_t *stage;                      // [nq x H]
  float *bias_nats;                    // optional
  int *msv_raw, *vit_raw;              // optional
  // HBM class: one launch per model and chunk of queries
  unsigned char *ws;                   // rows: 14 (M + 1) bytes per lane, lane-interleaved
  long long q0, q1;
  int h;
};
// the kernels with the bias filter take two more tables (a type of its own: the arguments of the kernels without the
// stage are laid out as they were)
struct FilterBiasArgs : FilterArgs {
  const FilterBias *bias;              // [H]
  const FilterBiasLen *blens;          // [lmax + 1]
};

// the kernels exist twice: without the bias stage (the pipeline of --nobias), and with it (the _bias launchers: the same
// source compiled a second time into an object of its own, so that the first compiles exactly as it does without the stage)
int launch_filter_class(int cls, const FilterArgs &a, long long npairs, void *stream);
int launch_filter_hbm(const FilterArgs &a, void *stream);
int launch_filter_class_bias(int cls, const FilterBiasArgs &a, long long npairs, void *stream);
int launch_filter_hbm_bias(const FilterBiasArgs &a, void *stream);
// counts[0..3] += pairs, passed MSV, passed bias, passed Viterbi over stage[0 .. n)
int launch_filter_count(const uint8_t *stage, long long n, unsigned long long *counts, void *stream);

}  // namespace whf
