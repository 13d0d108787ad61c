// E-value calibration of a freshly built model: the three "STATS LOCAL" lines hmmbuild 3.1b2 writes
// (MSV mu, Viterbi mu, Forward tau, one lambda).  Restated from HMMER's published behaviour (p7_Calibrate:
// p7_Lambda, p7_MSVMu, p7_ViterbiMu, p7_Tau with the builder's defaults EmL = EvL = 200, EfL = 100, 200 sequences
// each, tail mass 0.04; the generator is re-seeded with 42 for every model) and pinned on the STATS lines of the
// model files under tests/golden (written by the reference's bundled hmmbuild).  WITCH never reads these numbers
// (hmmsearch runs with -E 99999999 and only bit scores are parsed, witch_msa/gcmm/algorithm.py:526-532,
// loader.py:293); they make a file written by wh_hmmbuild acceptable to stock HMMER (-p <hmmdir> reruns,
// witch_msa/gcmm/gcmm.py:163-171).
//
// What has to be reproduced exactly for the printed digits to come out:
//  * the random sequences: Easel's "fast" generator (x <- 69069 x + 1, Jenkins-mixed seed) and esl_rnd_FChoose over
//    the float background, 600 sequences drawn in one stream (MSV, then Viterbi, then Forward);
//  * the MSV filter's 8-bit arithmetic (third-bit units, base 190, saturating unsigned adds / subtracts) and the
//    Viterbi filter's 16-bit arithmetic (1/500-bit units, base 12000, saturating signed adds): both are integer
//    dynamic programmes, so a scalar restatement gives the striped SSE code's numbers;
//  * the Forward score only enters a maximum-likelihood Gumbel fit of 200 values: float64 here against HMMER's
//    float32 parser moves tau in its fifth decimal at most.
//
// One source for the host and the device: the three dynamic programmes (calib_msv_core, calib_viterbi_core,
// calib_forward_core) are plain functions over row / table accessors, marked WH_HD, and hold no container.  The host
// path (calibrate_model) runs them over vectors with stride 1; wh_calibrate.hip runs the same functions with one lane
// per (model, sequence) over lane-interleaved rows in HBM.  The overflow exits of the two filters (xE + bias == 255,
// xE >= 32767) are not reachable with the seeded sequences, so no test can cover them on either side: they are the
// same statements on both.  Everything with a libm call in it (profile conversion, exp tables, the final log, the
// Gumbel fits) is host code, before and after the sweeps.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define WH_HD __host__ __device__
#else
#define WH_HD
#endif
#if defined(__clang__)
#define WH_UNROLL _Pragma("unroll")
#else
#define WH_UNROLL
#endif

namespace whc {

enum { tMM = 0, tMI, tMD, tIM, tII, tDM, tDD };

// hmmbuild's defaults: 200 sequences per filter; MSV and Viterbi on 200 residues, Forward on 100
enum { kCalibN = 200, kCalibEmL = 200, kCalibEvL = 200, kCalibEfL = 100 };

// The sweeps read row i-1 kCalibChunk nodes at a time, all loads of a chunk ahead of its first store: on the device the
// loads are in flight together instead of one memory latency per node.  Data movement only: the cells are computed in
// the same order from the same values, whatever the chunk.
enum { kCalibChunk = 8 };

// element k of a row (or of a sequence) that is <stride> elements apart: 1 on the host, the lanes of a launch on the device
template <class T> struct CalibRow {
  T *p;
  size_t stride;
  WH_HD T get(int k) const { return p[(size_t)k * stride]; }
  WH_HD void set(int k, T v) const { p[(size_t)k * stride] = v; }
  WH_HD CalibRow plus(size_t elems) const { return CalibRow{p + elems * stride, stride}; }
};


template <class T> WH_HD inline T calib_max(T a, T b) { return a < b ? b : a; }

struct CalibModel {
  int M, K;
  const float *t;      // [M+1][7]  node 0 = begin
  const float *mat;    // [M+1][K]
  const float *bg;     // [K]
};

struct CalibRng {
  uint32_t x;
  static uint32_t mix3(uint32_t a, uint32_t b, uint32_t c) {
    a -= b; a -= c; a ^= (c >> 13);
    b -= c; b -= a; b ^= (a << 8);
    c -= a; c -= b; c ^= (b >> 13);
    a -= b; a -= c; a ^= (c >> 12);
    b -= c; b -= a; b ^= (a << 16);
    c -= a; c -= b; c ^= (b >> 5);
    a -= b; a -= c; a ^= (c >> 3);
    b -= c; b -= a; b ^= (a << 10);
    c -= a; c -= b; c ^= (b >> 15);
    return c;
  }
  explicit CalibRng(uint32_t seed) { x = mix3(seed, 87654321u, 12345678u); if (x == 0) x = 42; }
  double next() { x = x * 69069u + 1u; return (double)x / 4294967296.0; }
  // esl_rnd_FChoose over K float probabilities (first i whose running sum / total exceeds the roll, in double)
  int choose(const float *p, int K) {
    const double roll = next();
    double norm = 0.0, sum = 0.0;
    for (int i = 0; i < K; i++) norm += p[i];
    for (int i = 0; i < K; i++) { sum += p[i]; if (sum / norm > roll) return i; }
    return K - 1;
  }
};

// The 600 sequences of one calibration: the generator is re-seeded with 42 for every model and draws from the
// background alone, so they are the same for every model of an alphabet.  s[0] MSV, s[1] Viterbi, s[2] Forward, each
// [kCalibN][L + 2] with the residues at 1 .. L.
struct CalibSeqs {
  int L[3];
  std::vector<uint8_t> s[3];
  const uint8_t *seq(int phase, int i) const { return s[phase].data() + (size_t)i * (size_t)(L[phase] + 2); }
};

inline void calib_draw(const float *bg, int K, CalibSeqs &q) {
  CalibRng rng(42u);
  q.L[0] = kCalibEmL; q.L[1] = kCalibEvL; q.L[2] = kCalibEfL;
  for (int ph = 0; ph < 3; ph++) {
    const int L = q.L[ph];
    q.s[ph].assign((size_t)kCalibN * (size_t)(L + 2), 0);
    for (int n = 0; n < kCalibN; n++)
      for (int i = 1; i <= L; i++) q.s[ph][(size_t)n * (size_t)(L + 2) + (size_t)i] = (uint8_t)rng.choose(bg, K);
  }
}

// the float32 log-odds profile p7_ProfileConfig builds in local multihit mode (what the optimized profile is converted from)
struct CalibProfile {
  int M, K;
  std::vector<float> msc;   // [M+1][K]   match emission scores
  std::vector<float> tsc;   // [M][7]     node k -> k+1 transitions, k = 0 .. M-1 (node 0: all -inf)
  std::vector<float> bm;    // [M]        B -> M_{k+1}, stored at k
};

inline void calib_profile(const CalibModel &h, CalibProfile &gm) {
  const int M = h.M, K = h.K;
  const float ninf = -INFINITY;
  gm.M = M; gm.K = K;
  gm.msc.assign((size_t)(M + 1) * K, ninf);
  gm.tsc.assign((size_t)M * 7, ninf);
  gm.bm.assign((size_t)M, ninf);
  // p7_hmm_CalculateOccupancy
  std::vector<float> occ((size_t)M + 1, 0.f);
  occ[1] = h.t[tMI] + h.t[tMM];
  for (int k = 2; k <= M; k++) {
    const float *tp = h.t + (size_t)(k - 1) * 7;
    occ[k] = (float)(occ[k - 1] * (tp[tMM] + tp[tMI]) + (1.0 - occ[k - 1]) * tp[tDM]);     // (HMMER's literal 1.0 is a double)
  }
  float Z = 0.f;
  for (int k = 1; k <= M; k++) Z += occ[k] * (float)(M - k + 1);
  for (int k = 1; k <= M; k++) gm.bm[(size_t)k - 1] = (float)std::log((double)(occ[k] / Z));
  for (int k = 1; k < M; k++)
    for (int z = 0; z < 7; z++) gm.tsc[(size_t)k * 7 + z] = (float)std::log((double)h.t[(size_t)k * 7 + z]);
  for (int k = 1; k <= M; k++)
    for (int x = 0; x < K; x++) gm.msc[(size_t)k * K + x] = (float)std::log((double)h.mat[(size_t)k * K + x] / (double)h.bg[x]);
}

// p7_bg_NullOne at length L
inline float calib_nullone(int L) {
  const float p1 = (float)L / (float)(L + 1);
  return (float)((float)L * std::log((double)p1) + std::log(1. - (double)p1));
}

// ---- MSV filter (8-bit) ------------------------------------------------------------------------------------
struct CalibMSV {
  int M, K;
  float scale;
  uint8_t base, bias, tbm, tec, tjb;
  std::vector<uint8_t> rb;   // [K][M+1] biased match costs
  uint8_t unbiased(float sc) const { sc = -1.0f * roundf(scale * sc); return sc > 255.f ? 255 : (uint8_t)sc; }
  // (a positive score is a negative cost: through int, so that the wrap-around HMMER's byte arithmetic relies on is defined)
  uint8_t biased(float sc) const { sc = -1.0f * roundf(scale * sc); return sc > (float)(255 - bias) ? 255 : (uint8_t)((uint8_t)(int)sc + bias); }
};

inline void calib_msv_convert(const CalibProfile &gm, CalibMSV &om) {
  const int M = gm.M, K = gm.K;
  om.M = M; om.K = K;
  float mx = 0.0f;       // (the insert scores, all 0, are part of the maximum)
  for (int k = 1; k <= M; k++) for (int x = 0; x < K; x++) mx = std::max(mx, gm.msc[(size_t)k * K + x]);
  om.scale = (float)(3.0 / 0.69314718055994529);
  om.base = 190;
  om.bias = om.unbiased(-1.0f * mx);
  om.rb.assign((size_t)K * (M + 1), 255);
  for (int x = 0; x < K; x++) for (int k = 1; k <= M; k++) om.rb[(size_t)x * (M + 1) + k] = om.biased(gm.msc[(size_t)k * K + x]);
  om.tbm = om.unbiased(logf(2.0f / ((float)M * (float)(M + 1))));
  om.tec = om.unbiased(logf(0.5f));
  om.tjb = 0;
}

WH_HD inline uint8_t sat_addu8(uint8_t a, uint8_t b) { const int s = (int)a + (int)b; return s > 255 ? 255 : (uint8_t)s; }
WH_HD inline uint8_t sat_subu8(uint8_t a, uint8_t b) { return a > b ? (uint8_t)(a - b) : 0; }

// the filter's scalars, as the sweep takes them
struct CalibMSVPar { uint8_t base, bias, tbm, tec, tjb; };

// The empty diagonal.  HMMER 3.1b2 answers the MSV filter from a single-hit pre-filter over ungapped diagonals wherever
// that can stand for it, and the pre-filter's best diagonal may be the EMPTY one, worth 0: xE is then xB itself,
// base - tjb - tbm, where the sweep below always pays for at least one emitted residue.  The two differ only on a query
// no residue of which scores 0 or better on any node; every other outcome of the pre-filter (a hit that J could extend, an
// overflow) is the sweep's own.  The pre-filter stands aside where tjb + tbm + tec + bias >= 127 - a condition on the model
// AND the query's length: the sweep's value is then final.  Read off the bundled hmmsearch alone: the recovered integers of
// tests/golden/filters/classes_* ("the empty diagonal").  0 where the rule does not apply.
WH_HD inline int calib_msv_floor(int base, int bias, int tbm, int tec, int tjb) {
  const int cost = tjb + tbm + tec;
  return cost + bias >= 127 ? 0 : base - cost;
}

// The sweep: rb [K][M+1] (any pointer: host memory, LDS, HBM), dsq residues 1 .. L, two rows r0 / r1 of M+1 bytes that
// it ping-pongs (the loads of row i-1 never alias the stores of row i).  Returns xJ - at least the empty diagonal's
// (calib_msv_floor) -, or -1 where the filter overflows (p7_MSVMu then takes the filter's ceiling: calib_msv_score).
template <class Tab, class Seq, class Row>
WH_HD inline int calib_msv_core(int M, CalibMSVPar om, Tab rb, Seq dsq, int L, Row r0, Row r1) {
  for (int k = 0; k <= M; k++) r0.set(k, 0);
  const uint8_t tjbm = (uint8_t)((int8_t)om.tjb + (int8_t)om.tbm);
  uint8_t xJ = 0, xB = sat_subu8(om.base, tjbm);
  for (int i = 1; i <= L; i++) {
    const Tab rsc = rb + (size_t)dsq.get(i) * (size_t)(M + 1);
    uint8_t xE = 0, prev = 0;          // prev = M(i-1, k-1); node 0 is -infinity (0)
    auto cell = [&](int k, uint8_t up) {      // up = M(i-1, k)
      uint8_t sv = calib_max(prev, xB);
      sv = sat_addu8(sv, om.bias);
      sv = sat_subu8(sv, rsc[k]);
      xE = calib_max(xE, sv);
      prev = up;
      r1.set(k, sv);
    };
    int k = 1;
    for (; k + kCalibChunk <= M + 1; k += kCalibChunk) {
      uint8_t up[kCalibChunk];
      WH_UNROLL for (int j = 0; j < kCalibChunk; j++) up[j] = r0.get(k + j);
      WH_UNROLL for (int j = 0; j < kCalibChunk; j++) cell(k + j, up[j]);
    }
    for (; k <= M; k++) cell(k, r0.get(k));
    if (sat_addu8(xE, om.bias) == 255) return -1;
    xE = sat_subu8(xE, om.tec);
    xJ = calib_max(xJ, xE);
    xB = calib_max(om.base, xJ);
    xB = sat_subu8(xB, tjbm);
    const Row t = r0; r0 = r1; r1 = t;
  }
  return calib_max((int)xJ, calib_msv_floor(om.base, om.bias, om.tbm, om.tec, om.tjb));
}

// score in nats; overflow returns the filter's ceiling like p7_MSVMu does
inline float calib_msv_score(const CalibMSV &om, int raw) {
  if (raw < 0) return (float)(255 - om.base) / om.scale;
  float sc = (float)(raw - (int)om.tjb) - (float)om.base;
  sc /= om.scale;
  sc -= 3.0f;
  return sc;
}

// ---- Viterbi filter (16-bit) -------------------------------------------------------------------------------
struct CalibVit {
  int M, K;
  float scale;
  int16_t base;
  std::vector<int16_t> rw;    // [K][M+1]
  std::vector<int16_t> tw;    // [M+1][8]: BM MM IM DM (into node k, from k-1), MD MI II DD (out of node k)
  int16_t xE_loop, xE_move, xNCJ_move;
  int16_t wordify(float sc) const {
    sc = roundf(scale * sc);
    if (sc >= 32767.0f) return 32767;
    if (sc <= -32768.0f) return -32768;
    return (int16_t)sc;
  }
};
enum { vBM = 0, vMM, vIM, vDM, vMD, vMI, vII, vDD };

inline void calib_vit_convert(const CalibProfile &gm, CalibVit &om) {
  const int M = gm.M, K = gm.K;
  om.M = M; om.K = K;
  om.scale = (float)(500.0 / 0.69314718055994529);
  om.base = 12000;
  om.rw.assign((size_t)K * (M + 1), -32768);
  for (int x = 0; x < K; x++) for (int k = 1; k <= M; k++) om.rw[(size_t)x * (M + 1) + k] = om.wordify(gm.msc[(size_t)k * K + x]);
  om.tw.assign((size_t)(M + 1) * 8, -32768);
  auto cap = [](int16_t v, int16_t mx) { return v <= mx ? v : mx; };
  for (int k = 1; k <= M; k++) {
    int16_t *tp = &om.tw[(size_t)k * 8];
    const int kb = k - 1;      // the incoming transitions live at node k-1 of the profile
    tp[vBM] = cap(om.wordify(gm.bm[(size_t)kb]), 0);
    tp[vMM] = cap(om.wordify(gm.tsc[(size_t)kb * 7 + tMM]), 0);
    tp[vIM] = cap(om.wordify(gm.tsc[(size_t)kb * 7 + tIM]), 0);
    tp[vDM] = cap(om.wordify(gm.tsc[(size_t)kb * 7 + tDM]), 0);
    if (k < M) {
      tp[vMD] = cap(om.wordify(gm.tsc[(size_t)k * 7 + tMD]), 0);
      tp[vMI] = cap(om.wordify(gm.tsc[(size_t)k * 7 + tMI]), 0);
      tp[vII] = cap(om.wordify(gm.tsc[(size_t)k * 7 + tII]), -1);
      tp[vDD] = om.wordify(gm.tsc[(size_t)k * 7 + tDD]);
    }
  }
  om.xE_loop = om.wordify(-0.69314718055994529f);
  om.xE_move = om.wordify(-0.69314718055994529f);
  om.xNCJ_move = 0;
}

WH_HD inline int16_t sat_add16(int16_t a, int16_t b) { const int s = (int)a + (int)b; return s > 32767 ? 32767 : s < -32768 ? -32768 : (int16_t)s; }

struct CalibVitPar { int16_t base, xE_loop, xE_move, xNCJ_move; };
enum { kCalibVitOverflow = 32768 };

// The sweep: rw [K][M+1], tw [M+1][8]; a / b: two sets of three rows (M, I, D; M+1 words each, one after the other)
// that it ping-pongs.  Only nodes 1 .. M of a row are ever read.  Returns xC (-32768: no path), or kCalibVitOverflow
// where the filter overflows (calib_vit_score).
template <class Tab, class Seq, class Row>
WH_HD inline int calib_viterbi_core(int M, CalibVitPar om, Tab rw, Tab tw, Seq dsq, int L, Row a, Row b) {
  const size_t W = (size_t)M + 1;
  for (int k = 0; k < 3 * (M + 1); k++) a.set(k, -32768);
  int16_t xN = om.base, xB = (int16_t)((int)xN + (int)om.xNCJ_move), xJ = -32768, xC = -32768, xE;
  for (int i = 1; i <= L; i++) {
    const Tab rsc = rw + (size_t)dsq.get(i) * W;
    const Row pM = a, pI = a.plus(W), pD = a.plus(2 * W);
    const Row cM = b, cI = b.plus(W), cD = b.plus(2 * W);
    int16_t pm = -32768, pi_ = -32768, pd = -32768;     // row i-1 at node k-1
    int16_t dcv = -32768;                               // D(i,k): M(i,k-1) + MD, closed over DD below
    xE = -32768;
    auto cell = [&](int k, int16_t um, int16_t ui, int16_t ud) {      // um, ui, ud = M, I, D of row i-1 at node k
      const Tab tp = tw + (size_t)k * 8;
      int16_t sv = sat_add16(xB, tp[vBM]);
      sv = calib_max(sv, sat_add16(pm, tp[vMM]));
      sv = calib_max(sv, sat_add16(pi_, tp[vIM]));
      sv = calib_max(sv, sat_add16(pd, tp[vDM]));
      sv = sat_add16(sv, rsc[k]);
      xE = calib_max(xE, sv);
      pm = um; pi_ = ui; pd = ud;
      cM.set(k, sv);
      // D(i,k) = max(M(i,k-1) + MD(k-1), D(i,k-1) + DD(k-1)): the lazy-F passes of the SSE code reach this closure
      cD.set(k, dcv);
      const int16_t fromD = sat_add16(dcv, tp[vDD]);
      dcv = calib_max(sat_add16(sv, tp[vMD]), fromD);
      cI.set(k, calib_max(sat_add16(pm, tp[vMI]), sat_add16(pi_, tp[vII])));
    };
    int k = 1;
    for (; k + kCalibChunk <= M + 1; k += kCalibChunk) {
      int16_t um[kCalibChunk], ui[kCalibChunk], ud[kCalibChunk];
      WH_UNROLL for (int j = 0; j < kCalibChunk; j++) { um[j] = pM.get(k + j); ui[j] = pI.get(k + j); ud[j] = pD.get(k + j); }
      WH_UNROLL for (int j = 0; j < kCalibChunk; j++) cell(k + j, um[j], ui[j], ud[j]);
    }
    for (; k <= M; k++) cell(k, pM.get(k), pI.get(k), pD.get(k));
    if (xE >= 32767) return kCalibVitOverflow;
    // NN = CC = JJ = 0 (the -3 nat approximation)
    xC = (int16_t)calib_max((int)xC, (int)xE + (int)om.xE_move);
    xJ = (int16_t)calib_max((int)xJ, (int)xE + (int)om.xE_loop);
    xB = (int16_t)calib_max((int)xJ + (int)om.xNCJ_move, (int)xN + (int)om.xNCJ_move);
    const Row t = a; a = b; b = t;
  }
  return (int)xC;
}

inline float calib_vit_score(const CalibVit &om, int raw) {
  if (raw == kCalibVitOverflow) return (32767.0f - (float)om.base) / om.scale;
  if (raw > -32768) {
    float sc = (float)(int16_t)raw + (float)om.xNCJ_move - (float)om.base;
    sc /= om.scale;
    sc -= 3.0f;
    return sc;
  }
  return -INFINITY;
}

// ---- Forward, local multihit, length model L (float64, scaled rows) ------------------------------------------
// probabilities from the float scores, as the optimized profile holds them
enum { fMM = 0, fIM, fDM, fBM, fMD, fMI, fII, fDD };
struct CalibFwd {
  int M, K;
  std::vector<double> ft;    // [M+1][8]: MM IM DM BM (into node k), MD MI II DD (out of node k)
  std::vector<double> em;    // [K][M+1]: exp(match emission score)
  double pmove, ploop;
};

inline void calib_fwd_convert(const CalibProfile &gm, int L, CalibFwd &f) {
  const int M = gm.M, K = gm.K;
  f.M = M; f.K = K;
  f.ft.assign((size_t)(M + 1) * 8, 0.0);
  f.em.assign((size_t)K * (M + 1), 0.0);
  for (int k = 1; k <= M; k++) {
    const int kb = k - 1;
    double *tp = &f.ft[(size_t)k * 8];
    tp[fBM] = std::exp((double)gm.bm[(size_t)kb]);
    tp[fMM] = std::exp((double)gm.tsc[(size_t)kb * 7 + tMM]);
    tp[fIM] = std::exp((double)gm.tsc[(size_t)kb * 7 + tIM]);
    tp[fDM] = std::exp((double)gm.tsc[(size_t)kb * 7 + tDM]);
    if (k < M) {
      tp[fMD] = std::exp((double)gm.tsc[(size_t)k * 7 + tMD]);
      tp[fMI] = std::exp((double)gm.tsc[(size_t)k * 7 + tMI]);
      tp[fII] = std::exp((double)gm.tsc[(size_t)k * 7 + tII]);
      tp[fDD] = std::exp((double)gm.tsc[(size_t)k * 7 + tDD]);
    }
    for (int x = 0; x < K; x++) f.em[(size_t)x * (M + 1) + k] = std::exp((double)gm.msc[(size_t)k * K + x]);
  }
  const float pmove_f = 3.0f / ((float)L + 3.0f), ploop_f = 1.0f - pmove_f;
  f.pmove = pmove_f; f.ploop = ploop_f;
}

// The sweep: float64 multiplies and adds in one fixed order, never fused (a fused multiply-add rounds once where the
// host rounds twice), so the device's values are the host's to the bit.  a / b: two sets of three rows (M, I, D) of M+1
// doubles; only nodes 1 .. M are read.  A row whose sums leave the double range is rescaled by s; the factors go to
// scales[0 .. *nscale) and the host takes their logarithms (calib_forward_score).  Returns xC * pmove.
template <class Tab, class Seq, class Row, class Sc>
WH_HD inline double calib_forward_core(int M, Tab ft, Tab em, double pmove, double ploop, Seq dsq, int L, Row a, Row b, Sc scales, int *nscale) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const size_t W = (size_t)M + 1;
  double xN = 1.0, xB = pmove, xJ = 0.0, xC = 0.0;
  int ns = 0;
  for (int k = 0; k < 3 * (M + 1); k++) a.set(k, 0.0);
  for (int i = 1; i <= L; i++) {
    const Tab esc = em + (size_t)dsq.get(i) * W;
    const Row pM = a, pI = a.plus(W), pD = a.plus(2 * W);
    const Row cM = b, cI = b.plus(W), cD = b.plus(2 * W);
    double xE = 0.0;
    double pm1 = 0.0, pi1 = 0.0, pd1 = 0.0;      // row i-1 at node k-1 (node 0: 0)
    double cm1 = 0.0, cd1 = 0.0, tmd1 = 0.0, tdd1 = 0.0;      // row i at node k-1, and that node's MD / DD
    auto cell = [&](int k, double um, double ui, double ud) {      // um, ui, ud = M, I, D of row i-1 at node k
      const Tab tp = ft + (size_t)k * 8;
      const double e = esc[k];
      const double m = e * (xB * tp[fBM] + pm1 * tp[fMM] + pi1 * tp[fIM] + pd1 * tp[fDM]);
      pm1 = um; pi1 = ui; pd1 = ud;
      cM.set(k, m);
      cI.set(k, k < M ? pm1 * tp[fMI] + pi1 * tp[fII] : 0.0);
      const double d = k > 1 ? cm1 * tmd1 + cd1 * tdd1 : 0.0;
      cD.set(k, d);
      xE += m + d;
      cm1 = m; cd1 = d; tmd1 = tp[fMD]; tdd1 = tp[fDD];
    };
    int k = 1;
    for (; k + kCalibChunk <= M + 1; k += kCalibChunk) {
      double um[kCalibChunk], ui[kCalibChunk], ud[kCalibChunk];
      WH_UNROLL for (int j = 0; j < kCalibChunk; j++) { um[j] = pM.get(k + j); ui[j] = pI.get(k + j); ud[j] = pD.get(k + j); }
      WH_UNROLL for (int j = 0; j < kCalibChunk; j++) cell(k + j, um[j], ui[j], ud[j]);
    }
    for (; k <= M; k++) cell(k, pM.get(k), pI.get(k), pD.get(k));
    xJ = xJ * ploop + xE * 0.5;
    xC = xC * ploop + xE * 0.5;
    xN = xN * ploop;
    xB = (xN + xJ) * pmove;
    if (xE > 1e100 || (xE > 0.0 && xE < 1e-100) || xN < 1e-250) {
      const double s = 1.0 / calib_max(calib_max(xE, xN), calib_max(xJ, xC));
      for (int k = 1; k <= M; k++) { cM.set(k, cM.get(k) * s); cI.set(k, cI.get(k) * s); cD.set(k, cD.get(k) * s); }
      xN *= s; xB *= s; xJ *= s; xC *= s;
      scales.set(ns++, s);
    }
    const Row t = a; a = b; b = t;
  }
  *nscale = ns;
  return xC * pmove;
}

// the Forward score in nats from what the sweep returns
inline double calib_forward_score(double xCp, const double *scales, size_t stride, int nscale) {
  double logscale = 0.0;
  for (int j = 0; j < nscale; j++) logscale -= std::log(scales[(size_t)j * stride]);
  return std::log(xCp) + logscale;
}

// ---- Gumbel fits (Easel) -----------------------------------------------------------------------------------
inline double calib_fit_loc(const std::vector<double> &x, double lambda) {
  double esum = 0.0;
  for (double v : x) esum += std::exp(-lambda * v);
  return -std::log(esum / (double)x.size()) / lambda;
}

inline void calib_fit_complete(const std::vector<double> &x, double &mu, double &lambda) {
  const int n = (int)x.size();
  double sum = 0.0, sqsum = 0.0;
  for (double v : x) { sum += v; sqsum += v * v; }
  const double variance = (sqsum - sum * sum / (double)n) / ((double)n - 1.0);
  lambda = 3.14159265358979323846264338328 / std::sqrt(6. * variance);
  auto lawless416 = [&](double lam, double &f, double &df) {
    double esum = 0., xesum = 0., xxesum = 0., xsum = 0.;
    for (double v : x) {
      xsum += v;
      xesum += v * std::exp(-1. * lam * v);
      xxesum += v * v * std::exp(-1. * lam * v);
      esum += std::exp(-1. * lam * v);
    }
    f = (1. / lam) - (xsum / n) + (xesum / esum);
    df = ((xesum / esum) * (xesum / esum)) - (xxesum / esum) - (1. / (lam * lam));
  };
  double fx = 0., dfx = 0.;
  int i;
  for (i = 0; i < 100; i++) {
    lawless416(lambda, fx, dfx);
    if (std::fabs(fx) < 1e-5) break;
    lambda = lambda - fx / dfx;
    if (lambda <= 0.) lambda = 0.001;
  }
  if (i == 100) {      // Newton/Raphson failed: bisection, as Easel does
    double left = 0., right = 3.14159265358979323846264338328 / std::sqrt(6. * variance);
    lawless416(lambda, fx, dfx);
    while (fx > 0.) { right *= 2.; if (right > 100.) break; lawless416(right, fx, dfx); }
    for (i = 0; i < 100; i++) {
      const double mid = (left + right) / 2.;
      lawless416(mid, fx, dfx);
      if (std::fabs(fx) < 1e-5) { lambda = mid; break; }
      if (fx > 0.) left = mid; else right = mid;
      lambda = mid;
    }
  }
  double esum = 0.;
  for (double v : x) esum += std::exp(-lambda * v);
  mu = -std::log(esum / n) / lambda;
}

// ---- one model: what the host prepares, and what it does with the sweeps' results ---------------------------
struct CalibPrep {
  CalibMSV msv;
  CalibVit vit;
  CalibFwd fwd;
  double lambda;
};

inline void calib_prepare(const CalibModel &h, double meanrelent_bits, CalibPrep &p) {
  const double LOG2 = 0.69314718055994529;
  CalibProfile gm;
  calib_profile(h, gm);
  p.lambda = LOG2 + 1.44 / ((double)h.M * meanrelent_bits);
  calib_msv_convert(gm, p.msv);
  p.msv.tjb = p.msv.unbiased(logf(3.0f / (float)(kCalibEmL + 3)));
  calib_vit_convert(gm, p.vit);
  p.vit.xNCJ_move = p.vit.wordify(logf(3.0f / ((float)kCalibEvL + 3.0f)));
  calib_fwd_convert(gm, kCalibEfL, p.fwd);
}

inline CalibMSVPar calib_msv_par(const CalibMSV &om) { return CalibMSVPar{om.base, om.bias, om.tbm, om.tec, om.tjb}; }
inline CalibVitPar calib_vit_par(const CalibVit &om) { return CalibVitPar{om.base, om.xE_loop, om.xE_move, om.xNCJ_move}; }

// msv / vit: the kCalibN raw results of the two filters; fwd: the kCalibN Forward scores in nats (calib_forward_score).
// out: lambda, MSV mu, Viterbi mu, Forward tau
inline void calib_finish(const CalibPrep &p, const int *msv, const int *vit, const double *fwd, double out[4]) {
  const double LOG2 = 0.69314718055994529;
  const double Eft = 0.04;
  const double lambda = p.lambda;
  std::vector<double> xv;
  {
    const float nullsc = calib_nullone(kCalibEmL);
    for (int i = 0; i < kCalibN; i++) xv.push_back((double)(calib_msv_score(p.msv, msv[i]) - nullsc) / LOG2);
  }
  const double mmu = calib_fit_loc(xv, lambda);
  {
    const float nullsc = calib_nullone(kCalibEvL);
    xv.clear();
    for (int i = 0; i < kCalibN; i++) xv.push_back((double)(calib_vit_score(p.vit, vit[i]) - nullsc) / LOG2);
  }
  const double vmu = calib_fit_loc(xv, lambda);
  {
    const float nullsc = calib_nullone(kCalibEfL);
    xv.clear();
    for (int i = 0; i < kCalibN; i++) xv.push_back((double)((float)fwd[i] - nullsc) / LOG2);
  }
  double gmu, glam;
  calib_fit_complete(xv, gmu, glam);
  const double tau = (gmu - std::log(-1. * std::log(1.0 - Eft)) / glam) + (std::log(Eft) / lambda);
  out[0] = lambda; out[1] = mmu; out[2] = vmu; out[3] = tau;
}

// the three sweeps of one prepared model on the host, sequence after sequence
inline void calib_sweeps_host(const CalibPrep &p, const CalibSeqs &q, int *msv, int *vit, double *fwd) {
  const int M = p.msv.M;
  const size_t W = (size_t)M + 1;
  typedef CalibRow<const uint8_t> Seq;
  {
    std::vector<uint8_t> dp(2 * W);
    for (int i = 0; i < kCalibN; i++)
      msv[i] = calib_msv_core(M, calib_msv_par(p.msv), p.msv.rb.data(), Seq{q.seq(0, i), 1}, q.L[0],
                              CalibRow<uint8_t>{dp.data(), 1}, CalibRow<uint8_t>{dp.data() + W, 1});
  }
  {
    std::vector<int16_t> mx(6 * W);
    for (int i = 0; i < kCalibN; i++)
      vit[i] = calib_viterbi_core(M, calib_vit_par(p.vit), p.vit.rw.data(), p.vit.tw.data(), Seq{q.seq(1, i), 1}, q.L[1],
                                  CalibRow<int16_t>{mx.data(), 1}, CalibRow<int16_t>{mx.data() + 3 * W, 1});
  }
  {
    std::vector<double> w(6 * W), sc((size_t)q.L[2]);
    for (int i = 0; i < kCalibN; i++) {
      int ns = 0;
      const double xCp = calib_forward_core(M, p.fwd.ft.data(), p.fwd.em.data(), p.fwd.pmove, p.fwd.ploop, Seq{q.seq(2, i), 1}, q.L[2],
                                            CalibRow<double>{w.data(), 1}, CalibRow<double>{w.data() + 3 * W, 1}, CalibRow<double>{sc.data(), 1}, &ns);
      fwd[i] = calib_forward_score(xCp, sc.data(), 1, ns);
    }
  }
}

// lambda, MSV mu, Viterbi mu, Forward tau
inline void calibrate_model(const CalibModel &h, double meanrelent_bits, double out[4]) {
  CalibPrep p;
  calib_prepare(h, meanrelent_bits, p);
  CalibSeqs q;
  calib_draw(h.bg, h.K, q);
  int msv[kCalibN], vit[kCalibN];
  double fwd[kCalibN];
  calib_sweeps_host(p, q, msv, vit, fwd);
  calib_finish(p, msv, vit, fwd, out);
}

}  // namespace whc
