// hmmsearch --tblout (wh_seq_expect, wh_seq_table): what the counting sweep's kernels (wh_seqtab.hip), its float64 host
// replica and the row assembly on both sides (wh_host_seqtab.hip) share - the thresholds of HMMER's domain definition, the
// launch arguments, and the assembly of one row as ONE inline function that the kernel and the host run.  No HIP call and
// no device type in here: tools/seq_table_host_sanitize.cpp compiles it for the host alone.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "wh_common.h"

#if defined(__HIPCC__)
#define WH_SEQTAB_HD __host__ __device__ __forceinline__
#else
#define WH_SEQTAB_HD inline
#endif

namespace whs {

// HMMER's p7_domaindef defaults: a region starts where the non-homologous occupancy drops to 1 - rt1 and extends while it
// stays below 1 - rt2; a region is multidomain (stochastic clustering) where max_z min(E mass up to z, B mass from z) >= rt3
constexpr float kRt1 = 0.25f, kRt2 = 0.10f, kRt3 = 0.20f;

constexpr int kSeqWaves = 4;                 // waves of a workgroup of the register kernel: one pair each, one model's tables
constexpr int kSeqSpecArrays = 6;            // per-row arrays of a wave's HBM workspace: N, B, E, J, C, scale (SP_N .. SP_S)
constexpr int kSeqItemPairs = 64;            // pairs of one work item (one model)

// one work item of the register kernel: <n> pairs of model <h>, order[lo .. lo + n)
struct SeqItem { int32_t h, n; int64_t lo; };

struct SeqExpArgs {
  const void *hmms;            // DevHMM[H]
  const float *tables;         // float32 tables of the scoring kernels
  const double *gtab;          // float64 tables (any-size path)
  const uint8_t *residues;
  const int64_t *offsets;
  const int64_t *pair_list;    // [n_pairs] q * H + h
  const int64_t *order;        // positions of pair_list, grouped by model
  const SeqItem *items;
  int32_t n_items, H, K, Kp, Klds, Lcap, SP, seq_lds;   // Klds: emission rows staged in LDS (K or 0); seq_lds: bytes of a wave's residues in LDS (0: in its workspace)
  int32_t Qmax;                // any-size path: the largest cells-per-lane (sizes a wave's rows)
  float *ws;                   // per-wave workspace, <ws_stride> floats each: kSeqSpecArrays x SP floats, then the residues
  int64_t ws_stride;
  double *gws;                 // any-size path: per-wave workspace, <gws_stride> doubles
  int64_t gws_stride;
  int *counter;                // work-queue head
  wh_seq_expect_rec *out;      // [n_pairs]
};

struct SeqTabArgs {
  const uint8_t *flags;        // [npairs]
  const wh_pair_detail *detail;
  const int64_t *offsets;
  const float *evp;            // [H][2] tau, lambda (NaN: none)
  const wh_seq_expect_rec *expect;   // [rows]
  const int64_t *pair_list;    // [rows]
  int64_t npairs, rows;
  int32_t H;
  double lnE_Z, lnIncE_Z, lnDomE_domZ, lnIncDomE_domZ;   // ln(threshold / Z): a decision is lnP <= that
  wh_seq_row *out;
  unsigned long long *status;  // [4]: -, capped rows, reg mismatches, -
};

// HMMER's per-domain score (p7_pipeline.c) in its order of operations and its types, as wh_domains.hip computes it for the
// domain records (tests/test_tblout_gpu.py requires the two copies to give the same bits)
WH_SEQTAB_HD void seq_domain_score(float envsc, float domcorr, int L, int Ld, float tau, float lambda, float *bits, float *bias_bits,
                                   float *lnP) {
  const float bitscore = (float)((double)envsc + (double)(L - Ld) * log((double)((float)L / (float)(L + 3))));
  const float p1 = (float)L / (float)(L + 1);
  const float nullsc = (float)((double)(float)L * log((double)p1) + log(1.0 - (double)p1));
  const float x = (float)(log(1.0 / 256.0) + (double)domcorr);
  const float dombias = x > 0.f ? x + log1pf(expf(-x)) : log1pf(expf(x));
  const float b = (float)((double)(bitscore - (nullsc + dombias)) / 0.69314718055994529);
  *bits = b;
  *bias_bits = (float)((double)dombias / 0.69314718055994529);
  *lnP = (tau != tau || lambda != lambda) ? __builtin_nanf("") : (b < tau ? 0.f : (float)(-(double)lambda * ((double)b - (double)tau)));
}

// One row of the per-sequence table from the pair's detail record and the sweep's counts.  Returns reg mismatch | capped << 1.
WH_SEQTAB_HD int seq_table_row(int64_t pair, const wh_pair_detail &d, int L, float tau, float lambda, const wh_seq_expect_rec &x,
                               double lnE_Z, double lnIncE_Z, double lnDomE_domZ, double lnIncDomE_domZ, wh_seq_row *r) {
  const bool stats = tau == tau && lambda == lambda;
  const int n = d.nenv < WH_MAX_ENVELOPES ? (d.nenv > 0 ? d.nenv : 0) : WH_MAX_ENVELOPES;
  r->pair = pair;
  r->seq_bits = d.seq_score;
  r->seq_bias_bits = d.pre_score - d.seq_score > 0.f ? d.pre_score - d.seq_score : 0.f;
  const double slnP = !stats ? (double)__builtin_nanf("") : (d.seq_score < tau ? 0.0 : -(double)lambda * ((double)d.seq_score - (double)tau));
  r->seq_lnP = slnP;
  r->exp = x.exp; r->clu = x.clu; r->reg = d.nregions;
  r->env = n; r->dom = n;
  const bool seq_rep = !stats || slnP <= lnE_Z, seq_inc = !stats || slnP <= lnIncE_Z;
  int ov = 0, rep = 0, inc = 0, best = -1;
  float bb = 0.f, bbias = 0.f, blnP = 0.f;
  for (int t = 0; t < n; t++) {
    if (t >= 1 && d.env_i[t] <= d.env_j[t - 1]) ov++;
    float bits, bias, lnP;
    seq_domain_score(d.envsc[t], d.domcorr[t], L, d.env_j[t] - d.env_i[t] + 1, tau, lambda, &bits, &bias, &lnP);
    if (best < 0 || bits > bb) { best = t; bb = bits; bbias = bias; blnP = lnP; }
    if (seq_rep && (!stats || (double)lnP <= lnDomE_domZ)) rep++;
    if (seq_inc && (!stats || (double)lnP <= lnIncDomE_domZ)) inc++;
  }
  r->ov = ov; r->rep = rep; r->inc = inc;
  r->best = best; r->best_bits = bb; r->best_bias_bits = bbias; r->best_lnP = blnP;
  const int capped = (d.nenv >= WH_MAX_ENVELOPES || d.nregions > WH_MAX_ENVELOPES) ? 1 : 0;
  r->capped = capped; r->reserved = 0;
  return (x.reg != d.nregions ? 1 : 0) | (capped << 1);
}

// ---- the float64 host replica of the counting sweep (wh_seq_expect_host): plain scalar multihit local Forward and Backward
// over the configured profile (wh::configure_profile: the tables the kernels are built from), the posteriors, the cumulative
// sums and the region scan with the thresholds above.  Rows are rescaled as the float64 kernels rescale them.
inline wh_seq_expect_rec seq_expect_pair_host(const wh::HostHMM &h, const uint8_t *seq, int L) {
  enum { tMM = 0, tMI, tMD, tIM, tII, tDM, tDD };
  wh_seq_expect_rec out;
  out.exp = 0.f; out.reg = 0; out.clu = 0;
  if (L <= 0) return out;
  const int M = h.M;
  const size_t W = (size_t)M + 2;
  // the length model in float32, as HMMER evaluates it
  const float pmove = 3.0f / ((float)L + 3.0f), ploop = 1.0f - pmove;
  const double move = pmove, loop = ploop, EJ = 0.5, EC = 0.5, kBig = 1e60;
  auto pt = [&](int k, int x) -> double { return h.pt[(size_t)k * 7 + x]; };
  auto od = [&](int x, int k) -> double { return h.odds[(size_t)(x < h.Kp ? x : h.Kp - 1) * (M + 1) + k]; };
  const size_t R = (size_t)L + 1;
  std::vector<double> fN(R), fB(R), fE(R), fJ(R), fC(R), fS(R), bN(R), bB(R), bE(R), bJ(R), bC(R), bS(R);
  std::vector<double> Mp(W, 0.0), Ip(W, 0.0), Dp(W, 0.0), Mc(W, 0.0), Ic(W, 0.0), Dc(W, 0.0);
  double ls = 0.0;
  fN[0] = 1.0; fB[0] = move; fE[0] = 0.0; fJ[0] = 0.0; fC[0] = 0.0; fS[0] = 0.0;
  for (int i = 1; i <= L; i++) {
    const int x = seq[i - 1];
    double xe = 0.0;
    Mc[0] = Ic[0] = Dc[0] = 0.0;
    for (int k = 1; k <= M; k++) {
      Mc[k] = od(x, k) * (fB[(size_t)i - 1] * h.entry[(size_t)k] + Mp[k - 1] * pt(k - 1, tMM) + Ip[k - 1] * pt(k - 1, tIM) + Dp[k - 1] * pt(k - 1, tDM));
      Ic[k] = Mp[k] * pt(k, tMI) + Ip[k] * pt(k, tII);
      Dc[k] = Mc[k - 1] * pt(k - 1, tMD) + Dc[k - 1] * pt(k - 1, tDD);
      xe += Mc[k] + Dc[k];
    }
    double xn = fN[(size_t)i - 1] * loop, xc = fC[(size_t)i - 1] * loop + xe * EC, xj = fJ[(size_t)i - 1] * loop + xe * EJ;
    if (xe > kBig) {
      const double r = 1.0 / xe;
      for (int k = 1; k <= M; k++) { Mc[k] *= r; Ic[k] *= r; Dc[k] *= r; }
      xn *= r; xc *= r; xj *= r; ls += std::log(xe); xe = 1.0;
    }
    fN[(size_t)i] = xn; fE[(size_t)i] = xe; fJ[(size_t)i] = xj; fC[(size_t)i] = xc; fB[(size_t)i] = (xj + xn) * move; fS[(size_t)i] = ls;
    Mp.swap(Mc); Ip.swap(Ic); Dp.swap(Dc);
  }
  const double fwd = ls + std::log(fC[(size_t)L] * move);
  if (!std::isfinite(fwd) || !std::isfinite((float)fwd)) return out;
  // Backward: Mp / Ip hold row i + 1 (zero behind the last row), Mc / Ic / Dc receive row i
  std::fill(Mp.begin(), Mp.end(), 0.0); std::fill(Ip.begin(), Ip.end(), 0.0);
  double bs = 0.0, nN = 0.0, nJ = 0.0, nC = move;
  for (int i = L; i >= 0; i--) {
    double xb = 0.0, xj = 0.0, xc = move, xn = 0.0;
    if (i < L) {
      const int x = seq[i];
      for (int k = 1; k <= M; k++) xb += h.entry[(size_t)k] * od(x, k) * Mp[k];
      xj = nJ * loop + xb * move; xc = nC * loop; xn = nN * loop + xb * move;
    }
    double xe = xc * EC + xj * EJ;
    if (xb > kBig || xn > kBig) {
      const double big = xb > xn ? xb : xn, r = 1.0 / big;
      xb *= r; xj *= r; xc *= r; xn *= r; xe *= r; bs += std::log(big);
      for (int k = 1; k <= M; k++) { Mp[k] *= r; Ip[k] *= r; }
    }
    if (i >= 1) {
      const int x = i < L ? seq[i] : 0;
      double dnext = 0.0;
      Mc[(size_t)M + 1] = 0.0;
      for (int k = M; k >= 1; k--) {
        const double g = (k < M && i < L) ? od(x, k + 1) * Mp[k + 1] : 0.0;
        const double dv = xe + pt(k, tDM) * g + pt(k, tDD) * dnext;
        Mc[k] = xe + pt(k, tMM) * g + pt(k, tMI) * Ip[k] + pt(k, tMD) * dnext;
        Ic[k] = pt(k, tIM) * g + pt(k, tII) * Ip[k];
        dnext = dv;
      }
      Mp.swap(Mc); Ip.swap(Ic);
    }
    bN[(size_t)i] = xn; bB[(size_t)i] = xb; bE[(size_t)i] = xe; bJ[(size_t)i] = xj; bC[(size_t)i] = xc; bS[(size_t)i] = bs;
    nN = xn; nJ = xj; nC = xc;
  }
  // posteriors, cumulative sums, regions
  std::vector<double> mocc(R, 0.0), btot(R, 0.0), etot(R, 0.0);
  for (int i = 1; i <= L; i++) {
    const size_t a = (size_t)i - 1, b = (size_t)i;
    const double pb = fB[a] * bB[a] * std::exp(fS[a] + bS[a] - fwd);
    const double pe = fE[b] * bE[b] * std::exp(fS[b] + bS[b] - fwd);
    const double njc = (fN[a] * bN[b] + fJ[a] * bJ[b] + fC[a] * bC[b]) * loop * std::exp(fS[a] + bS[b] - fwd);
    mocc[b] = 1.0 - njc; btot[b] = btot[a] + pb; etot[b] = etot[a] + pe;
  }
  int i0 = -1, nreg = 0, clu = 0;
  bool trig = false;
  for (int j = 1; j <= L; j++) {
    const double m = mocc[(size_t)j];
    if (!trig) {
      if (m - (btot[(size_t)j] - btot[(size_t)j - 1]) < (double)kRt2) i0 = j;
      else if (i0 == -1) i0 = j;
      if (m >= (double)kRt1) trig = true;
    } else if (m - (etot[(size_t)j] - etot[(size_t)j - 1]) < (double)kRt2) {
      double mx = -1.0;
      for (int z = i0; z <= j; z++) {
        const double u = etot[(size_t)z] - etot[(size_t)i0 - 1], v = btot[(size_t)j] - btot[(size_t)z - 1];
        const double w = u < v ? u : v;
        mx = w > mx ? w : mx;
      }
      if (mx >= (double)kRt3) clu++;
      nreg++;
      i0 = -1; trig = false;
    }
  }
  out.exp = (float)btot[(size_t)L]; out.reg = nreg; out.clu = clu;
  return out;
}

// the assembly's host half: one row per reported pair, in pair order (wh_seq_table_host)
inline int64_t seq_table_rows_host(int H, const float *tau, const float *lambda, const int64_t *lengths, int64_t nq, const uint8_t *flags,
                                   const wh_pair_detail *detail, const wh_seq_expect_rec *expect, const wh_seq_table_opts &o,
                                   wh_seq_row *out, int64_t cap, int64_t status[4]) {
  const int64_t npairs = nq * H;
  int64_t rows = 0;
  for (int64_t p = 0; p < npairs; p++) rows += (flags[p] & WH_FLAG_REPORTED) ? 1 : 0;
  status[0] = rows; status[1] = status[2] = status[3] = 0;
  if (rows > cap) return -1;
  const double Z = o.Z > 0 ? o.Z : (double)nq, domZ = o.domZ > 0 ? o.domZ : (double)rows;
  const double lnE = std::log(o.E / Z), lnIncE = std::log(o.incE / Z), lnDomE = std::log(o.domE / domZ), lnIncDomE = std::log(o.incdomE / domZ);
  int64_t t = 0;
  for (int64_t p = 0; p < npairs; p++) {
    if (!(flags[p] & WH_FLAG_REPORTED)) continue;
    const int h = (int)(p % H);
    const int st = seq_table_row(p, detail[p], (int)lengths[p / H], tau[h], lambda[h], expect[t], lnE, lnIncE, lnDomE, lnIncDomE, out + t);
    status[1] += (st >> 1) & 1; status[2] += st & 1;
    t++;
  }
  return rows;
}

static_assert(sizeof(wh_seq_row) == 80 && sizeof(wh_seq_expect_rec) == 12, "the records' layout is part of the ABI (witch_amd/_lib.py)");

}  // namespace whs

// launchers of wh_seqtab.hip
namespace wh {
size_t seq_expect_lds_bytes(int Q, int Klds, int seq_lds);
int seq_expect_launch(int Q, const whs::SeqExpArgs &a, int blocks, size_t lds, void *stream);      // hipError_t as int
int seq_expect_any_launch(const whs::SeqExpArgs &a, int blocks, void *stream);
size_t seq_expect_any_doubles(int Lcap, int Qmax);
int seq_table_compact_launch(const uint8_t *flags, int64_t npairs, int64_t *list, unsigned long long *count, int64_t cap, void *stream);
int seq_table_rows_launch(const whs::SeqTabArgs &a, void *stream);
}  // namespace wh
