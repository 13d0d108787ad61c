// hmmsearch --tblout: the counts of HMMER's domain definition that the scoring kernels do not export (wh_seq_expect_dev), and
// the two small kernels of the row assembly (wh_seq_table_dev).  Purely additive: nothing here is called by a scoring call.
//
//   seq_expect_kernel<Q>   models of up to 3 072 nodes, one instantiation per cells-per-lane class (4 .. 48).  One wavefront
//                          per pair, the DP row in VGPRs, float32 in HMMER's arithmetic: sweeps P1 and P2 of the scoring
//                          kernel at FULL WIDTH only - no node window, no certificate, no band, no stored match rows -
//                          through the row primitives of wh_device.h (forward_sweep, backward_emit, backward_cells,
//                          RowsDown, region_scan_global).  The special states of every row go to a per-wave HBM workspace
//                          of 6 x (L + 1) floats, so the query length sets no limit.  A workgroup is four waves on ONE
//                          model, pass-synchronous: the eight transition arrays of one orientation are resident in LDS at
//                          a time (Forward's while the four waves run P1, Backward's while they run P2) and the emission
//                          rows beside them where they fit, as the long-model scoring kernel lays them out.
//   seq_expect_any_kernel  models beyond: float64, one wave per pair, the row in HBM (gforward of wh_f64.h and a Backward
//                          sweep of the same shape).  For correctness; it need not be fast.
//   seq_compact_kernel     the reported pairs of a scoring call in pair order (one workgroup: an ordered compaction)
//   seq_rows_kernel        one lane per row: whs::seq_table_row, the inline the host half runs too
#include <hip/hip_runtime.h>

#include "wh_device.h"
#include "wh_f64.h"
#include "wh_seqtab.h"

namespace wh {

using namespace whs;

namespace {

// the multidomain test of a region (ri .. rj): max_z min(etot[z] - etot[ri - 1], btot[rj] - btot[z - 1]) >= rt3, the
// cumulative sums where region_scan_global left them (SP_C: etot, SP_J: btot)
__device__ __forceinline__ bool region_is_multi(const float *spec, int SP, int ri, int rj, int lane) {
  const float e0 = __builtin_nontemporal_load(spec + SP_C * SP + ri - 1), bj = __builtin_nontemporal_load(spec + SP_J * SP + rj);
  float mx = -1.0f;
  for (int z = ri + lane; z <= rj; z += kWave) {
    const float u = __builtin_nontemporal_load(spec + SP_C * SP + z) - e0, v = bj - __builtin_nontemporal_load(spec + SP_J * SP + z - 1);
    mx = fmaxf(mx, fminf(u, v));
  }
  return wave_max(mx) >= kRt3;
}

// P2 at full width: the multihit Backward sweep over the special states P1 left in the wave's workspace; overwrites the
// SP_E, SP_B, SP_N rows with the posteriors pe, pb, njc (64 rows per access in both directions: RowsDown)
template <int Q>
__device__ __forceinline__ void backward_decode_full(const float *bwL, const float *emL, const float *emG, int Klds, const uint8_t *seq, int L,
                                                     LenCfg cm, float invZ, int ef_L, float *spec, int SP, int lane) {
  TransTab<Q, false> T;
  T.load(nullptr, bwL, lane);
  const ScanC sc = scan_prepare(lane_product<Q, false>(T, BW_DD));
  float Mb[Q], Ib[Q];
#pragma unroll
  for (int p = 0; p < Q; p++) { Mb[p] = 0.f; Ib[p] = 0.f; }
  float xC = cm.move, xJ = 0.f, xN = 0.f, xB = 0.f;
  int eb = 0;
  RowsDown<7> R;
  const int r_off[7] = {SP_S * SP, SP_S * SP, SP_E * SP, SP_B * SP, SP_N * SP, SP_J * SP, SP_C * SP};
  const int r_sh[7] = {0, -1, 0, 0, -1, -1, -1};
  float wE = 0.f, wB = 0.f, wN = 0.f;
  auto flush = [&](int lo) {                   // rows R.top - lane down to <lo>
    const int r = R.top - lane;
    if (r >= lo) {
      __builtin_nontemporal_store(wE, spec + SP_E * SP + r);
      __builtin_nontemporal_store(wB, spec + SP_B * SP + r);
      __builtin_nontemporal_store(wN, spec + SP_N * SP + r);
    }
  };
  R.load(spec, r_off, r_sh, L, lane);
#pragma unroll 1
  for (int i = L; i >= 0; i--) {
    asm volatile("" ::: "memory");
    if (R.spent(i)) { flush(i + 1); R.load(spec, r_off, r_sh, i, lane); }
    if (i < L) {
      xB = wave_sum(backward_emit<Q, false>(T, emL, emG, seq[i], Klds, lane, Mb));
      xJ = fmaf(xJ, cm.loop, xB * cm.move);
      xC = xC * cm.loop;
      xN = fmaf(xN, cm.loop, xB * cm.move);
    }
    float xE = fmaf(xC, cm.EC, xJ * cm.EJ);
    if (i >= 1) backward_cells<Q, false, false>(T, sc, Mb, Ib, xE);
    const float big = fmaxf(xB, xN);
    if (big > 1048576.0f) {                    // (wh_device.h: kRescaleHi, 2^20)
      const int e = f32_exponent(big);
      const float r = pow2f_int(-e);
#pragma unroll
      for (int p = 0; p < Q; p++) { Mb[p] *= r; Ib[p] *= r; }
      xB *= r; xJ *= r; xC *= r; xN *= r; xE *= r;
      eb += e;
    }
    const float s_i = ldexpf(invZ, R.s(0, i) + eb - ef_L);
    const float pe = R.f(2, i) * xE * s_i;
    const float pb = R.f(3, i) * xB * s_i;
    float njc = 0.f;
    if (i >= 1) {
      const float s_p = ldexpf(invZ, R.s(1, i) + eb - ef_L);
      njc = R.f(4, i) * xN;
      njc = fmaf(R.f(5, i), xJ, njc);
      njc = fmaf(R.f(6, i), xC, njc);
      njc = njc * cm.loop * s_p;
    }
    if (lane == R.top - i) { wE = pe; wB = pb; wN = njc; }
  }
  flush(0);
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
}

// exp, reg, clu of one pair from the posteriors: the region scan of wh_device.h (its list holds WH_MAX_ENVELOPES regions; it
// counts all), the multidomain test of every listed region, and - for a pair with more regions than the list holds - the
// regions behind the list from the cumulative sums the scan stored: btot[j] - btot[j - 1] and etot[j] - etot[j - 1] are the
// very differences the scan decided on, so these are its regions to the bit.
__device__ __forceinline__ wh_seq_expect_rec count_regions(float *spec, int SP, int L, int *regs, int lane) {
  int nenv = 0, nreg = 0, flags = 0;
  region_scan_global<SPEC_SOA>(spec, SP, L, regs, lane, nenv, nreg, flags);
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  int clu = 0;
  for (int e = 0; e < nenv; e++) clu += region_is_multi(spec, SP, regs[2 * e], regs[2 * e + 1], lane) ? 1 : 0;
  if (nreg > nenv) {
    int i0 = -1, seen = nenv;
    bool trig = false;
    for (int j0 = regs[2 * (nenv - 1) + 1] + 1; j0 <= L; j0 += kWave) {
      const int jj = j0 + lane;
      const bool valid = jj <= L;
      const float mo = valid ? 1.0f - __builtin_nontemporal_load(spec + SP_N * SP + jj) : 0.f;
      const float db = valid ? __builtin_nontemporal_load(spec + SP_J * SP + jj) - __builtin_nontemporal_load(spec + SP_J * SP + jj - 1) : 0.f;
      const float de = valid ? __builtin_nontemporal_load(spec + SP_C * SP + jj) - __builtin_nontemporal_load(spec + SP_C * SP + jj - 1) : 0.f;
      const int cnt = L - j0 + 1 < kWave ? L - j0 + 1 : kWave;
      for (int t = 0; t < cnt; t++) {
        const int j = j0 + t;
        const float mocc = readlane_f(mo, t);
        if (!trig) {
          if (mocc - readlane_f(db, t) < kRt2) i0 = j;
          else if (i0 == -1) i0 = j;
          if (mocc >= kRt1) trig = true;
        } else if (mocc - readlane_f(de, t) < kRt2) {
          clu += region_is_multi(spec, SP, i0, j, lane) ? 1 : 0;
          seen++;
          i0 = -1;
          trig = false;
        }
      }
    }
    if (seen != nreg) nreg = -seen;      // (cannot happen: the host counts a negative reg as a mismatch)
  }
  wh_seq_expect_rec o;
  o.exp = __builtin_nontemporal_load(spec + SP_J * SP + L);
  o.reg = nreg; o.clu = clu;
  return o;
}

}  // namespace

template <int Q>
__global__ __launch_bounds__(kSeqWaves * 64) void seq_expect_kernel(SeqExpArgs a) {
  extern __shared__ __attribute__((aligned(16))) float seq_smem[];
  volatile int *s_item = reinterpret_cast<volatile int *>(seq_smem);
  constexpr int TBL = Q * kWave;
  float *trL = seq_smem + 4;                            // eight arrays of ONE orientation
  float *emL = trL + FW_NARR * TBL;                     // Klds emission rows
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int wave_words = 2 * WH_MAX_ENVELOPES + a.seq_lds / 4;
  int *regs = reinterpret_cast<int *>(emL + (size_t)a.Klds * TBL) + (size_t)wave * wave_words;
  const int SP = a.SP;
  float *spec = a.ws + ((size_t)blockIdx.x * kSeqWaves + wave) * a.ws_stride;
  uint8_t *seq = a.seq_lds ? reinterpret_cast<uint8_t *>(regs + 2 * WH_MAX_ENVELOPES) : reinterpret_cast<uint8_t *>(spec + (size_t)kSeqSpecArrays * SP);
  const DevHMM *hmms = reinterpret_cast<const DevHMM *>(a.hmms);
  const double LOG2 = 0.69314718055994529;

  for (;;) {
    __syncthreads();
    if (threadIdx.x == 0) s_item[0] = atomicAdd(a.counter, 1);
    __syncthreads();
    const int item = __builtin_amdgcn_readfirstlane(s_item[0]);
    if (item >= a.n_items) break;
    const SeqItem it = a.items[item];
    const int h = __builtin_amdgcn_readfirstlane(it.h), n = __builtin_amdgcn_readfirstlane(it.n);
    const DevHMM *hm = hmms + h;
    const float *emG = a.tables + hm->em_off;
    {
      const float4 *src = reinterpret_cast<const float4 *>(emG);
      float4 *dst = reinterpret_cast<float4 *>(emL);
      for (int t = threadIdx.x; t < a.Klds * TBL / 4; t += blockDim.x) dst[t] = src[t];
    }
    for (int base = 0; base < n; base += kSeqWaves) {
      {
        const float4 *src = reinterpret_cast<const float4 *>(a.tables + hm->fw_off);
        float4 *dst = reinterpret_cast<float4 *>(trL);
        for (int t = threadIdx.x; t < FW_NARR * TBL / 4; t += blockDim.x) dst[t] = src[t];
      }
      __syncthreads();
      const bool has = base + wave < n;
      int64_t t_out = 0;
      int L = 0;
      bool ok = false;
      LenCfg cm = len_config(1, true);
      float invZ = 0.f;
      int ef_L = 0;
      if (has) {
        t_out = a.order[it.lo + base + wave];
        const int64_t qi = a.pair_list[t_out] / a.H;
        const int64_t off = a.offsets[qi];
        L = __builtin_amdgcn_readfirstlane((int)(a.offsets[qi + 1] - off));
        if (L > 0 && L <= a.Lcap) {
          for (int t = lane; t < L; t += kWave) { const int r = a.residues[off + t]; seq[t] = (uint8_t)(r < a.Kp ? r : a.Kp - 1); }
          __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
          __builtin_amdgcn_wave_barrier();
          cm = len_config(L, true);
          TransTab<Q, false> T;
          T.load(nullptr, trL, lane);
          const ScanC sc = scan_prepare(lane_product<Q, false>(T, FW_D2));
          float xC = 0.f;
          forward_sweep<Q, false, false>(T, sc, emL, emG, a.Klds, seq, L, cm, spec, SP, nullptr, 0.f, lane, xC, ef_L);
          __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
          xC = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, xC)));
          ef_L = __builtin_amdgcn_readfirstlane(ef_L);
          const float fwdsc = (float)((double)ef_L * LOG2 + log((double)(xC * cm.move)));
          ok = xC > 0.f && isfinite(fwdsc);
          invZ = 1.0f / (xC * cm.move);
        }
      }
      __syncthreads();                              // every wave has finished P1: the other orientation
      {
        const float4 *src = reinterpret_cast<const float4 *>(a.tables + hm->bw_off);
        float4 *dst = reinterpret_cast<float4 *>(trL);
        for (int t = threadIdx.x; t < BW_NARR * TBL / 4; t += blockDim.x) dst[t] = src[t];
      }
      __syncthreads();
      if (has) {
        wh_seq_expect_rec o;
        o.exp = 0.f; o.reg = 0; o.clu = 0;
        if (ok) {
          backward_decode_full<Q>(trL, emL, emG, a.Klds, seq, L, cm, invZ, ef_L, spec, SP, lane);
          o = count_regions(spec, SP, L, regs, lane);
        }
        if (lane == 0) a.out[t_out] = o;
      }
      __syncthreads();                              // ... and P2: the tables may change again
    }
  }
}

size_t seq_expect_lds_bytes(int Q, int Klds, int seq_lds) {
  return 16 + (size_t)(FW_NARR + Klds) * Q * kWave * sizeof(float) + (size_t)kSeqWaves * (2 * WH_MAX_ENVELOPES * sizeof(int) + (size_t)seq_lds);
}

template <int Q>
static hipError_t launch_seq_expect_t(const SeqExpArgs &a, int blocks, size_t lds, hipStream_t s) {
  hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void *>(&seq_expect_kernel<Q>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL((seq_expect_kernel<Q>), dim3(blocks), dim3(kSeqWaves * 64), lds, s, a);
  return hipGetLastError();
}

int seq_expect_launch(int Q, const SeqExpArgs &a, int blocks, size_t lds, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  switch (Q) {
    case 4: return (int)launch_seq_expect_t<4>(a, blocks, lds, s);
    case 8: return (int)launch_seq_expect_t<8>(a, blocks, lds, s);
    case 12: return (int)launch_seq_expect_t<12>(a, blocks, lds, s);
    case 16: return (int)launch_seq_expect_t<16>(a, blocks, lds, s);
    case 20: return (int)launch_seq_expect_t<20>(a, blocks, lds, s);
    case 24: return (int)launch_seq_expect_t<24>(a, blocks, lds, s);
    case 28: return (int)launch_seq_expect_t<28>(a, blocks, lds, s);
    case 32: return (int)launch_seq_expect_t<32>(a, blocks, lds, s);
    case 36: return (int)launch_seq_expect_t<36>(a, blocks, lds, s);
    case 40: return (int)launch_seq_expect_t<40>(a, blocks, lds, s);
    case 44: return (int)launch_seq_expect_t<44>(a, blocks, lds, s);
    case 48: return (int)launch_seq_expect_t<48>(a, blocks, lds, s);
    default: return (int)hipErrorInvalidValue;
  }
}

// ---------------------------------------------------------------------------------------------- any size, float64
namespace {

__device__ __forceinline__ double shfl_down_dd(double v, int d) {
  const long long u = __double_as_longlong(v);
  const int lo = __shfl_down((int)(u & 0xFFFFFFFFll), d), hi = __shfl_down((int)(u >> 32), d);
  return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ double wave_max_dd(double x) {
  for (int m = 32; m >= 1; m >>= 1) {
    const long long u = __double_as_longlong(x);
    const int lo = __shfl_xor((int)(u & 0xFFFFFFFFll), m), hi = __shfl_xor((int)(u >> 32), m);
    const double o = __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
    x = o > x ? o : x;
  }
  return x;
}
// the value of node k + 1 for node (q, lane) of a lane-blocked array (0 behind the last lane's last node)
__device__ __forceinline__ double node_after(const double *base, int Q, int q, int lane) {
  if (q + 1 < Q) return __builtin_nontemporal_load(base + ofs2(q + 1, lane));
  if (lane < 63) return __builtin_nontemporal_load(base + ofs2(0, lane + 1));
  return 0.0;
}

// Multihit Backward sweep in float64 with the row in HBM (two alternating rows of 3 x Q x 64 doubles: M, I, D), node by
// node: the special states of every row go to xs ((L + 1) x xNSPEC doubles: N B E J C, xCLS = the cumulated scale).  The
// recurrences and their order are those of the any-size scoring kernel's sweep; one node per step - slow, and simple.
__device__ void backward_specials_f64(const GModel &m, const uint8_t *seq, int L, GLen c, double *brow0, double *brow1, double *xs, int lane) {
  const int Q = m.Q, M = m.M;
  const size_t SQ = (size_t)Q * 64;
  const double *tf = m.tf;
  double ls = 0.0, nN = 0.0, nJ = 0.0, nC = c.move, xbsum_prev = 0.0;
  for (int i = L; i >= 0; i--) {
    double xBv, xJv, xCv, xNv;
    if (i == L) { xCv = c.move; xJv = 0.0; xNv = 0.0; xBv = 0.0; }
    else {
      xBv = wave_sum_d(xbsum_prev);
      xJv = nJ * c.loop + xBv * c.move;
      xCv = nC * c.loop;
      xNv = nN * c.loop + xBv * c.move;
    }
    double xEv = xCv * c.EC + xJv * c.EJ;
    double rs = 1.0;
    if (xBv > 1e60 || xNv > 1e60) {
      const double big = xBv > xNv ? xBv : xNv;
      rs = 1.0 / big;
      xBv *= rs; xJv *= rs; xCv *= rs; xNv *= rs; xEv *= rs; ls += log(big);
    }
    if (i >= 1) {
      wave_mem_sync();     // row i + 1 was written by other lanes of this wave
      const bool have_next = i < L;
      const double *nr = (i + 1) & 1 ? brow1 : brow0;
      double *cr = i & 1 ? brow1 : brow0;
      const double *odn = m.te + (size_t)seq[have_next ? i : i - 1] * SQ;       // residue x_{i+1} (not read on the last row)
      const double *odc = m.te + (size_t)seq[i - 1] * SQ;                       // residue x_i
      // pass 1, the lane's nodes from the last to the first: I, the M terms that do not need D, the D chain with nothing
      // entering from the right
      double dloc = 0.0, P = 1.0;
      for (int q = Q - 1; q >= 0; q--) {
        const int k = lane * Q + q + 1;
        const size_t o = ofs2(q, lane);
        const double mn = have_next ? node_after(nr, Q, q, lane) : 0.0, on = have_next ? node_after(odn, Q, q, lane) : 0.0;
        const double tAn = node_after(tf + gA * SQ, Q, q, lane), tBn = node_after(tf + gB * SQ, Q, q, lane);
        const double tCn = node_after(tf + gC * SQ, Q, q, lane), tDn = node_after(tf + gD2 * SQ, Q, q, lane);
        const double inn = have_next ? __builtin_nontemporal_load(nr + SQ + o) : 0.0;
        const double mnext = mn * on * rs, in = inn * rs;
        double iv = mnext * tBn + in * tf[gII * SQ + o];
        double mpart = mnext * tAn + in * tf[gMI * SQ + o] + xEv;
        double av = mnext * tCn + xEv;
        if (k >= M) { iv = 0.0; if (k == M) { mpart = xEv; av = xEv; } else { mpart = 0.0; av = 0.0; } }
        dloc = k > M ? 0.0 : av + tDn * dloc;
        P = k > M ? 0.0 : P * tDn;
        cr[o] = mpart; cr[SQ + o] = iv; cr[2 * SQ + o] = dloc;
      }
      // cross-lane: D(first node of lane r) = dloc + P * D(first node of lane r + 1), from the last lane down
      double Bv = dloc, Av = P;
      for (int d = 1; d < 64; d <<= 1) {
        const double Bo = shfl_down_dd(Bv, d), Ao = shfl_down_dd(Av, d);
        if (lane + d < 64) { Bv = Bv + Av * Bo; Av = Av * Ao; }
      }
      const double dn = shfl_down_dd(Bv, 1);
      const double din = lane < 63 ? dn : 0.0;          // true D of the first node of lane + 1
      // pass 2: true D, the M term through D(k + 1), and what the row above needs from this one
      double Pq = 1.0, dnext = din, xbsum = 0.0;
      for (int q = Q - 1; q >= 0; q--) {
        const int k = lane * Q + q + 1;
        const size_t o = ofs2(q, lane);
        const double tDn = node_after(tf + gD2 * SQ, Q, q, lane), tMDn = node_after(tf + gD1 * SQ, Q, q, lane);
        Pq = k > M ? 0.0 : Pq * tDn;
        double dv = __builtin_nontemporal_load(cr + 2 * SQ + o) + Pq * din;
        double mv = __builtin_nontemporal_load(cr + o) + (k < M ? dnext * tMDn : 0.0);
        if (k > M) { dv = 0.0; mv = 0.0; }
        cr[o] = mv; cr[2 * SQ + o] = dv;
        dnext = dv;
        xbsum += mv * odc[o] * tf[gE * SQ + o];
      }
      xbsum_prev = xbsum;
    }
    if (lane == 0) { double *t = xs + (size_t)i * xNSPEC; t[xN] = xNv; t[xB] = xBv; t[xE] = xEv; t[xJ] = xJv; t[xC] = xCv; t[xCLS] = ls; }
    nN = xNv; nJ = xJv; nC = xCv;
  }
  wave_mem_sync();
}

__host__ __device__ inline size_t any_rowlen(int Q) { return (size_t)3 * Q * 64 + xNSPEC; }
__host__ __device__ inline size_t any_seq_doubles(int Lcap) { return ((size_t)Lcap + 16 + 7) / 8; }
__host__ __device__ inline size_t any_row_doubles(int Lcap) { return ((size_t)Lcap + 4 + 1) & ~(size_t)1; }

}  // namespace

// a wave's workspace: two rows, the Forward and the Backward special states of every row, five per-row arrays (pb, pe,
// mocc, btot, etot), the residues
size_t seq_expect_any_doubles(int Lcap, int Qmax) {
  return 2 * any_rowlen(Qmax) + 2 * (size_t)(Lcap + 2) * xNSPEC + 5 * any_row_doubles(Lcap) + any_seq_doubles(Lcap) + 8;
}

__global__ __launch_bounds__(64) void seq_expect_any_kernel(SeqExpArgs a) {
  const int lane = threadIdx.x;
  const DevHMM *hmms = reinterpret_cast<const DevHMM *>(a.hmms);
  double *slab = a.gws + (size_t)blockIdx.x * a.gws_stride;
  double *xsF = slab + 2 * any_rowlen(a.Qmax);
  double *xsB = xsF + (size_t)(a.Lcap + 2) * xNSPEC;
  const size_t RL = any_row_doubles(a.Lcap);
  double *pbv = xsB + (size_t)(a.Lcap + 2) * xNSPEC, *pev = pbv + RL, *moccv = pev + RL, *btotv = moccv + RL, *etotv = btotv + RL;
  uint8_t *seq = reinterpret_cast<uint8_t *>(etotv + RL);
  for (;;) {
    int item = 0;
    if (lane == 0) item = atomicAdd(a.counter, 1);
    item = __builtin_amdgcn_readfirstlane(__shfl(item, 0));
    if (item >= a.n_items) break;
    const int64_t t_out = a.order[item];
    const int64_t pl = a.pair_list[t_out];
    const int h = (int)(pl % a.H);
    const int64_t qi = pl / a.H;
    const DevHMM hm = hmms[h];
    GModel m;
    m.tf = a.gtab + hm.gfw_off; m.te = a.gtab + hm.gem_off;
    m.Q = __builtin_amdgcn_readfirstlane(hm.Q); m.M = __builtin_amdgcn_readfirstlane(hm.M);
    GMx mx;
    mx.Q = m.Q; mx.rowlen = any_rowlen(m.Q); mx.p = slab;
    const int64_t off = a.offsets[qi];
    const int L = (int)(a.offsets[qi + 1] - off);
    wh_seq_expect_rec o;
    o.exp = 0.f; o.reg = 0; o.clu = 0;
    if (L > 0 && L <= a.Lcap) {
      for (int t = lane; t < L; t += 64) { const int r = a.residues[off + t]; seq[t] = (uint8_t)(r < a.Kp ? r : a.Kp - 1); }
      wave_mem_sync();
      const GLen cm = glen_config(L, true);
      const double fwd = gforward<false>(m, seq, L, cm, mx, lane, xsF);
      if (isfinite(fwd) && isfinite((float)fwd)) {
        backward_specials_f64(m, seq, L, cm, mx.row(0), mx.row(1), xsB, lane);
        for (int i = 1 + lane; i <= L; i += 64) {
          const double *f0 = xsF + (size_t)(i - 1) * xNSPEC, *f1 = xsF + (size_t)i * xNSPEC;
          const double *b0 = xsB + (size_t)(i - 1) * xNSPEC, *b1 = xsB + (size_t)i * xNSPEC;
          const double pb = f0[xB] * b0[xB] * exp(f0[xCLS] + b0[xCLS] - fwd);
          const double pe = f1[xE] * b1[xE] * exp(f1[xCLS] + b1[xCLS] - fwd);
          const double sc = exp(f0[xCLS] + b1[xCLS] - fwd);
          const double njcp = (f0[xN] * b1[xN] + f0[xJ] * b1[xJ] + f0[xC] * b1[xC]) * cm.loop * sc;
          pbv[i] = pb; pev[i] = pe; moccv[i] = 1.0 - njcp;
        }
        if (lane == 0) { btotv[0] = 0.0; etotv[0] = 0.0; }
        wave_mem_sync();
        // the cumulative sums first (rows in order, one lane), then the scan over them
        double btot = 0.0, etot = 0.0;
        for (int j0 = 1; j0 <= L; j0 += 64) {
          const int jj = j0 + lane;
          const bool valid = jj <= L;
          const double pbl = valid ? __builtin_nontemporal_load(pbv + jj) : 0.0, pel = valid ? __builtin_nontemporal_load(pev + jj) : 0.0;
          double bout = 0.0, eout = 0.0;
          const int cnt = L - j0 + 1 < 64 ? L - j0 + 1 : 64;
          for (int t = 0; t < cnt; t++) {
            btot = btot + readlane_d(pbl, t);
            etot = etot + readlane_d(pel, t);
            if (lane == t) { bout = btot; eout = etot; }
          }
          if (valid) { btotv[jj] = bout; etotv[jj] = eout; }
        }
        wave_mem_sync();
        int nreg = 0, clu = 0, i0 = -1;
        bool trig = false;
        for (int j0 = 1; j0 <= L; j0 += 64) {
          const int jj = j0 + lane;
          const bool valid = jj <= L;
          const double mol = valid ? __builtin_nontemporal_load(moccv + jj) : 0.0;
          const double db = valid ? __builtin_nontemporal_load(btotv + jj) - __builtin_nontemporal_load(btotv + jj - 1) : 0.0;
          const double de = valid ? __builtin_nontemporal_load(etotv + jj) - __builtin_nontemporal_load(etotv + jj - 1) : 0.0;
          const int cnt = L - j0 + 1 < 64 ? L - j0 + 1 : 64;
          for (int t = 0; t < cnt; t++) {
            const int j = j0 + t;
            const double mocc = readlane_d(mol, t);
            if (!trig) {
              if (mocc - readlane_d(db, t) < (double)kRt2) i0 = j;
              else if (i0 == -1) i0 = j;
              if (mocc >= (double)kRt1) trig = true;
            } else if (mocc - readlane_d(de, t) < (double)kRt2) {
              const double e0 = __builtin_nontemporal_load(etotv + i0 - 1), bj = __builtin_nontemporal_load(btotv + j);
              double mxv = -1.0;
              for (int z = i0 + lane; z <= j; z += 64) {
                const double u = __builtin_nontemporal_load(etotv + z) - e0, v = bj - __builtin_nontemporal_load(btotv + z - 1);
                const double w = u < v ? u : v;
                mxv = w > mxv ? w : mxv;
              }
              if (wave_max_dd(mxv) >= (double)kRt3) clu++;
              nreg++;
              i0 = -1; trig = false;
            }
          }
        }
        o.exp = (float)btot; o.reg = nreg; o.clu = clu;
      }
    }
    if (lane == 0) a.out[t_out] = o;
    __builtin_amdgcn_wave_barrier();
  }
}

int seq_expect_any_launch(const SeqExpArgs &a, int blocks, void *stream) {
  hipLaunchKernelGGL(seq_expect_any_kernel, dim3(blocks), dim3(64), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- the row assembly
// the reported pairs in pair order: ONE workgroup walks the flags 1 024 at a time (ballot, wave totals in LDS); the count
// goes on beyond <cap>, the list does not
__global__ __launch_bounds__(1024) void seq_compact_kernel(const uint8_t *flags, long long npairs, long long *list, unsigned long long *count, long long cap) {
  __shared__ int wtot[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long done = 0;
  for (long long base = 0; base < npairs; base += 1024) {
    const long long p = base + threadIdx.x;
    const bool rep = p < npairs && (flags[p] & WH_FLAG_REPORTED);
    const unsigned long long bal = __ballot(rep);
    if (lane == 0) wtot[wave] = __builtin_popcountll(bal);
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < 16; w++) { const int c = wtot[w]; all += c; if (w < wave) before += c; }
    const long long pos = done + before + __builtin_popcountll(bal & ((1ull << lane) - 1));
    if (rep && pos < cap) list[pos] = p;
    done += all;
    __syncthreads();
  }
  if (threadIdx.x == 0) *count = (unsigned long long)done;
}

int seq_table_compact_launch(const uint8_t *flags, int64_t npairs, int64_t *list, unsigned long long *count, int64_t cap, void *stream) {
  hipLaunchKernelGGL(seq_compact_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, flags, (long long)npairs, (long long *)list, count, (long long)cap);
  return (int)hipGetLastError();
}

__global__ __launch_bounds__(256) void seq_rows_kernel(SeqTabArgs a) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.rows) return;
  const int64_t p = a.pair_list[t], q = p / a.H;
  const int h = (int)(p % a.H);
  const int L = (int)(a.offsets[q + 1] - a.offsets[q]);
  wh_seq_row r;
  const int st = seq_table_row(p, a.detail[p], L, a.evp[2 * h], a.evp[2 * h + 1], a.expect[t], a.lnE_Z, a.lnIncE_Z, a.lnDomE_domZ, a.lnIncDomE_domZ, &r);
  a.out[t] = r;
  if (st & 2) atomicAdd(a.status + 1, 1ull);
  if (st & 1) atomicAdd(a.status + 2, 1ull);
}

int seq_table_rows_launch(const SeqTabArgs &a, void *stream) {
  if (a.rows <= 0) return 0;
  hipLaunchKernelGGL(seq_rows_kernel, dim3((unsigned)((a.rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

}  // namespace wh
