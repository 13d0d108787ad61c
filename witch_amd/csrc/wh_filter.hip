// hmmsearch's two integer acceleration filters on the device: the 8-bit MSV filter and the 16-bit Viterbi filter over
// every (query, model) pair of a call, and the pipeline's decisions between them (wh_filter.h; host side:
// wh_host_filter.hip).
//
// ONE WAVEFRONT PER PAIR, the DP row in VGPRs: lane r owns the Q contiguous nodes r Q + 1 .. r Q + Q (Q = 2 .. 48 by
// model class, 64 Q >= M), one 32-bit register per cell - bytes and words are held widened and clamped explicitly, so
// every cell carries the scalar cores' value (calib_msv_core, calib_viterbi_core), whatever its representation.
//  * MSV: M(i,k) needs M(i-1,k-1) and xB only.  A row step is a one-node shift (in the lane, and one wave_shr:1 DPP move
//    for the lane's first node), max, saturating add and subtract, and a wave maximum for xE.
//  * Viterbi filter: M and I as in the scalar core; the D row is a max-plus prefix over the nodes.  Every DD cost is <= 0
//    and -32768 is the floor, so a chain of saturating 16-bit adds equals an int32 running sum clamped once at -32768:
//    each lane closes its own nodes from a carry of "nothing" (kNeg), the lanes combine (value leaving the lane, sum of
//    the lane's DD costs) with a six-step scan, and a second pass over the lane adds the carry.  Exact below 65 536
//    nodes (the int32 sums stay above -2^31).
//  * The quantised tables are read from global memory in the lane-blocked layout (a lane's Q cells are one or a few
//    16-byte accesses, a wavefront's access one contiguous line); the four waves of a workgroup and the workgroups next
//    to them work on the same model, whose tables (18 - 29 columns of Mpad bytes / words) stay in L2.  Residues are
//    fetched 64 at a time, one per lane, and handed out with v_readlane.
//  * The Viterbi sweep runs only where the pipeline asks for it (rejected pairs and pairs already below F2 skip it): the
//    decision is wave-uniform.
// Models beyond 3 072 nodes: one LANE per pair runs the scalar cores themselves with rows in HBM, lane-interleaved, as
// the calibration kernel does - no model-length limit.
// Results leave through ordinary vector stores of lane 0.
//
// THE BIAS FILTER (WH_FILTER_BIAS=1: this file compiled a second time into wh_filter_bias.o, whose launchers carry the
// suffix _bias; without it the kernels compile exactly as they did before the stage existed).  A pair past the MSV stage
// runs the composition Forward of wh_filter.h between the MSV sweep and the stage decision - the MSV row is dead by then.
// The two-value recurrence is wave-uniform (every lane computes it); residues are fetched 64 at a time, each lane looks
// up its own residue's odds ratio, and v_readlane hands them out.  Lane j keeps the maximum of row base + j, so the 64
// filter_logs of a chunk are taken in parallel; their float32 sum is then formed in row order, which makes the bits the
// scalar function's (filter_bias_score).  The long-model kernel calls the scalar function itself.
#include <hip/hip_runtime.h>

#include "wh_filter.h"

#ifndef WH_FILTER_BIAS
#define WH_FILTER_BIAS 0
#endif

namespace whf {

namespace {

constexpr bool kBias = WH_FILTER_BIAS != 0;
#if WH_FILTER_BIAS
using KArgs = FilterBiasArgs;
#else
using KArgs = FilterArgs;
#endif

constexpr int kNeg = -(1 << 29);       // "no path" of the int32 D closure: below every clamped value, far from overflow

__device__ __forceinline__ int clamp16(int x) { return min(max(x, -32768), 32767); }
// lane r <- lane r - 1; lane 0 <- fill
__device__ __forceinline__ int lane_shr1(int x, int fill) { return __builtin_amdgcn_update_dpp(fill, x, 0x138, 0xF, 0xF, false); }
__device__ __forceinline__ int wave_max_i(int x) {
  for (int d = 32; d >= 1; d >>= 1) x = max(x, __shfl_xor(x, d, 64));
  return x;
}

// Q bytes at p (aligned to min(Q, 16) bytes) -> Q ints
template <int Q> __device__ __forceinline__ void load_u8(const unsigned char *p, int (&c)[Q]) {
  if constexpr (Q % 16 == 0) {
    WH_UNROLL for (int i = 0; i < Q / 16; i++) {
      const uint4 v = reinterpret_cast<const uint4 *>(p)[i];
      const unsigned w[4] = {v.x, v.y, v.z, v.w};
      WH_UNROLL for (int j = 0; j < 16; j++) c[i * 16 + j] = (int)((w[j >> 2] >> (8 * (j & 3))) & 0xFFu);
    }
  } else if constexpr (Q == 8) {
    const uint2 v = *reinterpret_cast<const uint2 *>(p);
    WH_UNROLL for (int j = 0; j < 4; j++) { c[j] = (int)((v.x >> (8 * j)) & 0xFFu); c[4 + j] = (int)((v.y >> (8 * j)) & 0xFFu); }
  } else if constexpr (Q == 4) {
    const unsigned v = *reinterpret_cast<const unsigned *>(p);
    WH_UNROLL for (int j = 0; j < 4; j++) c[j] = (int)((v >> (8 * j)) & 0xFFu);
  } else {
    static_assert(Q == 2, "cells per lane");
    const unsigned v = *reinterpret_cast<const unsigned short *>(p);
    c[0] = (int)(v & 0xFFu); c[1] = (int)(v >> 8);
  }
}
// N words at p (aligned to min(2 N, 16) bytes) -> N ints, sign-extended
template <int N> __device__ __forceinline__ void load_i16(const int16_t *p, int (&c)[N]) {
  if constexpr (N % 8 == 0) {
    WH_UNROLL for (int i = 0; i < N / 8; i++) {
      const uint4 v = reinterpret_cast<const uint4 *>(p)[i];
      const unsigned w[4] = {v.x, v.y, v.z, v.w};
      WH_UNROLL for (int j = 0; j < 8; j++) c[i * 8 + j] = (int)(int16_t)(w[j >> 1] >> (16 * (j & 1)));
    }
  } else if constexpr (N == 4) {
    const uint2 v = *reinterpret_cast<const uint2 *>(p);
    c[0] = (int)(int16_t)v.x; c[1] = (int)(int16_t)(v.x >> 16); c[2] = (int)(int16_t)v.y; c[3] = (int)(int16_t)(v.y >> 16);
  } else {
    static_assert(N == 2, "cells per chunk");
    const unsigned v = *reinterpret_cast<const unsigned *>(p);
    c[0] = (int)(int16_t)v; c[1] = (int)(int16_t)(v >> 16);
  }
}

// ---- MSV: calib_msv_core's values.  res: the query's residues (0-based) ----------------------------------------
template <int Q> __device__ int msv_sweep(const FilterDevModel &d, const unsigned char *rb, const uint8_t *res, int L, int tjb, int lane) {
  const int Mpad = 64 * Q;
  const int bias = d.bias_b, base = d.base_b, tec = d.tec;
  const int tjbm = (tjb + d.tbm) & 0xFF;
  int m[Q];
  WH_UNROLL for (int j = 0; j < Q; j++) m[j] = 0;
  int xJ = 0, xB = max(base - tjbm, 0);
  const unsigned char *col = rb + (size_t)lane * Q;
  for (int i0 = 0; i0 < L; i0 += 64) {
    const int mine = i0 + lane < L ? min((int)res[i0 + lane], d.Kp - 1) : 0;      // (a code outside the alphabet must not leave the table)
    const int n = min(64, L - i0);
    for (int r = 0; r < n; r++) {
      const int x = __builtin_amdgcn_readlane(mine, r);
      int c[Q];
      load_u8<Q>(col + (size_t)x * Mpad, c);
      int prev = lane_shr1(m[Q - 1], 0);
      int xE = 0;
      WH_UNROLL for (int j = 0; j < Q; j++) {
        int sv = max(prev, xB);
        sv = min(sv + bias, 255);
        sv = max(sv - c[j], 0);
        prev = m[j];
        m[j] = sv;
        xE = max(xE, sv);
      }
      xE = wave_max_i(xE);
      if (min(xE + bias, 255) == 255) return -1;
      xE = max(xE - tec, 0);
      xJ = max(xJ, xE);
      xB = max(max(base, xJ) - tjbm, 0);
    }
  }
  return max(xJ, calib_msv_floor(base, bias, d.tbm, tec, tjb));      // the empty diagonal (wh_calibrate.h)
}

// ---- Viterbi filter: calib_viterbi_core's values ---------------------------------------------------------------------
template <int Q> __device__ int vit_sweep(const FilterDevModel &d, const int16_t *rw, const int16_t *tw, const uint8_t *res, int L, int xmove, int lane) {
  constexpr int CH = Q < 8 ? Q : 8;      // nodes per table access
  const int Mpad = 64 * Q;
  constexpr bool kKeepPfx = Q <= 16;     // the DD prefix sums of pass 1 stay in registers; larger classes form them again in pass 2
  int vm[Q], vi[Q], vd[Q], pfx[kKeepPfx ? Q : 1];
  WH_UNROLL for (int j = 0; j < Q; j++) { vm[j] = -32768; vi[j] = -32768; vd[j] = -32768; }
  const int xN = d.base_w;
  int xB = xN + xmove, xJ = -32768, xC = -32768;
  const int16_t *col = rw + (size_t)lane * Q;
  const int16_t *tcol = tw + (size_t)lane * Q;
  for (int i0 = 0; i0 < L; i0 += 64) {
    const int mine = i0 + lane < L ? min((int)res[i0 + lane], d.Kp - 1) : 0;      // (a code outside the alphabet must not leave the table)
    const int n = min(64, L - i0);
    for (int r = 0; r < n; r++) {
      const int x = __builtin_amdgcn_readlane(mine, r);
      const int16_t *rsc = col + (size_t)x * Mpad;
      // the transition costs do not change from row to row: the small classes keep them in registers (the compiler hoists the
      // loads), the large ones have no room for 8 Q more values and fetch them again (L1 / L2) - the pointer is made opaque
      if constexpr (Q >= 16) asm volatile("" : "+v"(tcol));
      // row i-1 at the node in front of the lane's first
      int pm = lane_shr1(vm[Q - 1], -32768), pi = lane_shr1(vi[Q - 1], -32768), pd = lane_shr1(vd[Q - 1], -32768);
      int xE = -32768;
      int dloc = kNeg, dsum = 0;       // the lane's D chain from "nothing": value entering node j, sum of DD in front of it
      WH_UNROLL for (int c0 = 0; c0 < Q; c0 += CH) {
        int e[CH], tBM[CH], tMM[CH], tIM[CH], tDM[CH], tMD[CH], tMI[CH], tII[CH], tDD[CH];
        load_i16<CH>(rsc + c0, e);
        load_i16<CH>(tcol + (size_t)vBM * Mpad + c0, tBM);
        load_i16<CH>(tcol + (size_t)vMM * Mpad + c0, tMM);
        load_i16<CH>(tcol + (size_t)vIM * Mpad + c0, tIM);
        load_i16<CH>(tcol + (size_t)vDM * Mpad + c0, tDM);
        load_i16<CH>(tcol + (size_t)vMD * Mpad + c0, tMD);
        load_i16<CH>(tcol + (size_t)vMI * Mpad + c0, tMI);
        load_i16<CH>(tcol + (size_t)vII * Mpad + c0, tII);
        load_i16<CH>(tcol + (size_t)vDD * Mpad + c0, tDD);
        WH_UNROLL for (int jj = 0; jj < CH; jj++) {
          const int j = c0 + jj;
          int sv = clamp16(xB + tBM[jj]);
          sv = max(sv, clamp16(pm + tMM[jj]));
          sv = max(sv, clamp16(pi + tIM[jj]));
          sv = max(sv, clamp16(pd + tDM[jj]));
          sv = clamp16(sv + e[jj]);
          xE = max(xE, sv);
          pm = vm[j]; pi = vi[j]; pd = vd[j];
          vm[j] = sv;
          vi[j] = max(clamp16(pm + tMI[jj]), clamp16(pi + tII[jj]));
          vd[j] = dloc;
          if constexpr (kKeepPfx) pfx[j] = dsum;
          dloc = max(clamp16(sv + tMD[jj]), dloc + tDD[jj]);
          dsum += tDD[jj];
        }
      }
      // the lanes' chains: (value leaving the lane, sum of its DD costs), left to right
      int A = dloc, S = dsum;
      WH_UNROLL for (int dd = 1; dd < 64; dd <<= 1) {
        const int Ap = __shfl_up(A, dd, 64), Sp = __shfl_up(S, dd, 64);
        if (lane >= dd) { A = max(A, max(Ap, kNeg) + S); S += Sp; }
      }
      const int carry = lane_shr1(A, kNeg);
      if constexpr (kKeepPfx) {
        WH_UNROLL for (int j = 0; j < Q; j++) vd[j] = max(max(vd[j], carry + pfx[j]), -32768);
      } else {
        int run = carry;
        WH_UNROLL for (int c0 = 0; c0 < Q; c0 += CH) {
          int tDD[CH];
          load_i16<CH>(tcol + (size_t)vDD * Mpad + c0, tDD);
          WH_UNROLL for (int jj = 0; jj < CH; jj++) { vd[c0 + jj] = max(max(vd[c0 + jj], run), -32768); run += tDD[jj]; }
        }
      }
      xE = wave_max_i(xE);
      if (xE >= 32767) return kCalibVitOverflow;
      xC = max(xC, xE + d.xE_move);
      xJ = max(xJ, xE + d.xE_loop);
      xB = max(xJ + xmove, xN + xmove);
    }
  }
  return xC;
}

#if WH_FILTER_BIAS
// ---- bias filter: filter_bias_score's value -----------------------------------------------------------------------
__device__ __forceinline__ float readlane_f(float x, int r) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), r)); }

__device__ float bias_sweep(const FilterBias *bm, FilterBiasLen bl, const uint8_t *res, int L, int Kp, int lane) {
  const float t10 = bm->t10, t11 = bm->t11;
  FilterBiasRow s{0.f, 0.f};
  float nullsc = 0.f;
  for (int i0 = 0; i0 < L; i0 += 64) {
    const int mine = i0 + lane < L ? min((int)res[i0 + lane], Kp - 1) : 0;      // (a code outside the alphabet must not leave the table)
    const float myeo = bm->eo1[mine];
    const int n = min(64, L - i0);
    float mymx = 1.f;
    for (int r = 0; r < n; r++) {
      const float mx = filter_bias_row(s, i0 + r == 0, readlane_f(myeo, r), t10, t11, bl);
      if (lane == r) mymx = mx;
    }
    const float lg = filter_log(mymx);
    for (int r = 0; r < n; r++) nullsc = nullsc + readlane_f(lg, r);      // in row order
  }
  return filter_bias_end(nullsc, s, bl);
}
#endif

template <int Q> __global__ __launch_bounds__(256) void filter_kernel(KArgs a, long long npairs) {
  const int lane = threadIdx.x & 63;
  // (with the bias sweep, up to 16 cells per lane: the wave's number is made known to be uniform, so that the pair's model
  // record and settings stay in scalar registers across the three sweeps - that keeps the waves per SIMD of the kernel
  // without the sweep for Q = 2, 4, 8; the two largest classes keep theirs without it and lose one with it)
  const long long p = (long long)blockIdx.x * 4 + (kBias && Q <= 16 ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : (int)(threadIdx.x >> 6));
  if (p >= npairs) return;
  // consecutive waves: consecutive queries of one model
  const long long q = p % a.nq;
  const int h = a.list[p / a.nq];
  const FilterDevModel d = a.models[h];
  const long long o0 = a.offsets[q];
  const int L = (int)(a.offsets[q + 1] - o0);
  const long long out = q * a.H + h;
  int stage = 0, msv = 0, vit = kVitNotRun;
  float bias_nats = 0.f;
  if (L > a.lmax) stage = kStageBadLen;      // (the caller's max_len is wrong: no record for this length)
  else if (L > 0) {
    FilterLen fl = a.lens[L];
    const uint8_t *res = a.residues + o0;
    msv = msv_sweep<Q>(d, a.tables + d.rb, res, L, fl.tjb, lane);
    msv = __builtin_amdgcn_readfirstlane(msv);
    bool run_vit = false;
#if !WH_FILTER_BIAS
    stage = filter_stage12(msv, fl, d.base_b, d.scale_b, d.thr, &run_vit);
#else
    float usc;
    if (filter_stage1(msv, fl, d.base_b, d.scale_b, d.thr, &usc)) {
      const float filtersc = readlane_f(bias_sweep(a.bias + h, a.blens[L], res, L, d.Kp, lane), 0);
      stage = filter_stage2_bias(usc, filtersc, d.thr, &run_vit);
      bias_nats = filtersc - fl.nullsc;
      fl.nullsc = filtersc;              // the Viterbi stage scores against it
    }
#endif
    if (run_vit) {
      vit = vit_sweep<Q>(d, reinterpret_cast<const int16_t *>(a.tables + d.rw), reinterpret_cast<const int16_t *>(a.tables + d.tw), res, L, fl.xmove, lane);
      vit = __builtin_amdgcn_readfirstlane(vit);
      stage |= filter_stage3(vit, fl, d.base_w, d.scale_w, d.thr);
    }
  }
  if (lane == 0) {
    a.stage[out] = (uint8_t)stage;
    if (a.bias_nats) a.bias_nats[out] = bias_nats;
    if (a.msv_raw) a.msv_raw[out] = msv;
    if (a.vit_raw) a.vit_raw[out] = vit;
  }
}

// residue i of a query (1-based) for the scalar cores; a code outside the alphabet must not leave the table here either
struct ClampedSeq {
  const uint8_t *p;
  int kmax;
  __device__ int get(int i) const { return min((int)p[i], kmax); }
};

// ---- models beyond the register classes: the scalar cores, one lane per pair, rows in HBM (lane-interleaved) --------
__global__ __launch_bounds__(64) void filter_hbm_kernel(KArgs a) {
  const long long lanes = a.q1 - a.q0;
  const long long t = (long long)blockIdx.x * 64 + threadIdx.x;
  if (t >= lanes) return;
  const long long q = a.q0 + t;
  const FilterDevModel d = a.models[a.h];
  const int M = d.M;
  const size_t W = (size_t)M + 1, S = (size_t)lanes;
  const long long o0 = a.offsets[q];
  const int L = (int)(a.offsets[q + 1] - o0);
  const long long out = q * a.H + a.h;
  int stage = 0, msv = 0, vit = kVitNotRun;
  float bias_nats = 0.f;
  if (L > a.lmax) stage = kStageBadLen;
  else if (L > 0) {
    FilterLen fl = a.lens[L];
    const ClampedSeq seq{a.residues + o0 - 1, d.Kp - 1};
    const CalibMSVPar mp{(uint8_t)d.base_b, (uint8_t)d.bias_b, (uint8_t)d.tbm, (uint8_t)d.tec, fl.tjb};
    const CalibRow<uint8_t> b0{a.ws + t, S};
    msv = calib_msv_core(M, mp, a.tables + d.rb, seq, L, b0, b0.plus(W));
    bool run_vit = false;
#if !WH_FILTER_BIAS
    stage = filter_stage12(msv, fl, d.base_b, d.scale_b, d.thr, &run_vit);
#else
    float usc;
    if (filter_stage1(msv, fl, d.base_b, d.scale_b, d.thr, &usc)) {
      const FilterBias *bm = a.bias + a.h;
      const float filtersc = filter_bias_score(bm->eo1, bm->t10, bm->t11, a.blens[L], seq, L);
      stage = filter_stage2_bias(usc, filtersc, d.thr, &run_vit);
      bias_nats = filtersc - fl.nullsc;
      fl.nullsc = filtersc;
    }
#endif
    if (run_vit) {
      const CalibVitPar vp{(int16_t)d.base_w, (int16_t)d.xE_loop, (int16_t)d.xE_move, fl.xmove};
      const CalibRow<int16_t> w0{reinterpret_cast<int16_t *>(a.ws + 2 * W * S) + t, S};
      vit = calib_viterbi_core(M, vp, reinterpret_cast<const int16_t *>(a.tables + d.rw), reinterpret_cast<const int16_t *>(a.tables + d.tw), seq, L, w0,
                               w0.plus(3 * W));
      stage |= filter_stage3(vit, fl, d.base_w, d.scale_w, d.thr);
    }
  }
  a.stage[out] = (uint8_t)stage;
  if (a.bias_nats) a.bias_nats[out] = bias_nats;
  if (a.msv_raw) a.msv_raw[out] = msv;
  if (a.vit_raw) a.vit_raw[out] = vit;
}

#if !WH_FILTER_BIAS
__global__ __launch_bounds__(256) void filter_count_kernel(const uint8_t *stage, long long n, unsigned long long *counts) {
  unsigned c1 = 0, c2 = 0, c3 = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const unsigned s = stage[i];
    c1 += s & 1u; c2 += (s >> 1) & 1u; c3 += (s >> 2) & 1u;
  }
  for (int d = 32; d >= 1; d >>= 1) { c1 += __shfl_xor(c1, d, 64); c2 += __shfl_xor(c2, d, 64); c3 += __shfl_xor(c3, d, 64); }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&counts[1], (unsigned long long)c1);
    atomicAdd(&counts[2], (unsigned long long)c2);
    atomicAdd(&counts[3], (unsigned long long)c3);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&counts[0], (unsigned long long)n);
}

#endif

template <int Q> int launch_q(const KArgs &a, long long npairs, hipStream_t s) {
  const long long blocks = (npairs + 3) / 4;
  hipLaunchKernelGGL(filter_kernel<Q>, dim3((unsigned)blocks), dim3(256), 0, s, a, npairs);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace

#if WH_FILTER_BIAS
#define launch_filter_class launch_filter_class_bias
#define launch_filter_hbm launch_filter_hbm_bias
#endif

int launch_filter_class(int cls, const KArgs &a, long long npairs, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  if (npairs <= 0) return 0;
  if ((npairs + 3) / 4 > 0x7FFFFFFFll) return -1;
  switch (cls) {
    case 0: return launch_q<kFilterQ[0]>(a, npairs, s);
    case 1: return launch_q<kFilterQ[1]>(a, npairs, s);
    case 2: return launch_q<kFilterQ[2]>(a, npairs, s);
    case 3: return launch_q<kFilterQ[3]>(a, npairs, s);
    case 4: return launch_q<kFilterQ[4]>(a, npairs, s);
    case 5: return launch_q<kFilterQ[5]>(a, npairs, s);
  }
  return -1;
}

int launch_filter_hbm(const KArgs &a, void *stream) {
  const long long lanes = a.q1 - a.q0;
  if (lanes <= 0) return 0;
  hipLaunchKernelGGL(filter_hbm_kernel, dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

#if !WH_FILTER_BIAS
int launch_filter_count(const uint8_t *stage, long long n, unsigned long long *counts, void *stream) {
  if (n <= 0) return 0;
  const unsigned blocks = (unsigned)std::min<long long>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(filter_count_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, stage, n, counts);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
#endif

}  // namespace whf
