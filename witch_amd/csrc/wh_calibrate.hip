// E-value calibration of a batch of freshly built models on the device (wh_hmmbuild_batch with WH_BUILD_STATS).
//
// Per model the calibration is 200 random sequences x 200 residues through the 8-bit MSV filter, 200 x 200 through the
// 16-bit Viterbi filter and 200 x 100 through a float64 Forward: nothing is shared between sequences or between models.
// The mapping is the simplest exact one: ONE LANE PER (model, sequence) runs the host's own sweep (wh_calibrate.h:
// calib_msv_core, calib_viterbi_core, calib_forward_core - the same functions, compiled for the device), so the two
// integer filters and the contraction-free float64 recurrence give the host's values bit for bit.  One workgroup of
// 256 threads (200 of them with a sequence) per (model, sweep); the three sweeps of a model are three workgroups of one
// launch (blockIdx.x: 0 Forward, the longest, first; 1 Viterbi; 2 MSV).
//
// Memory: the DP rows are lane-interleaved in HBM ([node][lane]: the 64 lanes of a wave read one node of their 64 rows
// in one or two lines), two sets per sweep that are ping-ponged, read kCalibChunk nodes ahead.  The quantised tables of
// the two filters are staged in LDS when they fit 64 KiB (MSV K(M+1) bytes; Viterbi 2K(M+1) + 16(M+1): a 2 574-node
// DNA model needs 62 KB) and read from global memory otherwise - model length has no limit here either.  The Forward
// tables are float64 ((8 + K)(M+1) doubles) and always read from global memory: every lane of a workgroup reads the
// same transition line, and one of K emission lines.
//
// The host (calibrate_device below) converts the profiles, uploads tables and sequences, sizes the row workspace from
// the batch, runs the models in groups that fit the budget (one stream, one synchronise per group) and finishes the
// Forward scores (the logarithm is the host's).  The Gumbel fits follow in wh_build.cpp.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "wh_calibrate.h"
#include "wh_devbuf.h"

namespace wh {

using namespace whc;

namespace {

constexpr int kThreads = 256;                    // 200 lanes with a sequence, in four waves
constexpr size_t kLdsLimit = 65536;              // the filters' tables in LDS up to here (two workgroups per CU)

// one model of a group, as the kernel reads it
struct CalibDesc {
  int M, K;
  CalibMSVPar msv;
  CalibVitPar vit;
  double pmove, ploop;
  unsigned long long rb, rw, tw, ft, em;         // byte offsets of its tables in the group's table block (16-byte aligned)
  unsigned long long ws;                         // byte offset of its rows in the workspace
  int lds;                                       // the two filters read their tables from LDS
  int pad;
};

struct CalibArgs {
  const CalibDesc *desc;
  const unsigned char *tables;
  unsigned char *ws;
  const uint8_t *dsq[3];                         // [L + 1][kCalibN] each: residue i of sequence n at i * kCalibN + n
  int *msv, *vit, *nscale;                       // [models of the group][kCalibN]
  double *fwd;
};

__host__ __device__ inline size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }
__host__ __device__ inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

// the rows of one model: MSV 2 rows of bytes, Viterbi 6 rows of words, Forward 6 rows of doubles, and the Forward's
// rescale factors (one per residue at most), all kCalibN lanes wide
__host__ __device__ inline size_t ws_msv_bytes(int M) { return (size_t)2 * (size_t)(M + 1) * kCalibN; }
__host__ __device__ inline size_t ws_vit_bytes(int M) { return (size_t)6 * (size_t)(M + 1) * kCalibN * 2; }
inline size_t ws_fwd_bytes(int M) { return (size_t)6 * (size_t)(M + 1) * kCalibN * 8; }
inline size_t ws_bytes(int M) { return up256(ws_msv_bytes(M) + ws_vit_bytes(M) + ws_fwd_bytes(M) + (size_t)kCalibEfL * kCalibN * 8); }
inline size_t table_bytes(int M, int K) {
  const size_t W = (size_t)M + 1;
  return up256(up16(K * W) + up16(2 * K * W) + up16(16 * W) + up16(64 * W) + up16(8 * K * W));
}
inline size_t lds_bytes(int M, int K) {
  const size_t W = (size_t)M + 1;
  return std::max(up16(K * W), up16(2 * K * W) + up16(16 * W));
}

// <n16> 16-byte pieces from global memory into LDS, by the whole workgroup
__device__ inline void stage(uint4 *dst, const unsigned char *src, size_t n16) {
  const uint4 *s = reinterpret_cast<const uint4 *>(src);
  for (size_t i = threadIdx.x; i < n16; i += kThreads) dst[i] = s[i];
}

__global__ __launch_bounds__(kThreads) void calib_kernel(CalibArgs a) {
  extern __shared__ uint4 smem[];
  const CalibDesc d = a.desc[blockIdx.y];
  const int phase = blockIdx.x, lane = threadIdx.x;
  const int M = d.M, K = d.K;
  const size_t W = (size_t)M + 1, S = kCalibN;
  const bool active = lane < kCalibN;
  const size_t out = (size_t)blockIdx.y * kCalibN + (size_t)lane;
  unsigned char *ws = a.ws + d.ws;
  if (phase == 2) {              // ---- MSV
    const uint8_t *rb = a.tables + d.rb;
    const CalibRow<const uint8_t> dsq{a.dsq[0] + (active ? lane : 0), S};
    const CalibRow<uint8_t> r0{ws + (active ? lane : 0), S}, r1 = r0.plus(W);
    if (d.lds) {
      stage(smem, rb, up16(K * W) / 16);
      __syncthreads();
      if (active) a.msv[out] = calib_msv_core(M, d.msv, reinterpret_cast<const uint8_t *>(smem), dsq, kCalibEmL, r0, r1);
    } else if (active) a.msv[out] = calib_msv_core(M, d.msv, rb, dsq, kCalibEmL, r0, r1);
  } else if (phase == 1) {       // ---- Viterbi
    const int16_t *rw = reinterpret_cast<const int16_t *>(a.tables + d.rw), *tw = reinterpret_cast<const int16_t *>(a.tables + d.tw);
    const CalibRow<const uint8_t> dsq{a.dsq[1] + (active ? lane : 0), S};
    const CalibRow<int16_t> r0{reinterpret_cast<int16_t *>(ws + ws_msv_bytes(M)) + (active ? lane : 0), S}, r1 = r0.plus(3 * W);
    if (d.lds) {
      const size_t n_rw = up16(2 * K * W) / 16;
      stage(smem, a.tables + d.rw, n_rw);
      stage(smem + n_rw, a.tables + d.tw, W);
      __syncthreads();
      if (active)
        a.vit[out] = calib_viterbi_core(M, d.vit, reinterpret_cast<const int16_t *>(smem), reinterpret_cast<const int16_t *>(smem + n_rw), dsq,
                                        kCalibEvL, r0, r1);
    } else if (active) a.vit[out] = calib_viterbi_core(M, d.vit, rw, tw, dsq, kCalibEvL, r0, r1);
  } else if (active) {           // ---- Forward
    const double *ft = reinterpret_cast<const double *>(a.tables + d.ft), *em = reinterpret_cast<const double *>(a.tables + d.em);
    const CalibRow<const uint8_t> dsq{a.dsq[2] + lane, S};
    double *rows = reinterpret_cast<double *>(ws + ws_msv_bytes(M) + ws_vit_bytes(M));
    const CalibRow<double> r0{rows + lane, S}, r1 = r0.plus(3 * W), sc = r0.plus(6 * W);
    int ns = 0;
    a.fwd[out] = calib_forward_core(M, ft, em, d.pmove, d.ploop, dsq, kCalibEfL, r0, r1, sc, &ns);
    a.nscale[out] = ns;
  }
}

struct Stream {
  hipStream_t s = nullptr;
  ~Stream() { if (s) (void)hipStreamDestroy(s); }
};

}  // namespace

int calibrate_device(int device, int n, const CalibPrep *preps, const CalibSeqs &seqs, int flags, int *msv, int *vit, double *fwd) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) {
    set_error("wh_hmmbuild_batch: no HIP device %d (%d visible; device < 0 calibrates on the host)", device, ndev);
    return WH_ENODEV;
  }
  HIPCHK(hipSetDevice(device));
  // ---- the budget of one group: rows and tables of its models
  size_t budget = (size_t)1 << 30;
  if (const char *env = getenv("WH_CALIB_WS_MB")) {
    const long mb = atol(env);
    if (mb > 0) budget = (size_t)mb << 20;
  }
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  if (budget > free_b / 2) budget = free_b / 2;
  std::vector<size_t> need((size_t)n);
  for (int i = 0; i < n; i++) {
    const int M = preps[i].msv.M, K = preps[i].msv.K;
    need[(size_t)i] = ws_bytes(M) + table_bytes(M, K);
    if (need[(size_t)i] > budget) {
      set_error("wh_hmmbuild_batch: model %d (%d nodes) needs %zu bytes of calibration workspace on the device (rows %zu, tables %zu); "
                "the budget is %zu bytes (WH_CALIB_WS_MB or 1 GiB, and half of the %zu bytes free)",
                i, M, need[(size_t)i], ws_bytes(M), table_bytes(M, K), budget, free_b);
      return WH_ENOMEM;
    }
  }
  // ---- groups of consecutive models that fit it
  std::vector<int> first;      // first model of every group, and n
  size_t biggest = 0;
  {
    size_t sum = 0;
    for (int i = 0; i < n; i++) {
      if (i == 0 || sum + need[(size_t)i] > budget || i - first.back() >= 65535) { first.push_back(i); sum = 0; }      // (65 535: the grid's y limit)
      sum += need[(size_t)i];
      biggest = std::max(biggest, sum);
    }
    first.push_back(n);
  }
  int gmax = 0;
  for (size_t g = 0; g + 1 < first.size(); g++) gmax = std::max(gmax, first[g + 1] - first[g]);
  // ---- device memory: one block for rows and tables, the sequences, the descriptors, the results
  DevBuf d_blk, d_seq, d_desc, d_res;
  Stream st;
  size_t seq_off[3], seq_bytes = 0;
  for (int ph = 0; ph < 3; ph++) { seq_off[ph] = seq_bytes; seq_bytes += up256((size_t)(seqs.L[ph] + 1) * kCalibN); }
  const size_t res_int = up256((size_t)gmax * kCalibN * sizeof(int)), res_dbl = up256((size_t)gmax * kCalibN * sizeof(double));
  if (d_blk.ensure(biggest) || d_seq.ensure(seq_bytes) || d_desc.ensure((size_t)gmax * sizeof(CalibDesc)) || d_res.ensure(3 * res_int + res_dbl)) {
    set_error("wh_hmmbuild_batch: hipMalloc of the calibration workspace failed (%zu bytes for the largest of %zu groups, %zu bytes free)",
              biggest, first.size() - 1, free_b);
    return WH_ENOMEM;
  }
  HIPCHK(hipStreamCreate(&st.s));
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&calib_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsLimit));
  {
    std::vector<uint8_t> t(seq_bytes, 0);      // sequence-major on the host, residue-major (lanes adjacent) on the device
    for (int ph = 0; ph < 3; ph++)
      for (int s = 0; s < kCalibN; s++)
        for (int i = 1; i <= seqs.L[ph]; i++) t[seq_off[ph] + (size_t)i * kCalibN + (size_t)s] = seqs.seq(ph, s)[i];
    HIPCHK(hipMemcpyAsync(d_seq.p, t.data(), seq_bytes, hipMemcpyHostToDevice, st.s));
    HIPCHK(hipStreamSynchronize(st.s));
  }
  std::vector<unsigned char> tab;
  std::vector<CalibDesc> desc;
  std::vector<int> h_msv, h_vit, h_ns;
  std::vector<double> h_fwd, h_sc;
  for (size_t g = 0; g + 1 < first.size(); g++) {
    const int lo = first[g], cnt = first[g + 1] - lo;
    // tables first, rows behind them
    size_t tbytes = 0;
    for (int i = lo; i < lo + cnt; i++) tbytes += table_bytes(preps[i].msv.M, preps[i].msv.K);
    tab.assign(tbytes, 0);
    desc.assign((size_t)cnt, CalibDesc());
    size_t toff = 0, woff = tbytes, lds = 0;
    for (int i = lo; i < lo + cnt; i++) {
      const CalibPrep &p = preps[i];
      const int M = p.msv.M, K = p.msv.K;
      const size_t W = (size_t)M + 1;
      CalibDesc &d = desc[(size_t)(i - lo)];
      d.M = M; d.K = K;
      d.msv = calib_msv_par(p.msv);
      d.vit = calib_vit_par(p.vit);
      d.pmove = p.fwd.pmove; d.ploop = p.fwd.ploop;
      size_t o = toff;
      d.rb = o; memcpy(&tab[o], p.msv.rb.data(), K * W); o += up16(K * W);
      d.rw = o; memcpy(&tab[o], p.vit.rw.data(), 2 * K * W); o += up16(2 * K * W);
      d.tw = o; memcpy(&tab[o], p.vit.tw.data(), 16 * W); o += up16(16 * W);
      d.ft = o; memcpy(&tab[o], p.fwd.ft.data(), 64 * W); o += up16(64 * W);
      d.em = o; memcpy(&tab[o], p.fwd.em.data(), 8 * K * W); o += up16(8 * K * W);
      toff += table_bytes(M, K);
      d.ws = woff;
      woff += ws_bytes(M);
      d.lds = !(flags & WH_BUILD_CALIB_NO_LDS) && lds_bytes(M, K) <= kLdsLimit;
      if (d.lds) lds = std::max(lds, lds_bytes(M, K));
    }
    if (woff > biggest) { set_error("wh_hmmbuild_batch: internal error: group %zu needs %zu bytes, %zu were planned", g, woff, biggest); return WH_EINVAL; }
    HIPCHK(hipMemcpyAsync(d_blk.p, tab.data(), tbytes, hipMemcpyHostToDevice, st.s));
    HIPCHK(hipMemcpyAsync(d_desc.p, desc.data(), (size_t)cnt * sizeof(CalibDesc), hipMemcpyHostToDevice, st.s));
    CalibArgs a;
    a.desc = (const CalibDesc *)d_desc.p;
    a.tables = (const unsigned char *)d_blk.p;
    a.ws = (unsigned char *)d_blk.p;
    for (int ph = 0; ph < 3; ph++) a.dsq[ph] = (const uint8_t *)d_seq.p + seq_off[ph];
    a.msv = (int *)d_res.p;
    a.vit = (int *)((char *)d_res.p + res_int);
    a.nscale = (int *)((char *)d_res.p + 2 * res_int);
    a.fwd = (double *)((char *)d_res.p + 3 * res_int);
    hipLaunchKernelGGL(calib_kernel, dim3(3, (unsigned)cnt), dim3(kThreads), lds, st.s, a);
    HIPCHK(hipGetLastError());
    const size_t nres = (size_t)cnt * kCalibN;
    h_ns.resize(nres); h_fwd.resize(nres);
    HIPCHK(hipMemcpyAsync(msv + (size_t)lo * kCalibN, a.msv, nres * sizeof(int), hipMemcpyDeviceToHost, st.s));
    HIPCHK(hipMemcpyAsync(vit + (size_t)lo * kCalibN, a.vit, nres * sizeof(int), hipMemcpyDeviceToHost, st.s));
    HIPCHK(hipMemcpyAsync(h_ns.data(), a.nscale, nres * sizeof(int), hipMemcpyDeviceToHost, st.s));
    HIPCHK(hipMemcpyAsync(h_fwd.data(), a.fwd, nres * sizeof(double), hipMemcpyDeviceToHost, st.s));
    HIPCHK(hipStreamSynchronize(st.s));
    // the Forward scores: the logarithms are the host's; the rescale factors are fetched only where a sweep rescaled
    for (int i = lo; i < lo + cnt; i++) {
      const int M = preps[i].msv.M;
      const int *ns = &h_ns[(size_t)(i - lo) * kCalibN];
      bool any = false;
      for (int s = 0; s < kCalibN; s++) any = any || ns[s] > 0;
      if (any) {
        h_sc.resize((size_t)kCalibEfL * kCalibN);
        const size_t off = desc[(size_t)(i - lo)].ws + ws_msv_bytes(M) + ws_vit_bytes(M) + ws_fwd_bytes(M);
        HIPCHK(hipMemcpy(h_sc.data(), (char *)d_blk.p + off, h_sc.size() * sizeof(double), hipMemcpyDeviceToHost));
      }
      for (int s = 0; s < kCalibN; s++)
        fwd[(size_t)i * kCalibN + (size_t)s] = calib_forward_score(h_fwd[(size_t)(i - lo) * kCalibN + (size_t)s], any ? h_sc.data() + s : nullptr, kCalibN, ns[s]);
    }
  }
  return WH_OK;
}

}  // namespace wh
