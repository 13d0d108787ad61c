// hmmalign's alignment of MANY sequences to one model, assembled on the device (what HMMER's
// p7_tracealign_Seqs does on the host).  Input: what wh_align_pp_dev left in HBM for nq sequences against the model - per
// residue its node (or -1) and the posterior of its state - and the sequences' characters.  Layout rules (pinned by
// tests/golden/msa against the bundled 3.1b2 binary): every node is a column; block k (0..M) between the columns of nodes k
// and k + 1 is as wide as the LONGEST insert run any sequence has there; N-flank residues (block 0) are right-justified,
// C-flank residues (block M) left-justified, an internal run of n puts its first n / 2 residues flush left and the rest
// flush right; --trim drops both flanks.  A residue's code may also NAME its block, -(k + 2), whatever surrounds it - the
// rows of a --mapali alignment (wh_mapali.hip), the first n_nopp sequences: they carry no posteriors, get no PP row and
// take no part in PP_cons.
//   msa_widths_kernel   one wavefront per sequence; the thread that finds the first residue of an insert run walks it:
//                       run length -> atomicMax into width[block] (integer max: order-independent), per residue its block and
//                       its cell (from the left end, or from the right end) - the render kernel then needs no second walk;
//   msa_layout_kernel   one workgroup: exclusive scan of width -> first column of every block, matmap, W; the RF line and
//                       the insert columns of PP_cons;
//   msa_render_kernel   one workgroup per sequence: the sequence row and its PP row, built in LDS and streamed out in
//                       16-byte stores (or, beyond the LDS budget, written in place), and the sequence's row of the
//                       node-major posterior matrix the PP_cons kernel reads;
//   msa_cons_kernel     one thread per node, walking the sequences of a chunk in order: sequential float32 sums (no
//                       floating-point atomics anywhere), loads coalesced across nodes.
// HBM-bound byte work: 2 x nq x W bytes written once; nothing to do with MFMA.
#include <hip/hip_runtime.h>

#include "wh_launch.h"

namespace wh {

constexpr int kMsaRenderThreads = 256;

__device__ __forceinline__ bool msa_is_match(int c, int M) { return (unsigned)c < (unsigned)M; }

// hmmalign's character for a posterior (formats.pp_char: the same float64 arithmetic)
__device__ __forceinline__ uint8_t msa_pp_char(float p) {
  const double v = (double)p + 0.05;
  if (v >= 1.0) return '*';
  int d = (int)(v * 10.0);
  d = d < 0 ? 0 : d > 9 ? 9 : d;
  return (uint8_t)('0' + d);
}

// a residue's insert block where its code names it: -(k + 2) -> k
__device__ __forceinline__ int msa_code_block(int c) { return -(c + 2); }

// NAMED: the codes -(k + 2) have their meaning (a call with --mapali rows); without, the kernel is wh_msa's as it always was
template <bool NAMED>
__global__ __launch_bounds__(64) void msa_widths_kernel(MsaArgs a) {
  const int64_t q = blockIdx.x;
  const int64_t lo = a.off[q], hi = a.off[q + 1] < a.total ? a.off[q + 1] : a.total;
  for (int64_t r = lo + threadIdx.x; r < hi; r += blockDim.x) {
    const int c0 = a.cols[r];
    if (msa_is_match(c0, a.M)) continue;
    // a run: residues outside the match columns that share a block.  A code of -1 (or any other value without a meaning)
    // takes its block from what surrounds it, so such a run ends at the next match residue or explicit code; a code
    // -(k + 2), k in 0..M, names block k, so a run ends where the code changes, even with no match residue between.
    const bool named = NAMED && c0 <= -2 && c0 >= -(a.M + 2);
    auto in_run = [&](int c) {
      if (!NAMED) return !msa_is_match(c, a.M);
      return named ? c == c0 : !msa_is_match(c, a.M) && !(c <= -2 && c >= -(a.M + 2));
    };
    if (r > lo && in_run(a.cols[r - 1])) continue;                    // inside a run: its first residue's thread walks it
    int64_t e = r + 1;
    while (e < hi && in_run(a.cols[e])) e++;
    const int64_t n = e - r;
    bool nflank, cflank;
    int blk;
    if (named) {
      blk = msa_code_block(c0);
      nflank = blk == 0; cflank = blk == a.M;
      if ((nflank || cflank) && a.trim) blk = -1;
    } else {
      nflank = r == lo; cflank = e == hi;
      if (nflank && cflank) { blk = -1; if (!NAMED || q >= a.n_nopp) atomicAdd(a.pathless, 1); }     // no match state at all: gaps only, counted
      else if (nflank) blk = a.trim ? -1 : 0;
      else if (cflank) blk = a.trim ? -1 : a.M;
      else { const int p = a.cols[r - 1]; blk = !NAMED || msa_is_match(p, a.M) ? p + 1 : msa_code_block(p); }
    }
    if (blk >= 0) atomicMax(a.width + blk, (int)n);
    for (int64_t i = 0; i < n; i++) {
      a.res_blk[r + i] = blk;
      a.res_k[r + i] = nflank ? (int)(i - n) : cflank ? (int)i : i < n / 2 ? (int)i : (int)(i - n);
    }
  }
}

// layout[g] = sum_{g' < g} width[g'] + g ; matmap[g] = layout[g] + width[g] ; layout[M + 1] = W
__global__ __launch_bounds__(256) void msa_layout_kernel(MsaArgs a) {
  __shared__ long long part[256];
  const int t = threadIdx.x, n = a.M + 1;
  const int per = (n + 255) / 256, lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
  long long s = 0;
  for (int g = lo; g < hi; g++) s += a.width[g];
  part[t] = s;
  __syncthreads();
  if (t == 0) { long long run = 0; for (int u = 0; u < 256; u++) { const long long v = part[u]; part[u] = run; run += v; } a.layout[a.M + 1] = run + a.M; }
  __syncthreads();
  long long run = part[t];
  for (int g = lo; g < hi; g++) {
    const long long first = run + g;
    const int w = a.width[g];
    a.layout[g] = first;
    for (int j = 0; j < w; j++) { a.rf[first + j] = '.'; a.pp_cons[first + j] = '.'; }
    if (g < a.M) { a.matmap[g] = (int32_t)(first + w); a.rf[first + w] = 'x'; a.pp_cons[first + w] = '.'; }
    run += w;
  }
}

// the two rows of one sequence.  LDS: both rows are built in LDS, each at the offset its global row has inside a 16-byte
// line, so that aligned 16-byte pieces of LDS are aligned 16-byte pieces of the output; the unaligned head and tail of a
// row go out byte by byte.  Without LDS the rows are built in place.
// PP: the sequences of the launch have posteriors (false: the rows of a --mapali alignment, the sequence row alone)
template <bool LDS, bool PP>
__global__ __launch_bounds__(kMsaRenderThreads) void msa_render_kernel(MsaArgs a) {
  extern __shared__ __align__(16) uint8_t msa_smem[];
  const int64_t q = a.q0 + blockIdx.x;
  const long long W = a.layout[a.M + 1];
  const int tid = threadIdx.x;
  constexpr bool has_pp = PP;
  uint8_t *grow = a.rows + (size_t)q * (size_t)W, *gpp = has_pp ? a.pp_rows + (size_t)(q - a.n_nopp) * (size_t)W : nullptr;
  const size_t stride = (size_t)((W + 30) >> 4) << 4;
  const int shift_row = LDS ? (int)(reinterpret_cast<uintptr_t>(grow) & 15) : 0;
  const int shift_pp = LDS ? (int)(reinterpret_cast<uintptr_t>(gpp) & 15) : 0;
  uint8_t *row = LDS ? msa_smem + shift_row : grow;
  uint8_t *ppr = LDS ? msa_smem + stride + shift_pp : gpp;
  float *ppm = has_pp ? a.ppm + (size_t)blockIdx.x * (size_t)a.M : nullptr;
  const float *pp = a.pp - a.pp_shift;
  for (long long c = tid; c < W; c += kMsaRenderThreads) { row[c] = a.rf[c] == 'x' ? '-' : '.'; if (has_pp) ppr[c] = '.'; }
  if (has_pp) for (int k = tid; k < a.M; k += kMsaRenderThreads) ppm[k] = -1.0f;
  __syncthreads();
  const int64_t lo = a.off[q], hi = a.off[q + 1] < a.total ? a.off[q + 1] : a.total;
  for (int64_t r = lo + tid; r < hi; r += kMsaRenderThreads) {
    uint8_t ch = a.text[r];
    const bool alpha = (ch >= 'A' && ch <= 'Z') || (ch >= 'a' && ch <= 'z');
    const int c = a.cols[r];
    long long at;
    if (msa_is_match(c, a.M)) {
      if (alpha) ch &= 0xDF;
      at = a.matmap[c];
      if (has_pp) ppm[c] = pp[r];
    } else {
      const int b = a.res_blk[r];
      if (b < 0) continue;                             // a trimmed flank, a sequence without a path
      if (alpha) ch |= 32;
      const int k = a.res_k[r];
      at = a.layout[b] + (k >= 0 ? k : a.width[b] + k);
    }
    row[at] = ch;
    if (has_pp) ppr[at] = msa_pp_char(pp[r]);
  }
  if (!LDS) return;
  __syncthreads();
  for (int which = 0; which < (has_pp ? 2 : 1); which++) {
    uint8_t *dst = which ? gpp : grow;
    const uint8_t *src = which ? ppr : row;
    const int shift = which ? shift_pp : shift_row;
    const long long head = shift ? (16 - shift < W ? 16 - shift : W) : 0;
    const long long nvec = (W - head) >> 4, tail = head + (nvec << 4);
    if (tid < head) dst[tid] = src[tid];
    const uint4 *s16 = reinterpret_cast<const uint4 *>(src + head);       // (shift + head is 0 or 16: aligned in LDS)
    uint4 *d16 = reinterpret_cast<uint4 *>(dst + head);
    for (long long i = tid; i < nvec; i += kMsaRenderThreads) d16[i] = s16[i];
    if (tail + tid < W) dst[tail + tid] = src[tail + tid];
  }
}

// HMMER's own arithmetic for PP_cons (p7_tracealign.c: the rows' float posteriors summed in a double, divided by (float) n,
// the quotient handed to p7_alidisplay_EncodePostProb(float)): WH_MSA_CONS_HMMER, which the alignment of hmmsearch -A sets
__device__ __forceinline__ uint8_t msa_pp_char_hmmer(float p) {
  const double v = (double)p;
  if (v + 0.05 >= 1.0) return '*';
  int d = (int)(v * 10.0 + 0.5);
  d = d < 0 ? 0 : d > 9 ? 9 : d;
  return (uint8_t)('0' + d);
}

__global__ __launch_bounds__(64) void msa_cons_kernel(MsaArgs a) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= a.M) return;
  if (a.cons_sum64) {
    double s = a.cons_sum64[k];
    int n = a.cons_cnt[k];
    const float *col = a.ppm + k;
    const int64_t rows = a.q1 - a.q0;
    for (int64_t q = 0; q < rows; q++) {
      const float v = col[(size_t)q * (size_t)a.M];
      if (v > -0.5f) { s += (double)v; n++; }
    }
    a.cons_sum64[k] = s;
    a.cons_cnt[k] = n;
    if (a.last) a.pp_cons[a.matmap[k]] = n ? msa_pp_char_hmmer((float)(s / (double)(float)n)) : '.';
    return;
  }
  float s = a.cons_sum[k];
  int n = a.cons_cnt[k];
  const float *col = a.ppm + k;
  const int64_t rows = a.q1 - a.q0;
#pragma unroll 8
  for (int64_t q = 0; q < rows; q++) {
    const float v = col[(size_t)q * (size_t)a.M];
    if (v > -0.5f) { s += v; n++; }
  }
  a.cons_sum[k] = s;
  a.cons_cnt[k] = n;
  if (a.last) a.pp_cons[a.matmap[k]] = n ? msa_pp_char(s / (float)n) : '.';
}

size_t msa_render_lds_bytes(long long W) { return 2 * ((size_t)((W + 30) >> 4) << 4); }

hipError_t launch_msa_widths(const MsaArgs &a, hipStream_t s) {
  if (a.nq > 0 && a.n_nopp > 0) hipLaunchKernelGGL(msa_widths_kernel<true>, dim3((unsigned)a.nq), dim3(64), 0, s, a);
  else if (a.nq > 0) hipLaunchKernelGGL(msa_widths_kernel<false>, dim3((unsigned)a.nq), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_msa_layout(const MsaArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(msa_layout_kernel, dim3(1), dim3(256), 0, s, a);
  return hipGetLastError();
}

// the sequences q0 .. q1 - 1 (all with posteriors or all without: ppm holds the rows of a chunk from its row 0); <lds>: the caller checked msa_render_lds_bytes(W) against kMsaLdsBudget
hipError_t launch_msa_render(const MsaArgs &a, long long W, bool lds, hipStream_t s) {
  const unsigned n = (unsigned)(a.q1 - a.q0);
  if (n == 0) return hipSuccess;
  const bool pp = a.q0 >= a.n_nopp;
  if (!pp && a.q1 > a.n_nopp) return hipErrorInvalidValue;
  if (lds) {
    if (msa_render_lds_bytes(W) > kMsaLdsBudget) return hipErrorInvalidValue;
    if (pp) hipLaunchKernelGGL((msa_render_kernel<true, true>), dim3(n), dim3(kMsaRenderThreads), msa_render_lds_bytes(W), s, a);
    else hipLaunchKernelGGL((msa_render_kernel<true, false>), dim3(n), dim3(kMsaRenderThreads), msa_render_lds_bytes(W), s, a);
  } else {
    if (pp) hipLaunchKernelGGL((msa_render_kernel<false, true>), dim3(n), dim3(kMsaRenderThreads), 0, s, a);
    else hipLaunchKernelGGL((msa_render_kernel<false, false>), dim3(n), dim3(kMsaRenderThreads), 0, s, a);
  }
  return hipGetLastError();
}

hipError_t launch_msa_cons(const MsaArgs &a, hipStream_t s) {
  if (a.M > 0) hipLaunchKernelGGL(msa_cons_kernel, dim3((unsigned)((a.M + 63) / 64)), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace wh
