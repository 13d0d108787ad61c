// hmmsearch -A: the alignment of all hits that satisfy the inclusion thresholds (wh_hits_msa_dev).  The stage between the
// domain alignments (wh_domain_paths_dev: per envelope residue its node and posterior) and the alignment assembly
// (wh_msa_dev): decide inclusion, order and compact the included domains, slice each to its aligned range.
//
// Replaces what HMMER 3.1b2 does on the host for `hmmsearch -A FILE` (p7_tophits_Alignment: one trace per included domain,
// cut to ali_i..ali_j, posteriors decoded from the displayed PP characters, then p7_tracealign_*).
//   hits_mark_kernel        one thread per domain: included (its pair is of model h and reported, the sequence's and the
//                           domain's ln P are at or below the thresholds the host took the logarithm of, it has a path) and
//                           the length of its slice; the record is checked against dom_off, the envelope CSR and the query
//   hits_block_scan_kernel  one thread per output position i (query order[i]): rows and residues of the query's included
//                           domains, exclusive scan inside the workgroup (wave shuffles, then the waves' sums in LDS)
//   hits_top_scan_kernel    one workgroup: exclusive scan of the workgroups' sums, the two totals
//   hits_place_kernel       one thread per output position: row index, residue offset and record of each included domain
//   hits_slice_kernel       one wavefront per row: characters, columns and QUANTISED posteriors of residues ali_i..ali_j
// Integer and byte work, bound by HBM latency: a few bytes per envelope residue, nothing for MFMA.
#include <hip/hip_runtime.h>

#include "wh_launch.h"

namespace wh {

constexpr int kHitsScanThreads = 256;   // positions per workgroup of the scan
constexpr int kHitsWaves = 4;           // wavefronts per workgroup of the slice kernel

// HMMER's p7_alidisplay_EncodePostProb then _DecodePostProb on a float posterior: the character's arithmetic in double
// ('*' where p + 0.05 >= 1.0, else (int)(p * 10.0 + 0.5)), the value back as (float)d / 10
__device__ __forceinline__ float hits_quantise(float p) {
  if ((double)p + 0.05 >= 1.0) return 1.0f;
  int d = (int)((double)p * 10.0 + 0.5);
  d = d < 0 ? 0 : d > 9 ? 9 : d;
  return (float)d / 10.0f;
}

__global__ __launch_bounds__(256) void hits_mark_kernel(HitsArgs a) {
  const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= a.ndom) return;
  const wh_domain r = a.dom[d];
  const int64_t p = r.pair;
  int len = 0;
  if (p < 0 || p >= a.npairs || d < a.dom_off[p] || d >= a.dom_off[p + 1]) { *a.bad = 1; a.len[d] = 0; return; }
  if (p % a.H == a.h && (a.flags[p] & WH_FLAG_REPORTED) && r.ali_i != 0) {
    const int64_t q = p / a.H;
    const int64_t L = a.offsets[q + 1] - a.offsets[q];
    const int64_t elen = a.env_off[d + 1] - a.env_off[d];
    if (r.env_i < 1 || r.env_j > L || r.ali_i < r.env_i || r.ali_j > r.env_j || r.ali_i > r.ali_j || elen != (int64_t)r.env_j - r.env_i + 1) {
      *a.bad = 1; a.len[d] = 0; return;
    }
    // the sequence's ln P: min(0, -lambda (score - tau)) in double from the float32 fields; a model without the STATS line
    // has no E-values and every hit counts as included, as in the level-0 tables
    const bool nostats = a.tau != a.tau || a.lambda != a.lambda;
    const double sc = (double)a.detail[p].seq_score;
    const double lnps = sc < (double)a.tau ? 0.0 : -(double)a.lambda * (sc - (double)a.tau);
    const bool seq_in = nostats || lnps <= a.ln_inc_seq;
    const bool dom_in = r.lnP != r.lnP || (double)r.lnP <= a.ln_inc_dom;
    if (seq_in && dom_in) len = r.ali_j - r.ali_i + 1;
  }
  a.len[d] = len;                 // 0: not included
}

// rows and residues of the included domains of output position i
__device__ __forceinline__ void hits_position_counts(const HitsArgs &a, int64_t i, int *rows, long long *res) {
  *rows = 0; *res = 0;
  const int64_t q = a.order ? (int64_t)a.order[i] : i;
  if (q < 0 || q >= a.nq) { *a.bad = 1; return; }
  const int64_t p = q * a.H + a.h;
  int64_t lo = a.dom_off[p], hi = a.dom_off[p + 1];
  if (lo < 0 || hi > a.ndom || hi - lo > WH_MAX_ENVELOPES) { *a.bad = 1; return; }
  for (int64_t d = lo; d < hi; d++) { const int n = a.len[d]; *rows += n > 0; *res += n; }
}

__global__ __launch_bounds__(kHitsScanThreads) void hits_block_scan_kernel(HitsArgs a) {
  __shared__ int wrow[kHitsScanThreads / 64];
  __shared__ long long wres[kHitsScanThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t i = (int64_t)blockIdx.x * kHitsScanThreads + tid;
  int rows = 0;
  long long res = 0;
  if (i < a.nq) hits_position_counts(a, i, &rows, &res);
  // inclusive scan over the wavefront, then over the workgroup's wavefronts
  int srow = rows;
  long long sres = res;
  for (int m = 1; m < 64; m <<= 1) {
    const int orow = __shfl_up(srow, m);
    const long long ores = __shfl_up(sres, m);
    if (lane >= m) { srow += orow; sres += ores; }
  }
  if (lane == 63) { wrow[wave] = srow; wres[wave] = sres; }
  __syncthreads();
  int brow = 0;
  long long bres = 0;
  for (int w = 0; w < wave; w++) { brow += wrow[w]; bres += wres[w]; }
  if (i < a.nq) { a.pos_row[i] = brow + srow - rows; a.pos_res[i] = bres + sres - res; }
  if (tid == kHitsScanThreads - 1) { a.blk_row[blockIdx.x] = brow + srow; a.blk_res[blockIdx.x] = bres + sres; }
}

// exclusive scan of the nblk workgroup sums in place, 256 at a time with a carry; totals[0] = rows, totals[1] = residues
__global__ __launch_bounds__(kHitsScanThreads) void hits_top_scan_kernel(HitsArgs a) {
  __shared__ long long srow[kHitsScanThreads], sres[kHitsScanThreads];
  const int tid = threadIdx.x;
  long long crow = 0, cres = 0;
  for (int64_t base = 0; base < a.nblk; base += kHitsScanThreads) {
    const int64_t b = base + tid;
    const long long r0 = b < a.nblk ? a.blk_row[b] : 0, s0 = b < a.nblk ? a.blk_res[b] : 0;
    srow[tid] = r0; sres[tid] = s0;
    __syncthreads();
    for (int m = 1; m < kHitsScanThreads; m <<= 1) {
      const long long orow = tid >= m ? srow[tid - m] : 0, ores = tid >= m ? sres[tid - m] : 0;
      __syncthreads();
      srow[tid] += orow; sres[tid] += ores;
      __syncthreads();
    }
    if (b < a.nblk) { a.blk_row[b] = crow + srow[tid] - r0; a.blk_res[b] = cres + sres[tid] - s0; }
    crow += srow[kHitsScanThreads - 1]; cres += sres[kHitsScanThreads - 1];
    __syncthreads();
  }
  if (tid == 0) { a.totals[0] = crow; a.totals[1] = cres; }
}

// (launched after the host has checked the totals against the sizes of the row arrays)
__global__ __launch_bounds__(kHitsScanThreads) void hits_place_kernel(HitsArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kHitsScanThreads + threadIdx.x;
  if (i == 0) a.row_off[a.nrows] = a.nres;
  if (i >= a.nq) return;
  const int64_t q = a.order ? (int64_t)a.order[i] : i;
  if (q < 0 || q >= a.nq) return;
  const int64_t p = q * a.H + a.h;
  const int64_t lo = a.dom_off[p], hi = a.dom_off[p + 1];
  if (lo < 0 || hi > a.ndom || hi - lo > WH_MAX_ENVELOPES) return;
  int64_t row = a.blk_row[blockIdx.x] + a.pos_row[i];
  int64_t at = a.blk_res[blockIdx.x] + a.pos_res[i];
  for (int64_t d = lo; d < hi; d++) {
    const int n = a.len[d];
    if (n <= 0) continue;
    if (row >= a.nrows || at + n > a.nres) return;          // (an order[] that names a query twice: refused by the host)
    const wh_domain &r = a.dom[d];
    a.row_dom[row] = d;
    a.row_off[row] = at;
    wh_hit_row rec;
    rec.query = (int32_t)q; rec.index = r.index; rec.ali_i = r.ali_i; rec.ali_j = r.ali_j;
    a.row_rec[row] = rec;
    row++; at += n;
  }
}

__global__ __launch_bounds__(kHitsWaves * 64) void hits_slice_kernel(HitsArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * kHitsWaves + (threadIdx.x >> 6);
  if (row >= a.nrows) return;
  const int64_t d = a.row_dom[row];
  const wh_domain &r = a.dom[d];
  const int64_t q = r.pair / a.H;
  const int64_t at = a.row_off[row];
  // (ali_j - ali_i + 1, checked by the mark kernel: inside the envelope and the query; read from the CSR so that a row the
  // place kernel did not reach - the host refuses the call afterwards - copies nothing)
  const int64_t n = a.row_off[row + 1] - at;
  if (n != (int64_t)r.ali_j - r.ali_i + 1 || at < 0 || at + n > a.nres) return;
  const uint8_t *text = a.text + a.offsets[q] + (r.ali_i - 1);
  const int64_t env = a.env_off[d] + (r.ali_i - r.env_i);
  for (int i = lane; i < n; i += 64) {
    a.out_text[at + i] = text[i];
    a.out_cols[at + i] = a.cols[env + i];
    a.out_pp[at + i] = hits_quantise(a.pp[env + i]);
  }
}

static unsigned hits_blocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

hipError_t launch_hits_mark(const HitsArgs &a, hipStream_t s) {
  if (a.ndom > 0) hipLaunchKernelGGL(hits_mark_kernel, dim3(hits_blocks(a.ndom, 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}
int64_t hits_scan_blocks(int64_t nq) { return (nq + kHitsScanThreads - 1) / kHitsScanThreads; }
// the two levels of the scan; a.nblk = hits_scan_blocks(a.nq)
hipError_t launch_hits_scan(const HitsArgs &a, hipStream_t s) {
  if (a.nq > 0) hipLaunchKernelGGL(hits_block_scan_kernel, dim3((unsigned)a.nblk), dim3(kHitsScanThreads), 0, s, a);
  hipLaunchKernelGGL(hits_top_scan_kernel, dim3(1), dim3(kHitsScanThreads), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_hits_place(const HitsArgs &a, hipStream_t s) {
  if (a.nq > 0) hipLaunchKernelGGL(hits_place_kernel, dim3((unsigned)a.nblk), dim3(kHitsScanThreads), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_hits_slice(const HitsArgs &a, hipStream_t s) {
  if (a.nrows > 0) hipLaunchKernelGGL(hits_slice_kernel, dim3(hits_blocks(a.nrows, kHitsWaves)), dim3(kHitsWaves * 64), 0, s, a);
  return hipGetLastError();
}

}  // namespace wh
