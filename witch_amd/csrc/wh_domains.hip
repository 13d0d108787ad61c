// Per-domain results of a scoring call (wh_domains_dev): the kernels around the alignment of the envelopes.
//
// Replaces hmmsearch's "Domain annotation for each sequence" section and its --domtblout file, which no reference code
// reads (evalHMMSearchOutput, witch_msa/gcmm/algorithm.py:579-605, parses the per-sequence table alone).  A domain is an
// envelope of a reported pair as the scoring kernels list it in wh_pair_detail; its alignment is wh_align_pp's alignment
// of the envelope's residues (wh_host_domains.hip runs it between envelope_gather_kernel and domain_summary_kernel).
//   domain_count_kernel     one thread per pair: the domains its record lists, the envelopes beyond them
//   domain_list_kernel      one thread per pair: the pair and the envelope length of each of its domains, checked
//   envelope_gather_kernel  one wavefront per domain: the envelope's residues into a packed array of its own (envelopes
//                           of one pair may overlap: a view into the query array cannot serve)
//   domain_summary_kernel   one wavefront per domain: end points, the sum of the path's posteriors, HMMER's per-domain
//                           score arithmetic, the record
#include <hip/hip_runtime.h>

#include "wh_launch.h"

namespace wh {

constexpr int kDomWaves = 4;   // wavefronts per workgroup of the one-wavefront-per-domain kernels

// domains the pair's record lists; <of>: its envelopes in all.  The scoring kernels cap nenv at the list's length: for a pair
// of the long-list pass (more regions than the list holds) the regions beyond the list stand for its further envelopes -
// one each unless such a region is multidomain, so <of> is then a lower bound.  A pair with at most that many regions but
// more envelopes (a multidomain region split many times) cannot be told from one with exactly the list's length: <of> = n
__device__ __forceinline__ int listed_domains(const DomainArgs &a, int64_t p, int *of) {
  *of = 0;
  if (!(a.flags[p] & WH_FLAG_REPORTED)) return 0;
  const wh_pair_detail &d = a.detail[p];
  const int n = d.nenv < 0 ? 0 : d.nenv > WH_MAX_ENVELOPES ? WH_MAX_ENVELOPES : d.nenv;
  *of = (n == WH_MAX_ENVELOPES && d.nregions > n) ? d.nregions : n;
  return n;
}

__global__ __launch_bounds__(256) void domain_count_kernel(DomainArgs a) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.npairs) return;
  int of;
  const int n = listed_domains(a, p, &of);
  a.counts[p] = n;
  if (a.n_unlisted) a.n_unlisted[p] = of - n;
}

// dom_off is the caller's: nothing is written through it before it is checked against the records and against ndom
__global__ __launch_bounds__(256) void domain_list_kernel(DomainArgs a) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.npairs) return;
  int of;
  const int n = listed_domains(a, p, &of);
  const int64_t lo = a.dom_off[p], hi = a.dom_off[p + 1];
  if (lo < 0 || hi > a.ndom || hi - lo != n || (p == 0 && lo != 0)) { *a.bad = 1; return; }
  const int64_t q = p / a.H;
  const int64_t L = a.offsets[q + 1] - a.offsets[q];
  const wh_pair_detail &d = a.detail[p];
  for (int t = 0; t < n; t++) {
    const int ei = d.env_i[t], ej = d.env_j[t];
    a.dom_pair[lo + t] = p;
    a.dom_len[lo + t] = (ei >= 1 && ei <= ej && ej <= L) ? ej - ei + 1 : -1;
    if (a.dom_seqlen) a.dom_seqlen[lo + t] = (int32_t)(L > 0x7FFFFFFF ? 0x7FFFFFFF : L);
  }
}

__global__ __launch_bounds__(kDomWaves * 64) void envelope_gather_kernel(DomainArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t d = (int64_t)blockIdx.x * kDomWaves + (threadIdx.x >> 6);
  if (d >= a.ndom) return;
  const int64_t p = a.dom_pair[d], q = p / a.H;
  const int t = (int)(d - a.dom_off[p]);
  const int len = a.dom_len[d];                                      // (checked on the host before this launch: >= 1)
  const uint8_t *src = a.residues + a.offsets[q] + (a.detail[p].env_i[t] - 1);
  uint8_t *dst = a.env_res + a.env_off[d];
  for (int i = lane; i < len; i += 64) dst[i] = src[i];
  if (lane == 0) { a.dom_q[d] = d; a.dom_h[d] = (int32_t)(p % a.H); }
}

// HMMER's per-domain score (p7_pipeline.c), in its order of operations and its types: floats, with the double
// intermediates that C's promotion of log() gives it.  logsum is evaluated exactly (HMMER's p7_FLogsum reads a table of
// 1/1000-nat steps: within 5e-4 nat of this)
__device__ __forceinline__ void domain_score(float envsc, float domcorr, int L, int Ld, float tau, float lambda,
                                             float *bits, float *bias_bits, float *lnP) {
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

__global__ __launch_bounds__(kDomWaves * 64) void domain_summary_kernel(DomainArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t d = (int64_t)blockIdx.x * kDomWaves + (threadIdx.x >> 6);
  if (d >= a.ndom) return;
  const int64_t p = a.dom_pair[d], q = p / a.H;
  const int h = (int)(p % a.H);
  const int t = (int)(d - a.dom_off[p]);
  const int Ld = a.dom_len[d];
  int of;
  (void)listed_domains(a, p, &of);
  const int32_t *cols = a.cols + a.env_off[d];
  const float *pp = a.pp + a.env_off[d];
  // lane r owns residues r, r + 64, ... in that order; then one butterfly over the lanes: the sum does not depend on the
  // launch shape
  int first = 0x7FFFFFFF, last = -1;
  float sum = 0.f;
  for (int i = lane; i < Ld; i += 64) {
    sum += pp[i];
    if (cols[i] >= 0) { first = first < i ? first : i; last = i; }
  }
  for (int m = 32; m >= 1; m >>= 1) {
    sum += __shfl_xor(sum, m);
    const int o1 = __shfl_xor(first, m), ol = __shfl_xor(last, m);
    first = o1 < first ? o1 : first;
    last = ol > last ? ol : last;
  }
  const wh_pair_detail &det = a.detail[p];
  const int ei = det.env_i[t], ej = det.env_j[t];
  const bool path = last >= 0;
  const int hmm_i = path ? cols[first] + 1 : 0, hmm_j = path ? cols[last] + 1 : 0;
  const int L = (int)(a.offsets[q + 1] - a.offsets[q]);
  float bits, bias, lnP;
  domain_score(det.envsc[t], det.domcorr[t], L, Ld, a.evp[2 * h], a.evp[2 * h + 1], &bits, &bias, &lnP);
  // the record is seven aligned 8-byte words: lanes 0..6 store one each, one store instruction over 56 contiguous bytes
  auto two = [](unsigned lo, unsigned hi) { return ((unsigned long long)hi << 32) | lo; };
  unsigned long long w;
  switch (lane) {
    case 0: w = (unsigned long long)p; break;
    case 1: w = two((unsigned)t, (unsigned)of); break;
    case 2: w = two((unsigned)ei, (unsigned)ej); break;
    case 3: w = two((unsigned)(path ? ei + first : 0), (unsigned)(path ? ei + last : 0)); break;
    case 4: w = two((unsigned)hmm_i, (unsigned)hmm_j); break;
    case 5: w = two(__float_as_uint(bits), __float_as_uint(bias)); break;
    default: w = two(__float_as_uint(sum), __float_as_uint(lnP)); break;
  }
  static_assert(sizeof(wh_domain) == 56 && alignof(wh_domain) == 8, "wh_domain is seven 8-byte words");
  if (lane < 7) reinterpret_cast<unsigned long long *>(a.out + d)[lane] = w;
}

static int blocks_of(int64_t n, int per_block) { return (int)((n + per_block - 1) / per_block); }

hipError_t launch_domain_count(const DomainArgs &a, hipStream_t s) {
  if (a.npairs <= 0) return hipSuccess;
  hipLaunchKernelGGL(domain_count_kernel, dim3(blocks_of(a.npairs, 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_domain_list(const DomainArgs &a, hipStream_t s) {
  if (a.npairs <= 0) return hipSuccess;
  hipLaunchKernelGGL(domain_list_kernel, dim3(blocks_of(a.npairs, 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_envelope_gather(const DomainArgs &a, hipStream_t s) {
  if (a.ndom <= 0) return hipSuccess;
  hipLaunchKernelGGL(envelope_gather_kernel, dim3(blocks_of(a.ndom, kDomWaves)), dim3(kDomWaves * 64), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_domain_summary(const DomainArgs &a, hipStream_t s) {
  if (a.ndom <= 0) return hipSuccess;
  hipLaunchKernelGGL(domain_summary_kernel, dim3(blocks_of(a.ndom, kDomWaves)), dim3(kDomWaves * 64), 0, s, a);
  return hipGetLastError();
}

}  // namespace wh
