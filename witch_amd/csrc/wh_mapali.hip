// hmmalign --mapali: the rows of the alignment a model was built from become sequences of the alignment assembly
// (wh_msa.hip).  A residue of such a row goes by its alignment COLUMN, not by a path: the column of
// node k (the model's MAP annotation) is node k's, a column between the columns of nodes k and k + 1 is an insert of block
// k.  The host turns MAP into one code per column (colcode: node - 1, or -(k + 2) for block k); the kernels here compact
// every row to its residues, the form the assembly kernels read:
//   mapali_count_kernel  one wavefront per row, consecutive lanes on consecutive bytes: a 64-bit ballot of "is a residue"
//                        per 64 columns, popcounts summed wave-uniformly -> count[row].  The host reads the counts back
//                        once and forms the CSR (as wh_domains_dev does with its counts);
//   mapali_map_kernel    one wavefront per row: a lane's rank among the residues of its 64 columns is the popcount of the
//                        ballot below the lane, the base of the 64 columns is carried wave-uniformly; the residue's
//                        character and its column's code go to text / cols at off[row] + base + rank.  The workgroups
//                        behind the rows write the offsets of the concatenation [rows | new sequences].
// Byte work, bound by HBM: n_map x alen bytes read twice, 5 bytes written per residue.
#include <hip/hip_runtime.h>

#include "wh_launch.h"

namespace wh {

__device__ __forceinline__ bool mapali_is_residue(uint8_t ch) { return (uint8_t)((ch | 32) - 'a') < 26; }

__global__ __launch_bounds__(64) void mapali_count_kernel(MapaliArgs a) {
  const int64_t row = blockIdx.x;
  const uint8_t *src = a.rows + (size_t)row * (size_t)a.alen;
  const int lane = threadIdx.x;
  int n = 0;                                                            // wave-uniform
  for (int64_t c0 = 0; c0 < a.alen; c0 += 64) {
    const int64_t c = c0 + lane;
    const bool res = c < a.alen && mapali_is_residue(src[c]);
    n += __popcll(__ballot(res));
  }
  if (lane == 0) a.count[row] = n;
}

__global__ __launch_bounds__(64) void mapali_map_kernel(MapaliArgs a) {
  const int lane = threadIdx.x;
  if ((int64_t)blockIdx.x >= a.n_map) {                                 // the offsets of the new sequences, behind the rows'
    const int64_t i = ((int64_t)blockIdx.x - a.n_map) * 64 + lane;
    if (i <= a.nq) a.all_off[a.n_map + i] = (a.nq > 0 ? a.seq_off[i] : 0) + a.shift;
    return;
  }
  const int64_t row = blockIdx.x;
  const uint8_t *src = a.rows + (size_t)row * (size_t)a.alen;
  const int64_t lo = a.off[row], hi = a.off[row + 1];
  if (lane == 0) a.all_off[row] = lo;
  int64_t base = lo;                                                    // wave-uniform
  for (int64_t c0 = 0; c0 < a.alen; c0 += 64) {
    const int64_t c = c0 + lane;
    const uint8_t ch = c < a.alen ? src[c] : (uint8_t)'-';
    const bool res = mapali_is_residue(ch);
    const unsigned long long b = __ballot(res);
    const int64_t at = base + __popcll(b & ((1ull << lane) - 1ull));
    if (res && at < hi) { a.text[at] = ch; a.cols[at] = a.colcode[c]; }
    base += __popcll(b);
  }
}

hipError_t launch_mapali_count(const MapaliArgs &a, hipStream_t s) {
  if (a.n_map > 0) hipLaunchKernelGGL(mapali_count_kernel, dim3((unsigned)a.n_map), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_mapali_map(const MapaliArgs &a, hipStream_t s) {
  const unsigned extra = (unsigned)((a.nq + 1 + 63) / 64);
  hipLaunchKernelGGL(mapali_map_kernel, dim3((unsigned)a.n_map + extra), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace wh
