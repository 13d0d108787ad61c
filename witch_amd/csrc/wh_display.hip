// hmmsearch's alignment display (wh_domain_display_dev): the four lines under "== domain N" - model consensus, match line,
// target, PP - of every reportable domain of model h, one character per alignment column.  The stage behind the domain
// alignments (wh_domain_paths_dev: per envelope residue its node and posterior).
//
// Replaces what HMMER 3.1b2 does on the host for every reported domain (p7_alidisplay_Create over the domain's trace).
//   display_count_kernel       one wavefront per domain: selected (its pair is of model h and reported, it has a path, its
//                              ln P is at or below the threshold the host took the logarithm of) and the columns of its
//                              lines; the record is checked against dom_off, the envelope CSR, the query and its own path
//   display_block_scan_kernel  one thread per domain: selected domains and columns in front of it, exclusive scan inside
//                              the workgroup (wave shuffles, then the waves' sums in LDS)
//   display_top_scan_kernel    one workgroup: exclusive scan of the workgroups' sums, the two totals
//   display_render_kernel      one wavefront per domain: its CSR entry, its record and every byte of its four lines
// Count and render walk the residues ali_i..ali_j 64 per trip with a carry between trips, and take a residue's column from
// ONE device function (display_columns), so the size the scan reserves and the bytes the render writes cannot disagree.
// Integer and byte work, bound by HBM latency: nothing for MFMA.  No memset, no atomic: every byte of a selected domain's
// range is written exactly once, by a plain vector byte store at a 64-bit offset.
#include <hip/hip_runtime.h>

#include "wh_launch.h"

namespace wh {

constexpr int kDispScanThreads = 256;   // domains per workgroup of the scan
constexpr int kDispWaves = 4;           // wavefronts (domains) per workgroup of the count and render kernels

// HMMER's p7_alidisplay_EncodePostProb on a float posterior, the arithmetic in double
__device__ __forceinline__ uint8_t display_pp_char(float p) {
  const double x = (double)p + 0.05;
  if (x >= 1.0) return '*';
  int d = (int)(x * 10.0);
  d = d < 0 ? 0 : d > 9 ? 9 : d;
  return (uint8_t)('0' + d);
}

// What the walk carries from one trip of 64 residues to the next: the inserts so far and the last match node (0-based).
struct DispCarry { int ins, prev; };
// A lane's residue in the lines: its column, the last match node in front of it and, for a match state, the delete states
// between the two (they take the columns col - gap .. col - 1)
struct DispLane { int col, gap, prev; };

// The column arithmetic of one trip, for count and render alike.  <node>: the lane's 0-based node, -1 for an insert;
// <valid>: the lane holds a residue of ali_i..ali_j; <hmm0>: the domain's first node, 0-based.  A residue's column is
// (node - hmm0) plus the inserts in front of it; an insert follows the last match state in front of it.  Every lane of the
// wavefront calls it (ballots and shuffles).  <ok> is cleared for a path whose nodes do not rise.
__device__ __forceinline__ DispLane display_columns(int node, bool valid, int hmm0, int lane, DispCarry &c, bool &ok) {
  const bool m = valid && node >= 0, ins = valid && node < 0;
  const unsigned long long mm = __ballot(m), im = __ballot(ins);
  const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
  const int ins_before = c.ins + __popcll(im & below);
  const unsigned long long mb = mm & below;
  const int src = mb ? 63 - __clzll((long long)mb) : 0;
  int pn = __shfl(node, src, 64);
  if (!mb) pn = c.prev;
  DispLane r;
  r.prev = pn;
  r.gap = m ? node - pn - 1 : 0;
  r.col = m ? node - hmm0 + ins_before : pn - hmm0 + 1 + ins_before;
  if (m && r.gap < 0) ok = false;
  const int last = __shfl(node, mm ? 63 - __clzll((long long)mm) : 0, 64);
  c.ins += __popcll(im);
  if (mm) c.prev = last;
  return r;
}

// the record of domain d against the arrays around it; its pair is of model h, reported, has a path and is reportable
__device__ __forceinline__ bool display_selected(const DisplayArgs &a, int64_t d, const wh_domain &r, bool &ok) {
  const int64_t p = r.pair;
  if (p < 0 || p >= a.npairs || d < a.dom_off[p] || d >= a.dom_off[p + 1]) { ok = false; return false; }
  if (p % a.H != a.h || !(a.flags[p] & WH_FLAG_REPORTED) || r.ali_i == 0) return false;
  const int64_t q = p / a.H;
  const int64_t L = a.offsets[q + 1] - a.offsets[q];
  const int64_t elen = a.env_off[d + 1] - a.env_off[d];
  if (r.env_i < 1 || r.env_j > L || r.ali_i < r.env_i || r.ali_j > r.env_j || r.ali_i > r.ali_j || elen != (int64_t)r.env_j - r.env_i + 1 ||
      r.hmm_i < 1 || r.hmm_j > a.M || r.hmm_i > r.hmm_j) { ok = false; return false; }
  return r.lnP != r.lnP || (double)r.lnP <= a.ln_rep_dom;
}

__global__ __launch_bounds__(kDispWaves * 64) void display_count_kernel(DisplayArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t d = (int64_t)blockIdx.x * kDispWaves + (threadIdx.x >> 6);
  if (d >= a.ndom) return;
  const wh_domain r = a.dom[d];
  bool ok = true;
  int len = 0;
  if (display_selected(a, d, r, ok)) {
    const int n = r.ali_j - r.ali_i + 1, hmm0 = r.hmm_i - 1;
    const int32_t *cols = a.cols + a.env_off[d] + (r.ali_i - r.env_i);
    DispCarry c = {0, hmm0 - 1};
    for (int base = 0; base < n; base += 64) {
      const bool valid = base + lane < n;
      const int node = valid ? cols[base + lane] : -1;
      if (valid && (node >= a.M || (base + lane == 0 && node != hmm0) || (base + lane == n - 1 && node != r.hmm_j - 1))) ok = false;
      (void)display_columns(node, valid, hmm0, lane, c, ok);
    }
    // (a lane that saw a bad node tells the others: the carry alone does not show it)
    ok = __ballot(!ok) == 0ull && c.prev == r.hmm_j - 1;
    len = ok ? c.prev - hmm0 + 1 + c.ins : 0;
  }
  if (lane == 0) {
    if (!ok) *a.bad = 1;
    a.len[d] = len;                 // 0: not selected
  }
}

__global__ __launch_bounds__(kDispScanThreads) void display_block_scan_kernel(DisplayArgs a) {
  __shared__ int wsel[kDispScanThreads / 64];
  __shared__ long long wlen[kDispScanThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t d = (int64_t)blockIdx.x * kDispScanThreads + tid;
  const int n = d < a.ndom ? a.len[d] : 0;
  const int sel = n > 0;
  // inclusive scan over the wavefront, then over the workgroup's wavefronts
  int ssel = sel;
  long long slen = n;
  for (int m = 1; m < 64; m <<= 1) {
    const int osel = __shfl_up(ssel, m);
    const long long olen = __shfl_up(slen, m);
    if (lane >= m) { ssel += osel; slen += olen; }
  }
  if (lane == 63) { wsel[wave] = ssel; wlen[wave] = slen; }
  __syncthreads();
  int bsel = 0;
  long long blen = 0;
  for (int w = 0; w < wave; w++) { bsel += wsel[w]; blen += wlen[w]; }
  if (d < a.ndom) { a.pos_sel[d] = bsel + ssel - sel; a.pos_len[d] = blen + slen - n; }
  if (tid == kDispScanThreads - 1) { a.blk_sel[blockIdx.x] = bsel + ssel; a.blk_len[blockIdx.x] = blen + slen; }
}

// exclusive scan of the nblk workgroup sums in place, 256 at a time with a carry; totals[0] = selected domains, totals[1] = columns
__global__ __launch_bounds__(kDispScanThreads) void display_top_scan_kernel(DisplayArgs a) {
  __shared__ long long ssel[kDispScanThreads], slen[kDispScanThreads];
  const int tid = threadIdx.x;
  long long csel = 0, clen = 0;
  for (int64_t base = 0; base < a.nblk; base += kDispScanThreads) {
    const int64_t b = base + tid;
    const long long r0 = b < a.nblk ? a.blk_sel[b] : 0, s0 = b < a.nblk ? a.blk_len[b] : 0;
    ssel[tid] = r0; slen[tid] = s0;
    __syncthreads();
    for (int m = 1; m < kDispScanThreads; m <<= 1) {
      const long long osel = tid >= m ? ssel[tid - m] : 0, olen = tid >= m ? slen[tid - m] : 0;
      __syncthreads();
      ssel[tid] += osel; slen[tid] += olen;
      __syncthreads();
    }
    if (b < a.nblk) { a.blk_sel[b] = csel + ssel[tid] - r0; a.blk_len[b] = clen + slen[tid] - s0; }
    csel += ssel[kDispScanThreads - 1]; clen += slen[kDispScanThreads - 1];
    __syncthreads();
  }
  if (tid == 0) { a.totals[0] = csel; a.totals[1] = clen; }
}

// (launched after the host has checked the totals against the sizes of the output arrays)
__global__ __launch_bounds__(kDispWaves * 64) void display_render_kernel(DisplayArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t d = (int64_t)blockIdx.x * kDispWaves + (threadIdx.x >> 6);
  if (d == 0 && lane == 0) a.disp_off[a.nsel] = a.total;
  if (d >= a.ndom) return;
  const int len = a.len[d];
  if (len <= 0) return;
  const int64_t blk = d / kDispScanThreads;
  const int64_t row = a.blk_sel[blk] + a.pos_sel[d];
  const int64_t at = a.blk_len[blk] + a.pos_len[d];
  if (row < 0 || row >= a.nsel || at < 0 || at + len > a.total) return;      // (the totals are the sums of these: never)
  const wh_domain r = a.dom[d];
  const int64_t q = r.pair / a.H;
  if (lane == 0) {
    a.disp_off[row] = at;
    wh_display_rec rec;
    rec.query = (int32_t)q; rec.index = r.index;
    a.recs[row] = rec;
  }
  const int n = r.ali_j - r.ali_i + 1, hmm0 = r.hmm_i - 1;
  const int64_t env = a.env_off[d] + (r.ali_i - r.env_i);
  const int32_t *cols = a.cols + env;
  const float *pp = a.pp + env;
  const uint8_t *res = a.residues + a.offsets[q] + (r.ali_i - 1);
  uint8_t *o_model = a.model + at, *o_match = a.match + at, *o_target = a.target + at, *o_pp = a.ppline + at;
  DispCarry c = {0, hmm0 - 1};
  bool ok = true;
  for (int base = 0; base < n; base += 64) {
    const bool valid = base + lane < n;
    const int node = valid ? cols[base + lane] : -1;
    const DispLane p = display_columns(node, valid, hmm0, lane, c, ok);
    if (valid && p.col >= 0 && p.col < len) {
      const int x = res[base + lane];
      const uint8_t sym = x < a.Kp ? a.tab_sym[x] : (uint8_t)'?';
      uint8_t mo = '.', ma = ' ', ta = (uint8_t)(sym >= 'A' && sym <= 'Z' ? sym + 32 : sym);
      if (node >= 0) {
        const int k = node + 1;
        mo = a.tab_cons[k];
        ta = sym;
        if (x < a.Kp) ma = x == a.tab_code[k] ? mo : a.tab_odds[(size_t)k * a.Kp + x] > 1.0f ? (uint8_t)'+' : (uint8_t)' ';
      }
      o_model[p.col] = mo; o_match[p.col] = ma; o_target[p.col] = ta; o_pp[p.col] = display_pp_char(pp[base + lane]);
    }
    // the delete states in front of the trip's match states: the lanes of the wavefront fill one run after the other
    unsigned long long gm = __ballot(valid && node >= 0 && p.gap > 0);
    while (gm) {
      const int src = __ffsll((long long)gm) - 1;
      gm &= gm - 1;
      const int g = __shfl(p.gap, src, 64), col = __shfl(p.col, src, 64), pn = __shfl(p.prev, src, 64);
      for (int t = lane; t < g; t += 64) {
        const int cc = col - g + t, k = pn + 2 + t;            // node pn + 1 + t, 1-based
        if (cc >= 0 && cc < len && k >= 1 && k <= a.M) { o_model[cc] = a.tab_cons[k]; o_match[cc] = ' '; o_target[cc] = '-'; o_pp[cc] = '.'; }
      }
    }
  }
}

static unsigned disp_blocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

int64_t display_scan_blocks(int64_t ndom) { return (ndom + kDispScanThreads - 1) / kDispScanThreads; }
hipError_t launch_display_count(const DisplayArgs &a, hipStream_t s) {
  if (a.ndom > 0) hipLaunchKernelGGL(display_count_kernel, dim3(disp_blocks(a.ndom, kDispWaves)), dim3(kDispWaves * 64), 0, s, a);
  return hipGetLastError();
}
// the two levels of the scan; a.nblk = display_scan_blocks(a.ndom)
hipError_t launch_display_scan(const DisplayArgs &a, hipStream_t s) {
  if (a.ndom > 0) hipLaunchKernelGGL(display_block_scan_kernel, dim3((unsigned)a.nblk), dim3(kDispScanThreads), 0, s, a);
  hipLaunchKernelGGL(display_top_scan_kernel, dim3(1), dim3(kDispScanThreads), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_display_render(const DisplayArgs &a, hipStream_t s) {
  if (a.ndom > 0) hipLaunchKernelGGL(display_render_kernel, dim3(disp_blocks(a.ndom, kDispWaves)), dim3(kDispWaves * 64), 0, s, a);
  return hipGetLastError();
}

}  // namespace wh
