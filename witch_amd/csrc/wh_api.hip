// C ABI of libwitch_hip.so (declared in include/witch_hip.h): handle management, options, getters of the last call's
// figures, the host-pointer entry points, top-k, consensus and the final merge.  wh_score_dev is in wh_host_score.hip
// (its resolver stage in wh_host_resolve.hip), wh_align_dev in wh_host_align.hip, the per-domain results (wh_domains*,
// wh_ehmm_evparams) in wh_host_domains.hip; what they share is in wh_host.h.
#include <atomic>
#include <chrono>
#include <memory>
#include <thread>

#include "wh_host.h"

static int g_device = -1;

extern "C" {

const char *wh_version(void) { return "witch_hip 0.1.0 (gfx950)"; }
const char *wh_last_error(void) { return wh::last_error(); }

int wh_init(int device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    set_error("no HIP device visible");
    return WH_ENODEV;
  }
  if (device < 0 || device >= n) {
    set_error("device %d out of range (0..%d)", device, n - 1);
    return WH_EINVAL;
  }
  HIPCHK(hipSetDevice(device));
  (void)hipFree(nullptr);        // creates the device context now (otherwise the first hipMalloc of wh_ehmm_load pays for it)
  {                              // ... and the host-to-device copy path (its first use costs ~0.1 s)
    void *tmp = nullptr;
    int word = 0;
    if (hipMalloc(&tmp, 256) == hipSuccess) { (void)hipMemcpy(tmp, &word, sizeof word, hipMemcpyHostToDevice); (void)hipFree(tmp); }
  }
  g_device = device;
  return WH_OK;
}

int wh_device_info(char *name, int name_len, int *cu_count, int64_t *hbm_bytes) {
  if (g_device < 0) { int rc = wh_init(0); if (rc) return rc; }
  hipDeviceProp_t p;
  HIPCHK(hipGetDeviceProperties(&p, g_device));
  if (name && name_len > 0) { strncpy(name, p.gcnArchName, (size_t)name_len - 1); name[name_len - 1] = 0; }
  if (cu_count) *cu_count = p.multiProcessorCount;
  if (hbm_bytes) *hbm_bytes = (int64_t)p.totalGlobalMem;
  return WH_OK;
}

int wh_digitize(int alphabet, const char *text, int64_t n, uint8_t *out) {
  int K, Kp;
  if (alphabet_sizes(alphabet, &K, &Kp) != 0 || !text || !out) { set_error("wh_digitize: bad argument"); return WH_EINVAL; }
  return digitize(alphabet, text, n, out);
}

void wh_ehmm_free(wh_ehmm *e) {
  if (!e) return;            // (a handle whose load failed half-way included: its buffers and the filter state free themselves)
  for (hipEvent_t ev : e->cls_ev) (void)hipEventDestroy(ev);
  for (auto &t : e->timers) {
    if (t.e0) (void)hipEventDestroy(t.e0);
    if (t.e1) (void)hipEventDestroy(t.e1);
  }
  delete e;
}

static void knobs_from_env(wh_ehmm *e);

wh_ehmm *wh_ehmm_load(const char *const *hmm_paths, const int32_t *hmm_index, const int32_t *nseq, int n) {
  if (!hmm_paths || n <= 0) { set_error("wh_ehmm_load: no models"); return nullptr; }
  if (g_device < 0 && wh_init(0) != WH_OK) return nullptr;
  std::unique_ptr<wh_ehmm, void (*)(wh_ehmm *)> e(new wh_ehmm, wh_ehmm_free);
  e->device = g_device;
  const bool trace_load = getenv("WH_TRACE") != nullptr;
  auto now_ms = []() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t_l0 = now_ms();
  e->hmms.resize((size_t)n);
  std::vector<float> tables;
  std::vector<double> gtab;
  e->dev.resize((size_t)n);
  // Parsing the text files and laying out the tables is host work per model (a few ms per 1 500-node model):
  // done on a small thread pool, then concatenated in model order so that the buffers do not depend on timing.
  struct Built { int rc = WH_OK; std::string err; int Q = -1, wideW = 0; std::vector<float> fw, bw, em, emn, wfw, wbw, wem; std::vector<double> gfw, gem, gsum; };
  // WH_FORCE_WIDE=<4|12|16|24|48>: every model that fits 8 waves of that many cells per lane ALSO gets wide tables and is scored by the
  // several-waves-per-pair kernel (tests run the golden cases through it; production: models beyond 3 072 nodes only)
  const int force_wide_q = getenv("WH_FORCE_WIDE") ? atoi(getenv("WH_FORCE_WIDE")) : 0;
  e->force_wide = force_wide_q == 4 || force_wide_q == kWideQ || force_wide_q == kWideQReg || force_wide_q == kWideQReg2 || force_wide_q == kWideQBig;
  e->force_wide_q = e->force_wide ? force_wide_q : 0;
  const bool force_wide = e->force_wide;
  // cells per lane of a model's wide tables: 12 up to 6 144 nodes, 16 up to 8 192 (transition tables in registers);
  // 24 up to 12 288 and 48 up to 24 576 (tables from L2); larger models have no wide tables (float64 kernels)
  auto wide_q_of = [force_wide, force_wide_q](int M) {
    if (force_wide) return force_wide_q;
    return M <= kWideQReg * kWave * kWideWavesMax ? kWideQReg : M <= kWideQReg2 * kWave * kWideWavesMax ? kWideQReg2
         : M <= kWideQ * kWave * kWideWavesMax ? kWideQ : kWideQBig;
  };
  std::vector<Built> built((size_t)n);
  {
    std::atomic<int> next{0};
    auto work = [&]() {
      for (;;) {
        const int i = next.fetch_add(1);
        if (i >= n) break;
        HostHMM &h = e->hmms[(size_t)i];
        Built &b = built[(size_t)i];
        if (parse_hmm_file(hmm_paths[i], h) != WH_OK) { b.rc = WH_EIO; b.err = last_error(); continue; }
        h.index = hmm_index ? hmm_index[i] : i;
        if (nseq) h.nseq = nseq[i];
        b.Q = choose_Q(h.M);
        if (b.Q <= kMaxQ) build_tables(h, b.Q, b.fw, b.bw, b.em);     // (the any-size kernels read the float64 tables only)
        if (b.Q > kMaxQ || force_wide) {
          const int wide_q = wide_q_of(h.M);
          const int ww = (h.M + kWave * wide_q - 1) / (kWave * wide_q);
          if (ww <= kWideWavesMax) { b.wideW = ww; build_tables(h, wide_q, b.wfw, b.wbw, b.wem, ww * kWave); }
        }
        // node-major float32 odds of the canonical residues: the resolver's null2-by-trace reads the K values of ONE
        // node together (one lane per sampled position), not K lane-blocked arrays
        b.emn.assign((size_t)(h.M + 1) * h.K, 0.f);
        for (int k = 1; k <= h.M; k++)
          for (int x = 0; x < h.K; x++) b.emn[(size_t)k * h.K + x] = (float)h.odds[(size_t)x * (h.M + 1) + k];
        build_tables_f64(h, b.Q, b.gfw, b.gem);
        // prefix sums over the nodes of those float32 odds, in double: the null2 vector of a sampled domain is a handful of
        // differences of these rows (one per run of match states) instead of one table row per residue (wh_resolve.hip)
        b.gsum.assign((size_t)(h.M + 1) * h.K, 0.0);
        for (int k = 1; k <= h.M; k++)
          for (int x = 0; x < h.K; x++) b.gsum[(size_t)k * h.K + x] = b.gsum[(size_t)(k - 1) * h.K + x] + (double)b.emn[(size_t)k * h.K + x];
      }
    };
    const unsigned hw = std::thread::hardware_concurrency();
    const int nthreads = std::max(1, std::min<int>(n, (int)std::min<unsigned>(16u, hw ? hw : 4u)));
    std::vector<std::thread> pool;
    for (int t = 1; t < nthreads; t++) pool.emplace_back(work);
    work();
    for (auto &t : pool) t.join();
  }
  const double t_l1 = now_ms();
  for (int i = 0; i < n; i++) {
    HostHMM &h = e->hmms[(size_t)i];
    Built &b = built[(size_t)i];
    if (b.rc != WH_OK) { set_error("%s", b.err.c_str()); return nullptr; }
    if (i == 0) { e->alphabet = h.alphabet; e->K = h.K; e->Kp = h.Kp; }
    else if ((h.alphabet == WH_ALPH_AMINO) != (e->alphabet == WH_ALPH_AMINO)) {
      set_error("%s: alphabet differs from the first model", hmm_paths[i]);
      return nullptr;
    }
    const int Q = b.Q;
    DevHMM &d = e->dev[(size_t)i];
    d.M = h.M; d.Q = Q; d.Mpad = Q * kWave; d.K = h.K; d.Kp = h.Kp; d.nseq = h.nseq; d.index = h.index; d.qclass = Q;
    d.fw_off = (int64_t)tables.size(); tables.insert(tables.end(), b.fw.begin(), b.fw.end());
    d.bw_off = (int64_t)tables.size(); tables.insert(tables.end(), b.bw.begin(), b.bw.end());
    d.em_off = (int64_t)tables.size(); tables.insert(tables.end(), b.em.begin(), b.em.end());
    tables.resize((tables.size() + 3) / 4 * 4, 0.f);          // 16-byte aligned: the node-major rows are read as float4
    d.emn_off = (int64_t)tables.size(); tables.insert(tables.end(), b.emn.begin(), b.emn.end());
    d.wideQ = 0; d.wideW = 0;
    if (b.wideW > 0) {
      tables.resize((tables.size() + 3) / 4 * 4, 0.f);
      d.wideQ = wide_q_of(h.M); d.wideW = b.wideW;
      d.wfw_off = (int64_t)tables.size(); tables.insert(tables.end(), b.wfw.begin(), b.wfw.end());
      d.wbw_off = (int64_t)tables.size(); tables.insert(tables.end(), b.wbw.begin(), b.wbw.end());
      d.wem_off = (int64_t)tables.size(); tables.insert(tables.end(), b.wem.begin(), b.wem.end());
      e->wide_by_w[d.wideQ * 16 + b.wideW].push_back(i);
    }
    d.gfw_off = (int64_t)gtab.size(); gtab.insert(gtab.end(), b.gfw.begin(), b.gfw.end());
    d.gem_off = (int64_t)gtab.size(); gtab.insert(gtab.end(), b.gem.begin(), b.gem.end());
    gtab.resize((gtab.size() + 1) & ~(size_t)1, 0.0);
    d.esum_off = (int64_t)gtab.size(); gtab.insert(gtab.end(), b.gsum.begin(), b.gsum.end());
    gtab.resize((gtab.size() + 1) & ~(size_t)1, 0.0);
    b = Built();                                              // release the per-model copies as we go
    if (Q <= kMaxQ) e->by_q[Q].push_back(i);
    else { e->generic.push_back(i); if (d.wideW == 0) e->generic_front.push_back(i); }
    e->max_Q = std::max(e->max_Q, Q);
    e->max_M = std::max(e->max_M, h.M);
  }
  degen_masks(e->alphabet, e->degen);
  knobs_from_env(e.get());
  const double t_l2 = now_ms();
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, e->device) == hipSuccess) e->cu_count = p.multiProcessorCount;
  std::vector<int32_t> ns((size_t)n), ix((size_t)n);
  for (int i = 0; i < n; i++) { ns[(size_t)i] = e->hmms[(size_t)i].nseq; ix[(size_t)i] = e->hmms[(size_t)i].index; }
  if (e->d_hmms.ensure(sizeof(DevHMM) * (size_t)n) || e->d_tables.ensure(sizeof(float) * tables.size()) ||
      e->d_nseq.ensure(sizeof(int32_t) * (size_t)n) || e->d_index.ensure(sizeof(int32_t) * (size_t)n) ||
      e->d_lists.ensure(sizeof(int32_t) * (size_t)(2 * n + 4)) || e->d_counter.ensure(kCounterInts * sizeof(int)) || e->d_gtab.ensure(sizeof(double) * gtab.size()))
    return nullptr;
  if (hipMemset(e->d_counter.p, 0, kCounterInts * sizeof(int)) != hipSuccess) { set_error("hipMemset of the counter block failed"); return nullptr; }
  const double t_l3 = now_ms();
  auto up = [&](void *dst, const void *src, size_t bytes) { return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) == hipSuccess; };
  std::vector<int32_t> lists;
  for (auto &kv : e->by_q) lists.insert(lists.end(), kv.second.begin(), kv.second.end());
  lists.insert(lists.end(), e->generic_front.begin(), e->generic_front.end());      // after the size classes
  for (auto &kv : e->wide_by_w) lists.insert(lists.end(), kv.second.begin(), kv.second.end());   // ... and the wide classes
  if (!up(e->d_hmms.p, e->dev.data(), sizeof(DevHMM) * (size_t)n) || !up(e->d_tables.p, tables.data(), sizeof(float) * tables.size()) ||
      !up(e->d_nseq.p, ns.data(), sizeof(int32_t) * (size_t)n) || !up(e->d_index.p, ix.data(), sizeof(int32_t) * (size_t)n) ||
      !up(e->d_lists.p, lists.data(), sizeof(int32_t) * lists.size()) || !up(e->d_gtab.p, gtab.data(), sizeof(double) * gtab.size())) {
    set_error("upload of the eHMM tables failed");
    return nullptr;
  }
  if (trace_load) fprintf(stderr, "[wh] eHMM load: %d models parsed + tables built in %.1f ms, concatenated in %.1f ms, device buffers allocated in %.1f ms, uploaded (%.1f MB float + %.1f MB float64) in %.1f ms\n", n,
                          t_l1 - t_l0, t_l2 - t_l1, t_l3 - t_l2, tables.size() * 4e-6, gtab.size() * 8e-6, now_ms() - t_l3);
  return e.release();
}

int wh_ehmm_count(const wh_ehmm *e) { return e ? (int)e->hmms.size() : WH_EINVAL; }
int wh_ehmm_alphabet(const wh_ehmm *e) { return e ? e->alphabet : WH_EINVAL; }

int wh_ehmm_info(const wh_ehmm *e, int32_t *M, int32_t *nseq, int32_t *hmm_index) {
  if (!e) { set_error("null handle"); return WH_EINVAL; }
  for (size_t i = 0; i < e->hmms.size(); i++) {
    if (M) M[i] = e->hmms[i].M;
    if (nseq) nseq[i] = e->hmms[i].nseq;
    if (hmm_index) hmm_index[i] = e->hmms[i].index;
  }
  return WH_OK;
}

int wh_ehmm_map(const wh_ehmm *e, int h, int32_t *map_cols) {
  if (!e || h < 0 || h >= (int)e->hmms.size() || !map_cols) { set_error("wh_ehmm_map: bad argument"); return WH_EINVAL; }
  const HostHMM &m = e->hmms[(size_t)h];
  for (int k = 1; k <= m.M; k++) map_cols[k - 1] = m.map[(size_t)k];
  return WH_OK;
}

int wh_ehmm_cksum(const wh_ehmm *e, int h, uint32_t *cksum, int32_t *present) {
  if (!e || h < 0 || h >= (int)e->hmms.size() || !cksum || !present) { set_error("wh_ehmm_cksum: bad argument"); return WH_EINVAL; }
  const HostHMM &m = e->hmms[(size_t)h];
  *cksum = m.cksum; *present = m.has_cksum ? 1 : 0;
  return WH_OK;
}

int wh_set_option(wh_ehmm *e, const char *name, const char *value) {
  if (!e || !name) { set_error("wh_set_option: bad argument"); return WH_EINVAL; }
  const int set = set_knob(e->knobs, name, value);
  if (set < 0) { set_error("%s=%s: this build has kernels 7 to 12", name, value ? value : ""); return WH_EINVAL; }      // (WH_SCORE_KERNEL: the one knob with a range)
  if (!set) { set_error("wh_set_option: unknown option %s", name); return WH_EINVAL; }
  return WH_OK;
}

static void knobs_from_env(wh_ehmm *e) {
  for (const KnobEntry &k : kKnobs)
    if (k.from_env)
      if (const char *v = getenv(k.name)) (void)wh_set_option(e, k.name, v);
}

int wh_set_timing(wh_ehmm *e, int enabled) {
  if (!e) return WH_EINVAL;
  e->timing = enabled != 0;
  return WH_OK;
}


int wh_last_align_status(wh_ehmm *e, int64_t *n_logspace, int64_t *n_unaligned, int64_t *unaligned_pairs, int64_t cap) {
  if (!e || cap < 0 || (cap > 0 && !unaligned_pairs)) { set_error("wh_last_align_status: bad argument"); return WH_EINVAL; }
  if (n_logspace) *n_logspace = e->last_align_redo;
  if (n_unaligned) *n_unaligned = (int64_t)e->last_unaligned_pairs.size();
  for (int64_t t = 0; t < cap && t < (int64_t)e->last_unaligned_pairs.size(); t++) unaligned_pairs[t] = e->last_unaligned_pairs[(size_t)t];
  return WH_OK;
}

int wh_last_align_paths(wh_ehmm *e, int64_t *paths4) {
  if (!e || !paths4) { set_error("wh_last_align_paths: bad argument"); return WH_EINVAL; }
  for (int t = 0; t < 4; t++) paths4[t] = e->last_align_paths[t];
  return WH_OK;
}

int wh_last_score_paths(wh_ehmm *e, int64_t *paths6) {
  int64_t *paths4 = paths6;
  if (!e || !paths4) { set_error("wh_last_score_paths: bad argument"); return WH_EINVAL; }
  HIPCHK(hipSetDevice(e->device));
  unsigned long long v[6] = {0, 0, 0, 0, 0, 0};
  // (the counters stay on the device until the next scoring call resets them; this copy waits for the device)
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(v, e->counter(kSlotScorePath), sizeof v, hipMemcpyDeviceToHost));
  for (int t = 0; t < 6; t++) paths4[t] = (int64_t)v[t];
  return WH_OK;
}

int wh_last_score_counters(wh_ehmm *e, int64_t *out8) {
  if (!e || !out8) { set_error("wh_last_score_counters: bad argument"); return WH_EINVAL; }
  HIPCHK(hipSetDevice(e->device));
  unsigned long long v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(v, e->counter(kSlotScorePath), sizeof v, hipMemcpyDeviceToHost));
  for (int t = 0; t < 8; t++) out8[t] = (int64_t)v[t];
  out8[7] = e->last_long_list;      // (the device's slot 7 holds the ADDRESS of the 16-bit path record, kPathRecSlot: never reported)
  return WH_OK;
}

int wh_set_path_buffer(wh_ehmm *e, uint8_t *d_paths) {
  if (!e) { set_error("wh_set_path_buffer: null handle"); return WH_EINVAL; }
  e->path_buf = d_paths;
  return WH_OK;
}

int wh_set_path_buffer16(wh_ehmm *e, uint16_t *d_paths) {
  if (!e) { set_error("wh_set_path_buffer16: null handle"); return WH_EINVAL; }
  e->path_buf16 = d_paths;
  return WH_OK;
}

int wh_last_region_overflow(wh_ehmm *e, int64_t *out4) {
  if (!e || !out4) { set_error("wh_last_region_overflow: bad argument"); return WH_EINVAL; }
  for (int t = 0; t < 4; t++) out4[t] = e->last_big[t];
  return WH_OK;
}

int wh_last_long_query_pairs(wh_ehmm *e, int64_t out[2]) {
  if (!e || !out) { set_error("wh_last_long_query_pairs: bad argument"); return WH_EINVAL; }
  out[0] = e->last_long[0]; out[1] = e->last_long[1];
  return WH_OK;
}

int wh_last_long_score_pairs(wh_ehmm *e, int64_t out[2]) {
  if (!e || !out) { set_error("wh_last_long_score_pairs: bad argument"); return WH_EINVAL; }
  out[0] = e->last_long_score[0]; out[1] = e->last_long_score[1];
  return WH_OK;
}

int wh_last_long_align_pairs(wh_ehmm *e, int64_t out[2]) {
  if (!e || !out) { set_error("wh_last_long_align_pairs: bad argument"); return WH_EINVAL; }
  out[0] = e->last_long_align[0]; out[1] = e->last_long_align[1];
  return WH_OK;
}

int wh_last_queue_reruns(wh_ehmm *e) {
  if (!e) { set_error("wh_last_queue_reruns: null handle"); return WH_EINVAL; }
  return e->last_queue_reruns;
}

int wh_last_score_launches(wh_ehmm *e, int32_t *cells_per_lane, int32_t *kind, double *ms, int cap) {
  if (!e || cap < 0) { set_error("wh_last_score_launches: bad argument"); return WH_EINVAL; }
  const int n = e->cls_n > 0 ? e->cls_n - 1 : 0;
  for (int t = 0; t < n && t < cap; t++) {
    HIPCHK(hipEventSynchronize(e->cls_ev[(size_t)t + 1]));
    float f = 0.f;
    HIPCHK(hipEventElapsedTime(&f, e->cls_ev[(size_t)t], e->cls_ev[(size_t)t + 1]));
    if (cells_per_lane) cells_per_lane[t] = e->cls_q[(size_t)t];
    if (kind) kind[t] = e->cls_kind[(size_t)t];
    if (ms) ms[t] = f;
  }
  return n;
}

int wh_last_score_shapes(wh_ehmm *e, int32_t *cells_per_lane, int32_t *waves, int32_t *p2win, int cap) {
  if (!e || cap < 0) { set_error("wh_last_score_shapes: bad argument"); return WH_EINVAL; }
  const int n = (int)e->last_shapes.size();
  for (int t = 0; t < n && t < cap; t++) {
    if (cells_per_lane) cells_per_lane[t] = e->last_shapes[(size_t)t].q;
    if (waves) waves[t] = e->last_shapes[(size_t)t].waves;
    if (p2win) p2win[t] = e->last_shapes[(size_t)t].p2win;
  }
  return n;
}

int wh_last_kernel_ms(wh_ehmm *e, int which, double *ms, int *launches) {
  if (!e || which < 0 || which >= wh_ehmm::kTimers) return WH_EINVAL;
  KernelTimer &t = e->timers[which];
  if (t.pending) {
    HIPCHK(hipEventSynchronize(t.e1));
    float f = 0.f;
    HIPCHK(hipEventElapsedTime(&f, t.e0, t.e1));
    t.ms = f;
    t.pending = false;
  }
  if (ms) *ms = t.ms;
  if (launches) *launches = t.launches;
  return WH_OK;
}

// ---------------------------------------------------------------------------------------------- final merge
int wh_merge(int device, const uint8_t *q_text, const int64_t *q_off, int64_t nq, const int32_t *codes, const int32_t *q_row,
             const uint8_t *backbone, int32_t nb, int32_t B, uint8_t **out_full, uint8_t **out_masked, int64_t *out_rows,
             int64_t *out_width) {
  return wh_merge_sharded(device, q_text, q_off, nq, codes, q_row, backbone, nb, B, nullptr, nullptr, out_full, out_masked, out_rows, out_width);
}

int wh_merge_sharded(int device, const uint8_t *q_text, const int64_t *q_off, int64_t nq, const int32_t *codes, const int32_t *q_row,
                     const uint8_t *backbone, int32_t nb, int32_t B, int32_t *widths_local, const int32_t *widths_global,
                     uint8_t **out_full, uint8_t **out_masked, int64_t *out_rows, int64_t *out_width) {
  const bool widths_only = widths_local != nullptr && out_full == nullptr;
  if (!q_off || !q_row || nq < 0 || nb < 0 || B < 1 || (nq > 0 && !codes) ||
      (!widths_only && (!backbone && nb > 0)) || (!widths_only && (!out_full || !out_masked || !out_rows || !out_width || (nq > 0 && !q_text)))) {
    set_error("wh_merge: bad argument");
    return WH_EINVAL;
  }
  if (g_device < 0 && wh_init(device) != WH_OK) return WH_EHIP;
  HIPCHK(hipSetDevice(device));
  // the merge needs no model: its device buffers live for this call only
  DevBuf m_buf[12];
  const int64_t total = nq > 0 ? q_off[nq] : 0;
  std::vector<int64_t> row_q;
  for (int64_t q = 0; q < nq; q++) {
    if (q_row[q] < -2) { set_error("wh_merge: q_row[%lld] = %d", (long long)q, q_row[q]); return WH_EINVAL; }
    if (q_row[q] >= 0) row_q.push_back(q);
  }
  for (int64_t r = 0; r < total; r++)
    if (codes[r] >= B || codes[r] < -1 - B) { set_error("wh_merge: code %d of residue %lld outside the backbone (%d columns)", codes[r], (long long)r, B); return WH_EINVAL; }
  const int64_t nrows = (int64_t)nb + (int64_t)row_q.size();
  enum { mTEXT = 0, mOFF, mCODES, mQROW, mROWQ, mBB, mW, mGAP, mK, mLAY, mFULL, mMASK };
  const size_t by[10] = {(size_t)total, sizeof(int64_t) * (size_t)(nq + 1), sizeof(int32_t) * (size_t)total, sizeof(int32_t) * (size_t)nq,
                         sizeof(int64_t) * row_q.size(), (size_t)nb * (size_t)B, sizeof(int32_t) * (size_t)(B + 1), sizeof(int32_t) * (size_t)total,
                         sizeof(int32_t) * (size_t)total, sizeof(long long) * (size_t)(2 * B + 2)};
  for (int t = 0; t < 10; t++) if (m_buf[t].ensure(by[t] + 16)) return WH_ENOMEM;
  const void *src[6] = {q_text, q_off, codes, q_row, row_q.data(), backbone};
  for (int t = 0; t < 6; t++) if (by[t] && src[t]) HIPCHK(hipMemcpy(m_buf[t].p, src[t], by[t], hipMemcpyHostToDevice));
  HIPCHK(hipMemset(m_buf[mW].p, 0, by[mW]));
  MergeArgs a;
  memset(&a, 0, sizeof a);
  a.q_text = (const uint8_t *)m_buf[mTEXT].p; a.q_off = (const int64_t *)m_buf[mOFF].p; a.codes = (const int32_t *)m_buf[mCODES].p;
  a.q_row = (const int32_t *)m_buf[mQROW].p; a.row_q = (const int64_t *)m_buf[mROWQ].p; a.nq = nq;
  a.bb = (const uint8_t *)m_buf[mBB].p; a.nb = nb; a.B = B;
  a.W = (int32_t *)m_buf[mW].p; a.res_gap = (int32_t *)m_buf[mGAP].p; a.res_k = (int32_t *)m_buf[mK].p;
  a.gap_start = (long long *)m_buf[mLAY].p; a.col_pos = a.gap_start + (B + 1); a.width = a.col_pos + B;
  hipError_t err = launch_merge_runs(a, nullptr);
  if (err != hipSuccess) { set_error("merge kernels failed to launch: %s", hipGetErrorString(err)); return WH_EHIP; }
  // sharded use (one process per GPU): the widest run per gap is a MAX over all ranks - the caller all-reduces
  // widths_local and hands the result back as widths_global; the layout is then the same on every rank
  if (widths_local) HIPCHK(hipMemcpy(widths_local, a.W, by[mW], hipMemcpyDeviceToHost));
  if (widths_only) return WH_OK;
  if (widths_global) {
    for (int g = 0; g <= B; g++) if (widths_global[g] < 0) { set_error("wh_merge: negative width at gap %d", g); return WH_EINVAL; }
    HIPCHK(hipMemcpy(a.W, widths_global, by[mW], hipMemcpyHostToDevice));
    err = launch_merge_layout(a, nullptr);
    if (err != hipSuccess) { set_error("merge layout kernel failed to launch: %s", hipGetErrorString(err)); return WH_EHIP; }
  }
  long long width = 0;
  HIPCHK(hipMemcpy(&width, a.width, sizeof width, hipMemcpyDeviceToHost));
  if (width < B || (double)width * (double)nrows > 6.0e10) { set_error("wh_merge: %lld rows x %lld columns is not a plausible alignment", (long long)nrows, width); return WH_ERANGE; }
  if (m_buf[mFULL].ensure((size_t)nrows * (size_t)width + 16) || m_buf[mMASK].ensure((size_t)nrows * (size_t)B + 16)) return WH_ENOMEM;
  a.out_full = (uint8_t *)m_buf[mFULL].p; a.out_masked = (uint8_t *)m_buf[mMASK].p;
  err = launch_merge_render(a, nrows, nullptr);
  if (err != hipSuccess) { set_error("merge render kernel failed to launch: %s", hipGetErrorString(err)); return WH_EHIP; }
  uint8_t *hf = (uint8_t *)malloc((size_t)nrows * (size_t)width + 1), *hm = (uint8_t *)malloc((size_t)nrows * (size_t)B + 1);
  if (!hf || !hm) { free(hf); free(hm); set_error("wh_merge: out of host memory"); return WH_ENOMEM; }
  hipError_t c1 = hipMemcpy(hf, a.out_full, (size_t)nrows * (size_t)width, hipMemcpyDeviceToHost);
  hipError_t c2 = hipMemcpy(hm, a.out_masked, (size_t)nrows * (size_t)B, hipMemcpyDeviceToHost);
  if (c1 != hipSuccess || c2 != hipSuccess) { free(hf); free(hm); set_error("wh_merge: copying the alignment back failed: %s", hipGetErrorString(c1 != hipSuccess ? c1 : c2)); return WH_EHIP; }
  *out_full = hf; *out_masked = hm; *out_rows = nrows; *out_width = width;
  return WH_OK;
}

int wh_score(wh_ehmm *e, const uint8_t *residues, const int64_t *offsets, int64_t nq, int32_t *decibits,
             uint8_t *flags, float *fwd_bits, wh_pair_detail *detail) {
  if (!e || !residues || !offsets || !decibits || !flags || nq < 0) { set_error("wh_score: bad argument"); return WH_EINVAL; }
  if (nq == 0) return WH_OK;
  HIPCHK(hipSetDevice(e->device));
  const int64_t total = offsets[nq];
  if (check_residues(e->Kp, residues, total)) return WH_EINVAL;
  const size_t np = (size_t)nq * e->hmms.size();
  Staging st(e);
  const uint8_t *d_res = st.in(residues, (size_t)total, 16);
  const int64_t *d_off = st.in(offsets, sizeof(int64_t) * (size_t)(nq + 1));
  int32_t *d_deci = st.out(decibits, sizeof(int32_t) * np);
  uint8_t *d_flags = st.out(flags, np);
  float *d_fwd = st.out(fwd_bits, sizeof(float) * np);
  wh_pair_detail *d_det = st.out(detail, sizeof(wh_pair_detail) * np);
  if (st.rc) return st.rc;
  return st.finish(wh_score_dev(e, d_res, d_off, nq, total, max_query_len(offsets, nq), d_deci, d_flags, d_fwd, d_det, nullptr));
}

// ------------------------------------------------------------------------------------ top-k
int wh_topk_dev(wh_ehmm *e, const int32_t *d_decibits, const uint8_t *d_flags, int64_t nq, int k, int32_t *d_idx,
                double *d_w, int32_t *d_n_kept, int32_t *d_n_used, void *stream) {
  if (!e || !d_decibits || !d_flags || !d_idx || !d_w || !d_n_kept || !d_n_used || k <= 0 || nq < 0) {
    set_error("wh_topk_dev: bad argument");
    return WH_EINVAL;
  }
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipSetDevice(e->device));
  if (timer_begin(e, 1, s)) return WH_EHIP;
  TopkArgs a;
  a.decibits = d_decibits; a.flags = d_flags; a.nseq = (const int32_t *)e->d_nseq.p;
  a.hmm_index = (const int32_t *)e->d_index.p; a.nq = nq; a.H = (int)e->hmms.size(); a.k = k;
  a.idx = d_idx; a.w = d_w; a.n_kept = d_n_kept; a.n_used = d_n_used;
  hipError_t err = launch_topk(a, s);
  if (err != hipSuccess) { set_error("topk kernel launch failed: %s", hipGetErrorString(err)); return WH_EHIP; }
  if (timer_end(e, 1, s, 1)) return WH_EHIP;
  return WH_OK;
}

int wh_topk(wh_ehmm *e, const int32_t *decibits, const uint8_t *flags, int64_t nq, int k, int32_t *idx, double *w,
            int32_t *n_kept, int32_t *n_used) {
  if (!e || !decibits || !flags || !idx || !w || !n_kept || !n_used || k <= 0 || nq < 0) { set_error("wh_topk: bad argument"); return WH_EINVAL; }
  if (nq == 0) return WH_OK;
  HIPCHK(hipSetDevice(e->device));
  const size_t np = (size_t)nq * e->hmms.size(), nk = (size_t)nq * (size_t)k;
  Staging st(e);
  const int32_t *d_deci = st.in(decibits, sizeof(int32_t) * np);
  const uint8_t *d_flags = st.in(flags, np);
  int32_t *d_idx = st.out(idx, sizeof(int32_t) * nk);
  double *d_w = st.out(w, sizeof(double) * nk);
  int32_t *d_nk = st.out(n_kept, sizeof(int32_t) * (size_t)nq);
  int32_t *d_nu = st.out(n_used, sizeof(int32_t) * (size_t)nq);
  if (st.rc) return st.rc;
  return st.finish(wh_topk_dev(e, d_deci, d_flags, nq, k, d_idx, d_w, d_nk, d_nu, nullptr));
}

int wh_align(wh_ehmm *e, const uint8_t *residues, const int64_t *offsets, int64_t nq, const int64_t *pair_q,
             const int32_t *pair_h, int64_t npairs, const int64_t *col_offsets, int32_t *cols) {
  return wh_align_pp(e, residues, offsets, nq, pair_q, pair_h, npairs, col_offsets, cols, nullptr);
}

static int align_host(wh_ehmm *e, const uint8_t *residues, const int64_t *offsets, int64_t nq, const int64_t *pair_q,
                      const int32_t *pair_h, int64_t npairs, const int64_t *col_offsets, int32_t *cols, void *pp, bool pp_is64, const int32_t *cfg_len = nullptr);

int wh_align_pp(wh_ehmm *e, const uint8_t *residues, const int64_t *offsets, int64_t nq, const int64_t *pair_q,
                const int32_t *pair_h, int64_t npairs, const int64_t *col_offsets, int32_t *cols, float *pp) {
  return align_host(e, residues, offsets, nq, pair_q, pair_h, npairs, col_offsets, cols, pp, false);
}

int wh_align_pp_len(wh_ehmm *e, const uint8_t *residues, const int64_t *offsets, int64_t nq, const int64_t *pair_q,
                    const int32_t *pair_h, int64_t npairs, const int64_t *col_offsets, int32_t *cols, float *pp, const int32_t *cfg_len) {
  // (checked before anything else: the refusal needs neither a handle nor a device)
  for (int64_t q = 0; cfg_len && q < nq; q++)
    if (cfg_len[q] < 1) { set_error("wh_align_pp_len: cfg_len[%lld] = %d: the length model of query %lld needs a length of 1 or more", (long long)q, cfg_len[q], (long long)q); return WH_EINVAL; }
  return align_host(e, residues, offsets, nq, pair_q, pair_h, npairs, col_offsets, cols, pp, false, cfg_len);
}

int wh_align_pp64(wh_ehmm *e, const uint8_t *residues, const int64_t *offsets, int64_t nq, const int64_t *pair_q,
                  const int32_t *pair_h, int64_t npairs, const int64_t *col_offsets, int32_t *cols, double *pp) {
  return align_host(e, residues, offsets, nq, pair_q, pair_h, npairs, col_offsets, cols, pp, true);
}

static int align_host(wh_ehmm *e, const uint8_t *residues, const int64_t *offsets, int64_t nq, const int64_t *pair_q,
                      const int32_t *pair_h, int64_t npairs, const int64_t *col_offsets, int32_t *cols, void *pp, bool pp_is64, const int32_t *cfg_len) {
  const size_t ppw = pp_is64 ? sizeof(double) : sizeof(float);
  if (!e || !residues || !offsets || !pair_q || !pair_h || !col_offsets || !cols || nq < 0 || npairs < 0) {
    set_error("wh_align: bad argument");
    return WH_EINVAL;
  }
  if (npairs == 0) return WH_OK;
  HIPCHK(hipSetDevice(e->device));
  const int64_t total = offsets[nq];
  if (check_residues(e->Kp, residues, total)) return WH_EINVAL;
  for (int64_t p = 0; p < npairs; p++)
    if (pair_q[p] < 0 || pair_q[p] >= nq) { set_error("pair %lld: query %lld out of range", (long long)p, (long long)pair_q[p]); return WH_EINVAL; }
  const int64_t ncols = col_offsets[npairs];
  const int max_len = max_query_len(offsets, nq);
  Staging st(e);
  const uint8_t *d_res = st.in(residues, (size_t)total, 16);
  const int64_t *d_off = st.in(offsets, sizeof(int64_t) * (size_t)(nq + 1));
  const int64_t *d_pq = st.in(pair_q, sizeof(int64_t) * (size_t)npairs);
  const int32_t *d_ph = st.in(pair_h, sizeof(int32_t) * (size_t)npairs);
  const int64_t *d_co = st.in(col_offsets, sizeof(int64_t) * (size_t)(npairs + 1));
  int32_t *d_cols = st.out(cols, sizeof(int32_t) * (size_t)ncols, 16);
  void *d_pp = st.inout(pp, ppw * (size_t)ncols, 16);      // what lies between the pairs' ranges comes back as given
  const int32_t *d_cfg = st.in(cfg_len, sizeof(int32_t) * (size_t)nq);
  if (st.rc) return st.rc;
  if (cfg_len) return st.finish(wh_align_pp_len_dev(e, d_res, d_off, nq, total, max_len, d_pq, d_ph, npairs, d_co, d_cols, (float *)d_pp, d_cfg, nullptr));
  return st.finish(pp_is64 && pp ? wh_align_pp64_dev(e, d_res, d_off, nq, total, max_len, d_pq, d_ph, npairs, d_co, d_cols, (double *)d_pp, nullptr)
                                 : wh_align_pp_dev(e, d_res, d_off, nq, total, max_len, d_pq, d_ph, npairs, d_co, d_cols, (float *)d_pp, nullptr));
}

// ------------------------------------------------------------------------------------ consensus
static const int kConsKmax = 4096;   // sanity bound only: the per-residue edge lists live in HBM scratch sized by the call's own k

int wh_consensus_dev(wh_ehmm *e, const int64_t *d_offsets, int64_t nq, int32_t max_len, const int64_t *d_qpair_off,
                     const int32_t *d_pair_h, const double *d_pair_w, const int64_t *d_col_offsets,
                     const int32_t *d_cols, const int64_t *d_ret_off, const int32_t *d_retained,
                     const int32_t *d_nongaps, int32_t backbone_length, int32_t max_pairs_per_query,
                     int32_t *d_out, int32_t *d_minmax, void *stream) {
  if (!e || !d_offsets || !d_qpair_off || !d_pair_h || !d_pair_w || !d_col_offsets || !d_cols || !d_ret_off ||
      !d_retained || !d_nongaps || !d_out || !d_minmax || nq < 0 || backbone_length <= 0 || max_len < 0) {
    set_error("wh_consensus_dev: bad argument");
    return WH_EINVAL;
  }
  if (max_pairs_per_query > kConsKmax || max_pairs_per_query < 0) { set_error("more than %d HMMs per query are not supported by the consensus kernel", kConsKmax); return WH_ERANGE; }
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipSetDevice(e->device));
  if (timer_begin(e, 3, s)) return WH_EHIP;
  if (nq > 0) {
    ConsArgs a;
    memset(&a, 0, sizeof a);
    a.offsets = d_offsets; a.nq = nq; a.qpair_off = d_qpair_off; a.pair_h = d_pair_h; a.pair_w = d_pair_w;
    a.col_offsets = d_col_offsets; a.cols = d_cols; a.ret_off = d_ret_off; a.retained = d_retained; a.nongaps = d_nongaps;
    a.backbone_length = backbone_length; a.out = d_out; a.minmax = d_minmax;
    // a residue collects at most one edge per kept HMM (the reference takes any -k, weighting.py:71-73)
    a.Lcap = std::max(max_len, 1); a.Wcap = backbone_length + 1; a.KMAX = std::max(4, (int)max_pairs_per_query);
    int waves = 4;
    while (waves >= 1 && (size_t)waves * (a.Wcap + 2) * sizeof(double) > kLdsBudget) waves--;
    const bool row_in_hbm = waves < 1;        // backbones beyond ~19 000 columns: the DP row moves to the wave's HBM region
    if (row_in_hbm) waves = 4;
    const size_t lds = row_in_hbm ? 0 : (size_t)waves * (a.Wcap + 2) * sizeof(double);
    int blocks = (int)std::min<int64_t>((nq + waves - 1) / waves, (int64_t)e->cu_count * 2);
    blocks = clamp_blocks(blocks, (size_t)waves * ((size_t)(a.Lcap + 1) * (a.Wcap + 2) + (size_t)a.Lcap * a.KMAX * 12 + (size_t)a.Lcap * 4 + (size_t)(a.Wcap + 2) * 8), e->d_back, backbone_length, a.Lcap, "consensus", true);
    if (blocks < 0) return WH_ENOMEM;
    const size_t nw = (size_t)blocks * waves;
    if (row_in_hbm) {
      if (e->d_crow.ensure(nw * (size_t)(a.Wcap + 2) * sizeof(double))) return WH_ENOMEM;
      a.rowg = (double *)e->d_crow.p;
    }
    if (e->d_back.ensure(nw * (size_t)(a.Lcap + 1) * (a.Wcap + 2)) || e->d_cwj.ensure(nw * (size_t)a.Lcap * a.KMAX * sizeof(int32_t)) ||
        e->d_cwv.ensure(nw * (size_t)a.Lcap * a.KMAX * sizeof(double)) || e->d_cwn.ensure(nw * (size_t)a.Lcap * sizeof(int32_t)))
      return WH_ENOMEM;
    a.back = (uint8_t *)e->d_back.p; a.cwj = (int32_t *)e->d_cwj.p; a.cwv = (double *)e->d_cwv.p; a.cwn = (int32_t *)e->d_cwn.p;
    a.counter = e->counter(kSlotConsensus);
    HIPCHK(hipMemsetAsync(a.counter, 0, sizeof(int), s));
    hipError_t err = launch_consensus(a, blocks, waves * kWave, lds, s);
    if (err != hipSuccess) { set_error("consensus kernel launch failed: %s", hipGetErrorString(err)); return WH_EHIP; }
  }
  if (timer_end(e, 3, s, nq > 0 ? 1 : 0)) return WH_EHIP;
  return WH_OK;
}

int wh_consensus(wh_ehmm *e, const int64_t *offsets, int64_t nq, const int64_t *qpair_off, const int32_t *pair_h,
                 const double *pair_w, const int64_t *col_offsets, const int32_t *cols, const int64_t *ret_off,
                 const int32_t *retained, const int32_t *nongaps, int32_t backbone_length, int32_t *out, int32_t *minmax) {
  if (!e || !offsets || !qpair_off || !pair_h || !pair_w || !col_offsets || !cols || !ret_off || !retained || !nongaps ||
      !out || !minmax || nq < 0) {
    set_error("wh_consensus: bad argument");
    return WH_EINVAL;
  }
  if (nq == 0) return WH_OK;
  HIPCHK(hipSetDevice(e->device));
  const int H = (int)e->hmms.size();
  const int64_t npairs = qpair_off[nq], ncols = col_offsets[npairs], nret = ret_off[H], total = offsets[nq];
  int maxpp = 0;
  for (int64_t q = 0; q < nq; q++) maxpp = std::max<int>(maxpp, (int)(qpair_off[q + 1] - qpair_off[q]));
  for (int64_t p = 0; p < npairs; p++)
    if (pair_h[p] < 0 || pair_h[p] >= H) { set_error("pair %lld: model position out of range", (long long)p); return WH_EINVAL; }
  for (int h = 0; h < H; h++)
    if (ret_off[h + 1] - ret_off[h] != e->hmms[(size_t)h].M) {
      set_error("model %d: %lld retained columns but %d match states", h, (long long)(ret_off[h + 1] - ret_off[h]), e->hmms[(size_t)h].M);
      return WH_EINVAL;
    }
  for (int64_t t = 0; t < nret; t++)
    if (retained[t] < 0 || retained[t] >= backbone_length) { set_error("retained column %d outside the backbone", retained[t]); return WH_EINVAL; }
  Staging st(e);
  const int64_t *d_off = st.in(offsets, sizeof(int64_t) * (size_t)(nq + 1), 16);
  const int64_t *d_qpo = st.in(qpair_off, sizeof(int64_t) * (size_t)(nq + 1), 16);
  const int32_t *d_ph = st.in(pair_h, sizeof(int32_t) * (size_t)npairs, 16);
  const double *d_pw = st.in(pair_w, sizeof(double) * (size_t)npairs, 16);
  const int64_t *d_co = st.in(col_offsets, sizeof(int64_t) * (size_t)(npairs + 1), 16);
  const int32_t *d_cols = st.in(cols, sizeof(int32_t) * (size_t)ncols, 16);
  const int64_t *d_ro = st.in(ret_off, sizeof(int64_t) * (size_t)(H + 1), 16);
  const int32_t *d_ret = st.in(retained, sizeof(int32_t) * (size_t)nret, 16);
  const int32_t *d_ng = st.in(nongaps, sizeof(int32_t) * (size_t)nret, 16);
  int32_t *d_out = st.out(out, sizeof(int32_t) * (size_t)total, 16);
  int32_t *d_mm = st.out(minmax, sizeof(int32_t) * (size_t)(2 * nq), 16);
  if (st.rc) return st.rc;
  return st.finish(wh_consensus_dev(e, d_off, nq, max_query_len(offsets, nq), d_qpo, d_ph, d_pw, d_co, d_cols, d_ro, d_ret, d_ng, backbone_length, maxpp,
                                    d_out, d_mm, nullptr));
}

// The length up to which queries stay on the float32 kernels, from the planner's own functions (wh_plan.h): the largest
// length every scoring launch (one-wave classes whichever kernel family they take, the wide kernel, the float64 front end
// of the models beyond them) and every alignment class of the handle can plan.  Longer queries are served by the long-query
// passes.
int wh_ehmm_max_query_len(const wh_ehmm *e) {
  if (!e) return WH_EINVAL;
  return query_len_cap(plan_knobs(e), plan_classes(e));
}

int wh_query_len_cap(int alphabet, const int32_t *model_nodes, int n) {
  int K, Kp;
  if (alphabet_sizes(alphabet, &K, &Kp) != 0 || !model_nodes || n <= 0) { set_error("wh_query_len_cap: bad argument"); return WH_EINVAL; }
  PlanClasses cl;
  cl.K = K;
  for (int i = 0; i < n; i++) {
    if (model_nodes[i] < 1) { set_error("wh_query_len_cap: model %d has %d nodes", i, model_nodes[i]); return WH_EINVAL; }
    const int Q = choose_Q(model_nodes[i]);
    if (Q > kMaxQ) {
      // (as wh_ehmm_load: wide tables up to 8 waves of 48 cells per lane, the float64 front end beyond)
      if ((model_nodes[i] + kWave * kWideQBig - 1) / (kWave * kWideQBig) <= kWideWavesMax) cl.wide = true; else cl.front = true;
    } else if (std::find(cl.score_q.begin(), cl.score_q.end(), Q) == cl.score_q.end()) { cl.score_q.push_back(Q); cl.align_q.push_back(Q); }
  }
  return query_len_cap(PlanKnobs(), cl);
}

}  // extern "C"
