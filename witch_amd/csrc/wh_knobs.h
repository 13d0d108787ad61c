// Development knobs: the struct, and ONE table of their names that both ways of setting them go
// through - wh_ehmm_load reads the flagged ones from the environment ONCE, wh_set_option changes any of them on a live
// handle (tools/ab_score.py).  None is needed in production.  No HIP here: tools/knobs_check.cpp runs it under the sanitizers.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>

struct Knobs {
  int kernel = 7;            // 7 phase-call scoring kernel (one query per wavefront); 8 its second compilation (A/B slot);
                             // 9 two queries per wavefront where a batch fits (wh_score9.hip; measured slower, kept for A/B: DESIGN.md);
                             // 10 staged launches (wh_staged.hip) for the size classes and batches they serve, 7 for the rest
  float keep_scale = 0.f;    // Forward-row spill threshold relative to E(row); 0 = the kernel's default
  int spill_band = 1;        // 0: envelope Forward rows stored at every lane block that passes keep_scale (A/B; the two-query kernel has no band)
  int max_waves = 0;         // cap on waves per workgroup (0 = planner's choice)
  bool force_specg = false;  // force the HBM special-state mode
  bool no_logspace = false;  // skip the log-space alignment pass
  bool no_wide_align = false; // models beyond 3 072 nodes are aligned by the float64 kernel only (A/B and debugging)
  bool no_window = false;    // envelope Backward sweeps run full width (no node window; A/B and debugging)
  bool no_p2win = false;     // the multihit Backward sweep runs full width only (A/B and debugging)
  bool no_long_list = false; // WH_NO_LONG_LIST: pairs with more than WH_MAX_ENVELOPES regions keep WH_FLAG_TRUNC (no second pass; tests)
  bool no_big_region = false; // WH_NO_BIG_REGION: a region with more domains, segments or clusters than the resolver's lists hold keeps WH_FLAG_TRUNC (no big-region pass; tests)
  bool no_long_query = false; // WH_NO_LONG_QUERY: a call whose longest query exceeds the resolver's LDS cap runs without the resolver, as before the long-query pass (tests)
  bool no_resolve = false;   // multidomain regions stay ONE envelope (round-1 behaviour) instead of HMMER's stochastic resolver
  int score_lmain = 0;       // WH_SCORE_LMAIN=<n>: the main length cap of scoring and alignment calls is at most n (tests: reaches the long-query scoring and alignment passes with short queries)
  bool no_long_score = false; // WH_NO_LONG_SCORE: no long-query scoring / alignment pass - a call with a query beyond a class's LDS plan is refused (WH_ERANGE), as before the pass
  bool longq_force = false;  // WH_LONGQ_FORCE: the passes run the float64 kernels' residues-in-HBM instantiations whatever the length (tests)
  int rqueue_cap = 0;        // test hook: size the resolver's queue for this many pairs instead of the estimate (forces the overflow re-run)
  int item_g = 0;            // queries per wave in a work item of the phase-call kernels (0 = 32; A/B)
  int st_units = 0;          // staged launches: envelope units (Forward slabs) per batch (0 = sized from the free HBM)
  bool stats = false, trace = false;
  int dbg = 0;
  int rdbg = 0;              // resolver: print the first <n> sampled segments and the cluster statistics of every region
};

// One knob: its name, whether wh_ehmm_load reads it from the environment (all but WH_SPILL_BAND, which only wh_set_option
// sets), and how a value is applied.  <v> is never null; "" restores the default.  false: the value is out of range.
struct KnobEntry {
  const char *name;
  bool from_env;
  bool (*apply)(Knobs &k, const char *v);
};
// a switch is on when its value is non-empty and not "0"; a number is clamped to lo..hi, "" gives its default
#define WH_KNOB_BOOL(name, field) {name, true, [](Knobs &k, const char *v) { k.field = *v && strcmp(v, "0") != 0; return true; }}
#define WH_KNOB_INT(name, from_env, field, lo, hi, dflt) \
  {name, from_env, [](Knobs &k, const char *v) { k.field = *v ? std::max(lo, std::min(hi, atoi(v))) : dflt; return true; }}
static const KnobEntry kKnobs[] = {
  {"WH_SCORE_KERNEL", true, [](Knobs &k, const char *v) { const int kv = *v ? atoi(v) : 7; if (kv < 7 || kv > 12) return false; k.kernel = kv; return true; }},
  {"WH_KEEP_LOG2", true, [](Knobs &k, const char *v) { k.keep_scale = *v ? ldexpf(1.0f, atoi(v)) : 0.f; return true; }},
  WH_KNOB_INT("WH_SPILL_BAND", false, spill_band, INT_MIN, INT_MAX, 1),
  WH_KNOB_INT("WH_MAX_WAVES", true, max_waves, 1, 16, 0),
  WH_KNOB_BOOL("WH_FORCE_SPECG", force_specg),
  WH_KNOB_BOOL("WH_NO_LOGSPACE", no_logspace),
  WH_KNOB_BOOL("WH_NO_RESOLVE", no_resolve),
  WH_KNOB_BOOL("WH_NO_LONG_LIST", no_long_list),
  WH_KNOB_BOOL("WH_NO_BIG_REGION", no_big_region),
  WH_KNOB_BOOL("WH_NO_LONG_QUERY", no_long_query),
  WH_KNOB_INT("WH_SCORE_LMAIN", true, score_lmain, 0, INT_MAX, 0),
  WH_KNOB_BOOL("WH_NO_LONG_SCORE", no_long_score),
  WH_KNOB_BOOL("WH_LONGQ_FORCE", longq_force),
  WH_KNOB_BOOL("WH_NO_WINDOW", no_window),
  WH_KNOB_BOOL("WH_NO_P2WIN", no_p2win),
  WH_KNOB_INT("WH_RQUEUE_CAP", true, rqueue_cap, 1, INT_MAX, 0),
  WH_KNOB_INT("WH_ITEM_G", true, item_g, 1, 1024, 0),
  WH_KNOB_INT("WH_ST_UNITS", true, st_units, 16, INT_MAX, 0),
  WH_KNOB_BOOL("WH_NO_WIDE_ALIGN", no_wide_align),
  WH_KNOB_BOOL("WH_STATS", stats),
  WH_KNOB_BOOL("WH_TRACE", trace),
  WH_KNOB_INT("WH_DBG", true, dbg, INT_MIN, INT_MAX, 0),
  WH_KNOB_INT("WH_RDBG", true, rdbg, INT_MIN, INT_MAX, 0),
};
#undef WH_KNOB_BOOL
#undef WH_KNOB_INT

// sets knob <name> of <k> to <value> (null: as ""): 1 done, 0 no knob of that name, -1 the value is out of the knob's range
static inline int set_knob(Knobs &k, const char *name, const char *value) {
  for (const KnobEntry &kn : kKnobs)
    if (!strcmp(name, kn.name)) return kn.apply(k, value ? value : "") ? 1 : -1;
  return 0;
}
