// Stand-alone check of the development knobs' table (witch_amd/csrc/wh_knobs.h), built with -fsanitize=address,undefined by
// tests/test_abi_host.py and run without a GPU: for each of the 23 names the default, a set value, the reset by "", every
// clamp and range; an unknown name is refused; and the names that wh_ehmm_load reads from the environment are the 22 written
// out below (not derived from the table).
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "wh_knobs.h"

static int bad = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAIL line %d: %s\n", __LINE__, #cond); bad++; } } while (0)

static bool same(const Knobs &a, const Knobs &b) {
  return a.kernel == b.kernel && a.keep_scale == b.keep_scale && a.spill_band == b.spill_band && a.max_waves == b.max_waves && a.force_specg == b.force_specg &&
         a.no_logspace == b.no_logspace && a.no_wide_align == b.no_wide_align && a.no_window == b.no_window && a.no_p2win == b.no_p2win &&
         a.no_long_list == b.no_long_list && a.no_big_region == b.no_big_region && a.no_long_query == b.no_long_query && a.no_resolve == b.no_resolve &&
         a.score_lmain == b.score_lmain && a.no_long_score == b.no_long_score && a.longq_force == b.longq_force && a.rqueue_cap == b.rqueue_cap &&
         a.item_g == b.item_g && a.st_units == b.st_units && a.stats == b.stats && a.trace == b.trace && a.dbg == b.dbg && a.rdbg == b.rdbg;
}

// a switch: off by default, on for a non-empty value that is not "0", off again for "", "0" and a null value
static void check_bool(const char *name, bool Knobs::*field) {
  Knobs k;
  CHECK(!(k.*field));
  CHECK(set_knob(k, name, "1") == 1 && k.*field);
  CHECK(set_knob(k, name, "") == 1 && !(k.*field));
  CHECK(set_knob(k, name, "yes") == 1 && k.*field);
  CHECK(set_knob(k, name, "0") == 1 && !(k.*field));
  CHECK(set_knob(k, name, "2") == 1 && k.*field);
  CHECK(set_knob(k, name, nullptr) == 1 && !(k.*field));
  if (bad) printf("  (%s)\n", name);
}

// a number: its default, values with what they become, the default again by ""
static void check_int(const char *name, int Knobs::*field, int dflt, const std::vector<std::pair<const char *, int>> &cases) {
  Knobs k;
  CHECK(k.*field == dflt);
  for (const auto &c : cases) {
    CHECK(set_knob(k, name, c.first) == 1 && k.*field == c.second);
    if (k.*field != c.second) printf("  %s=%s gave %d, expected %d\n", name, c.first, k.*field, c.second);
    CHECK(set_knob(k, name, "") == 1 && k.*field == dflt);
  }
  CHECK(set_knob(k, name, cases[0].first) == 1 && set_knob(k, name, nullptr) == 1 && k.*field == dflt);
}

int main() {
  check_bool("WH_FORCE_SPECG", &Knobs::force_specg);
  check_bool("WH_NO_LOGSPACE", &Knobs::no_logspace);
  check_bool("WH_NO_RESOLVE", &Knobs::no_resolve);
  check_bool("WH_NO_LONG_LIST", &Knobs::no_long_list);
  check_bool("WH_NO_BIG_REGION", &Knobs::no_big_region);
  check_bool("WH_NO_LONG_QUERY", &Knobs::no_long_query);
  check_bool("WH_NO_LONG_SCORE", &Knobs::no_long_score);
  check_bool("WH_LONGQ_FORCE", &Knobs::longq_force);
  check_bool("WH_NO_WINDOW", &Knobs::no_window);
  check_bool("WH_NO_P2WIN", &Knobs::no_p2win);
  check_bool("WH_NO_WIDE_ALIGN", &Knobs::no_wide_align);
  check_bool("WH_STATS", &Knobs::stats);
  check_bool("WH_TRACE", &Knobs::trace);
  check_int("WH_SPILL_BAND", &Knobs::spill_band, 1, {{"0", 0}, {"1", 1}, {"7", 7}, {"-3", -3}});
  check_int("WH_MAX_WAVES", &Knobs::max_waves, 0, {{"4", 4}, {"1", 1}, {"16", 16}, {"0", 1}, {"-5", 1}, {"17", 16}, {"1000", 16}});
  check_int("WH_ITEM_G", &Knobs::item_g, 0, {{"8", 8}, {"1", 1}, {"1024", 1024}, {"0", 1}, {"-1", 1}, {"1025", 1024}});
  check_int("WH_ST_UNITS", &Knobs::st_units, 0, {{"100", 100}, {"16", 16}, {"15", 16}, {"0", 16}, {"-2", 16}, {"1000000", 1000000}});
  check_int("WH_RQUEUE_CAP", &Knobs::rqueue_cap, 0, {{"50", 50}, {"1", 1}, {"0", 1}, {"-7", 1}});
  check_int("WH_SCORE_LMAIN", &Knobs::score_lmain, 0, {{"300", 300}, {"0", 0}, {"-1", 0}});
  check_int("WH_DBG", &Knobs::dbg, 0, {{"3", 3}, {"-1", -1}});
  check_int("WH_RDBG", &Knobs::rdbg, 0, {{"5", 5}, {"-2", -2}});
  {   // WH_SCORE_KERNEL: 7 to 12, anything else is refused and changes nothing
    Knobs k;
    CHECK(k.kernel == 7);
    for (int v = 7; v <= 12; v++) CHECK(set_knob(k, "WH_SCORE_KERNEL", std::to_string(v).c_str()) == 1 && k.kernel == v);
    for (const char *v : {"6", "13", "0", "-7", "abc", "100"}) CHECK(set_knob(k, "WH_SCORE_KERNEL", v) == -1 && k.kernel == 12);
    CHECK(set_knob(k, "WH_SCORE_KERNEL", "") == 1 && k.kernel == 7);
    CHECK(set_knob(k, "WH_SCORE_KERNEL", "9") == 1 && set_knob(k, "WH_SCORE_KERNEL", nullptr) == 1 && k.kernel == 7);
  }
  {   // WH_KEEP_LOG2=<n>: the scale is 2^n
    Knobs k;
    CHECK(k.keep_scale == 0.f);
    CHECK(set_knob(k, "WH_KEEP_LOG2", "3") == 1 && k.keep_scale == 8.f);
    CHECK(set_knob(k, "WH_KEEP_LOG2", "-4") == 1 && k.keep_scale == 0.0625f);
    CHECK(set_knob(k, "WH_KEEP_LOG2", "0") == 1 && k.keep_scale == 1.f);
    CHECK(set_knob(k, "WH_KEEP_LOG2", "") == 1 && k.keep_scale == 0.f);
  }
  {   // a knob changes its own field only, and a name the table does not have is refused
    Knobs k, fresh;
    CHECK(set_knob(k, "WH_MAX_WAVES", "4") == 1);
    k.max_waves = 0;
    CHECK(same(k, fresh));
    for (const char *name : {"WH_NO_SUCH_KNOB", "", "WH_MAX_WAVE", "WH_MAX_WAVES ", "wh_max_waves", "WH_FORCE_WIDE", "WH_CALIB_WS_MB", "WH_WIDE_DENSE"})
      CHECK(set_knob(k, name, "1") == 0);
    CHECK(same(k, fresh));
  }
  // the table: 23 names, none twice, and the 22 read from the environment (every one but WH_SPILL_BAND)
  const std::vector<std::string> from_env = {"WH_SCORE_KERNEL", "WH_ITEM_G", "WH_ST_UNITS", "WH_KEEP_LOG2", "WH_MAX_WAVES", "WH_FORCE_SPECG", "WH_NO_LOGSPACE",
                                             "WH_NO_RESOLVE", "WH_NO_LONG_LIST", "WH_NO_BIG_REGION", "WH_NO_LONG_QUERY", "WH_SCORE_LMAIN", "WH_NO_LONG_SCORE",
                                             "WH_LONGQ_FORCE", "WH_NO_WINDOW", "WH_NO_P2WIN", "WH_RQUEUE_CAP", "WH_NO_WIDE_ALIGN", "WH_STATS", "WH_TRACE", "WH_DBG",
                                             "WH_RDBG"};
  CHECK(from_env.size() == 22);
  int n = 0, n_env = 0;
  for (const KnobEntry &a : kKnobs) {
    n++;
    int same = 0;
    for (const KnobEntry &b : kKnobs) same += !strcmp(a.name, b.name);
    CHECK(same == 1);
    bool listed = false;
    for (const std::string &s : from_env) listed = listed || s == a.name;
    CHECK(listed == a.from_env);
    if (listed != a.from_env) printf("  %s: from_env is %d\n", a.name, (int)a.from_env);
    n_env += a.from_env;
    CHECK(a.from_env == (strcmp(a.name, "WH_SPILL_BAND") != 0));
  }
  CHECK(n == 23 && n_env == 22);
  printf(bad ? "knobs_check: %d failure(s)\n" : "knobs_check: ok\n", bad);
  return bad ? 1 : 0;
}
