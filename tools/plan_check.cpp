// Stand-alone check of the host planner (witch_amd/csrc/wh_plan.h), built with -fsanitize=address,undefined by
// tests/test_long_query_scoring.py and run without a GPU: for both alphabets and every one-wave size class it prints the main
// length cap of scoring and of alignment (the test reads them), and it fails when a cap is not positive, a plan at the cap
// overruns the LDS budget, a plan one residue beyond it is accepted, or a call's cap is not its longest query / the class cap.  Links libwitch_hip.so for the three LDS
// formulas that live beside their kernels.
#include <cstdio>

#include "wh_plan.h"

using namespace wh;

int main() {
  int bad = 0;
  const int Ks[2] = {4, 20};
  for (int K : Ks) {
    for (int Q = 4; Q <= kMaxQ; Q += 4) {
      PlanClasses cl;
      cl.K = K; cl.score_q = {Q}; cl.align_q = {Q};
      const PlanKnobs kn;
      const int s = largest_length([&](int L) { return score_fits(kn, cl, L, false); });
      const int a = largest_length([&](int L) { return align_fits(kn, cl, L); });
      printf("cap K=%d Q=%d score=%d align=%d\n", K, Q, s, a);
      if (s < 1 || a < 1 || s >= kMaxPlanLength || a >= kMaxPlanLength) { printf("FAIL: cap out of range\n"); bad++; continue; }
      ScoreLds sl;
      AlignLds al;
      if (!plan_score_lds(kn, K, Q, s, false, &sl) || sl.b.lds > kLdsBudget || sl.b.waves < 1 || sl.b.wave_lds * 4 < s) { printf("FAIL: scoring plan at the cap\n"); bad++; }
      if (plan_score_lds(kn, K, Q, s + 1, false, &sl)) { printf("FAIL: scoring plan beyond the cap\n"); bad++; }
      if (plan_align_lds(false, K, Q, a, &al) != 0 || al.lds > kLdsBudget || al.waves < 1 || al.wave_lds * 4 < a) { printf("FAIL: alignment plan at the cap\n"); bad++; }
      if (plan_align_lds(false, K, Q, a + 1, &al) != 1) { printf("FAIL: alignment plan beyond the cap\n"); bad++; }
      // a call's cap: its own longest query when that fits, the class cap beyond, whatever the knobs
      for (int kernel : {7, 9}) for (int mw : {0, 2}) for (int fs = 0; fs < 2; fs++) {
        PlanKnobs k2; k2.kernel = kernel; k2.max_waves = mw; k2.force_specg = fs != 0;
        const int c2 = largest_length([&](int L) { return score_fits(k2, cl, L, false); });
        for (int Lc : {1, 150, c2, c2 + 1, 4 * c2}) {
          const int m = score_main_cap(k2, cl, Lc);
          if (m != (Lc <= c2 ? Lc : c2)) { printf("FAIL: score_main_cap(K=%d Q=%d kernel=%d waves=%d specg=%d Lc=%d) = %d, class cap %d\n", K, Q, kernel, mw, fs, Lc, m, c2); bad++; }
        }
      }
      for (int Lc : {1, a, a + 1, 3 * a}) if (align_main_cap(kn, cl, Lc) != (Lc <= a ? Lc : a)) { printf("FAIL: align_main_cap\n"); bad++; }
    }
    // a handle with every class, the wide kernel and the front end: the smallest of them
    PlanClasses all;
    all.K = K; all.wide = true; all.front = true;
    for (int Q = 4; Q <= kMaxQ; Q += 4) { all.score_q.push_back(Q); all.align_q.push_back(Q); }
    const int cap = query_len_cap(PlanKnobs(), all);
    printf("cap K=%d all=%d wide_lds=%zu generic_lds=%zu\n", K, cap, wide_lds_bytes(cap, 0), generic_lds_bytes(cap));
    if (cap < 1 || wide_lds_bytes(cap, 0) > kLdsBudget || generic_lds_bytes(cap) > kLdsBudget) { printf("FAIL: cap of all classes\n"); bad++; }
  }
  printf(bad ? "plan_check: %d failure(s)\n" : "plan_check: ok\n", bad);
  return bad ? 1 : 0;
}
