// Stand-alone sanitizer run of the host side of hmmsearch --tblout (wh_seqtab.h: the code behind wh_seq_expect_host and
// wh_seq_table_host): parses model files, digitises a FASTA file, runs every (query, model) pair through the float64
// counting sweep (multihit Forward and Backward, posteriors, region scan, multidomain test) and assembles one row per pair
// with a region from a detail record made of the sweep's own numbers (one envelope over the whole query).
// Host code only - no HIP, no Python:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tools/seq_table_host_sanitize.cpp witch_amd/csrc/wh_hmm.cpp -o /tmp/seq_table_host_sanitize
//   /tmp/seq_table_host_sanitize tests/golden/dna_hmmbuild/queries.fasta tests/golden/dna_hmmbuild/hmms/A_0_*.hmm
// prints per model the pairs with a region, the sums of reg and clu and of exp (tests/golden/tblout holds hmmsearch's
// columns) and exits 0.
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../witch_amd/csrc/wh_seqtab.h"

int main(int argc, char **argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s QUERIES.fasta MODEL.hmm ...\n", argv[0]); return 2; }
  std::vector<std::string> text;
  std::ifstream fa(argv[1]);
  for (std::string line; std::getline(fa, line);) {
    if (!line.empty() && line[0] == '>') text.emplace_back();
    else if (!text.empty()) text.back() += line;
  }
  if (text.empty()) { fprintf(stderr, "%s: no sequences\n", argv[1]); return 2; }
  const int64_t nq = (int64_t)text.size();
  for (int m = 2; m < argc; m++) {
    wh::HostHMM h;
    if (wh::parse_hmm_file(argv[m], h) != 0) { fprintf(stderr, "%s: cannot parse\n", argv[m]); return 1; }
    wh::configure_profile(h);
    std::vector<uint8_t> flags((size_t)nq, 0);
    std::vector<wh_pair_detail> detail((size_t)nq);
    std::vector<wh_seq_expect_rec> expect;
    std::vector<int64_t> lengths((size_t)nq);
    long reg = 0, clu = 0;
    double exp_sum = 0.0;
    for (int64_t q = 0; q < nq; q++) {
      const std::string &t = text[(size_t)q];
      std::vector<uint8_t> dsq(t.size() + 1);
      if (wh::digitize(h.alphabet, t.data(), (int64_t)t.size(), dsq.data()) != 0) { fprintf(stderr, "a query has a character outside the alphabet\n"); return 1; }
      const int L = (int)t.size();
      lengths[(size_t)q] = L;
      const wh_seq_expect_rec r = whs::seq_expect_pair_host(h, dsq.data(), L);
      wh_pair_detail &d = detail[(size_t)q];
      d = wh_pair_detail();
      if (r.reg < 1) continue;
      flags[(size_t)q] = WH_FLAG_REPORTED;
      d.nregions = r.reg; d.nenv = 1; d.env_i[0] = 1; d.env_j[0] = L; d.envsc[0] = 0.5f * (float)L; d.domcorr[0] = 0.f;
      d.seq_score = 0.5f * (float)L; d.pre_score = d.seq_score + 0.25f;
      expect.push_back(r);
      reg += r.reg; clu += r.clu; exp_sum += r.exp;
    }
    const float tau = h.has_fstats ? h.ftau : __builtin_nanf(""), lambda = h.has_fstats ? h.flambda : __builtin_nanf("");
    wh_seq_table_opts o = {0, 0, 10.0, 10.0, 0.01, 0.01};
    std::vector<wh_seq_row> rows(expect.size());
    int64_t status[4];
    const int64_t n = whs::seq_table_rows_host(1, &tau, &lambda, lengths.data(), nq, flags.data(), detail.data(), expect.data(), o, rows.data(),
                                               (int64_t)rows.size(), status);
    if (n != (int64_t)expect.size() || status[2] != 0) { fprintf(stderr, "%s: %lld rows for %zu pairs, %lld reg mismatches\n", argv[m], (long long)n, expect.size(), (long long)status[2]); return 1; }
    long rep = 0, inc = 0;
    for (const wh_seq_row &r : rows) { rep += r.rep; inc += r.inc; }
    // (a capacity one short is refused, nothing is written)
    if (!rows.empty() && whs::seq_table_rows_host(1, &tau, &lambda, lengths.data(), nq, flags.data(), detail.data(), expect.data(), o, rows.data(),
                                                  (int64_t)rows.size() - 1, status) != -1) { fprintf(stderr, "a capacity one short was accepted\n"); return 1; }
    printf("%s: %lld targets, %lld with a region, reg %ld, clu %ld, sum of exp %.3f, rep %ld, inc %ld\n", argv[m], (long long)nq, (long long)n, reg, clu, exp_sum, rep, inc);
  }
  return 0;
}
