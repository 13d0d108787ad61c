// Stand-alone sanitizer run of the scalar filter pipeline (wh_filter.h: the code behind wh_filter_host): parses model
// files, digitises a FASTA file and runs every (query, model) pair through MSV -> Viterbi at HMMER's default thresholds,
// first as hmmsearch --nobias does, then with the bias filter (the two-state composition Forward and its logarithm).
// Host code only - no HIP, no Python:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tools/filter_host_sanitize.cpp witch_amd/csrc/wh_hmm.cpp -o /tmp/filter_host_sanitize
//   /tmp/filter_host_sanitize tests/golden/dna_hmmbuild/queries.fasta tests/golden/dna_hmmbuild/hmms/A_0_*.hmm
// prints the stage counts per model (tests/golden/filters and tests/golden/filters_bias hold hmmsearch's) and exits 0.
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../witch_amd/csrc/wh_filter.h"

int main(int argc, char **argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s QUERIES.fasta MODEL.hmm ...\n", argv[0]); return 2; }
  std::vector<std::string> text;
  std::ifstream fa(argv[1]);
  for (std::string line; std::getline(fa, line);) {
    if (!line.empty() && line[0] == '>') text.emplace_back();
    else if (!text.empty()) text.back() += line;
  }
  if (text.empty()) { fprintf(stderr, "%s: no sequences\n", argv[1]); return 2; }
  const whf::FilterOpts opts;
  for (int m = 2; m < argc; m++) {
    wh::HostHMM h;
    if (wh::parse_hmm_file(argv[m], h) != 0) { fprintf(stderr, "%s: cannot parse\n", argv[m]); return 1; }
    uint32_t degen[32];
    wh::degen_masks(h.alphabet, degen);
    whf::FilterModel fm;
    if (const char *missing = whf::filter_model_of(h, degen, fm)) { fprintf(stderr, "%s: no STATS LOCAL %s line\n", argv[m], missing); return 1; }
    const whf::FilterThr thr = whf::filter_thresholds(fm.evp, opts);
    std::vector<int16_t> rows((size_t)7 * ((size_t)fm.M + 1));
    for (int bias = 0; bias < 2; bias++) {
      long n[4] = {0, 0, 0, 0};
      for (const std::string &t : text) {
        std::vector<uint8_t> dsq(t.size() + 1);
        if (wh::digitize(h.alphabet, t.data(), (int64_t)t.size(), dsq.data()) != 0) { fprintf(stderr, "a query has a character outside the alphabet\n"); return 1; }
        const whf::FilterPairOut r = whf::filter_pair_host(fm, thr, dsq.data(), (int)t.size(), rows.data(), bias != 0);
        n[0]++; n[1] += (r.stage & whf::kStageMSV) != 0; n[2] += (r.stage & whf::kStageBias) != 0; n[3] += (r.stage & whf::kStageVit) != 0;
      }
      printf("%s%s: %ld targets, passed MSV %ld, bias %ld, Viterbi %ld\n", argv[m], bias ? " (bias filter)" : "", n[0], n[1], n[2], n[3]);
    }
  }
  return 0;
}
