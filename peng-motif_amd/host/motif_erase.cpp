#include "motif_erase.h"

#include <sys/stat.h>

#include <cstdio>
#include <cstdlib>
#include <iostream>

#include "device.h"

namespace {
struct MotifLine {
  std::string id;
  int w = 0;
  int32_t thr = 0;
  unsigned long long sites = 0;
};
struct Round {
  size_t seeds = 0, windows = 0;
  unsigned long long erased_before = 0;
  std::vector<MotifLine> motifs;
};

// s / 100 with exactly two decimals, from the integer (as --sites writes its scores)
std::string score_str(int32_t s) {
  char b[24];
  const long long a = s < 0 ? -(long long)s : s;
  snprintf(b, sizeof b, "%s%lld.%02lld", s < 0 ? "-" : "", a / 100, a % 100);
  return b;
}

void dump_file(const std::string& path, const void* p, size_t bytes) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f || fwrite(p, 1, bytes, f) != bytes) {
    std::cerr << "Error: PENGK_DUMP_TABLES: cannot write " << path << std::endl;
    exit(1);
  }
  fclose(f);
}

// the redundancy filter's test (Peng::filter_redundancy) of one motif against another
bool redundant(IUPACPattern* kept, IUPACPattern* p, BackgroundModel& bg, float factor) {
  if (kept->get_pattern_length() != p->get_pattern_length()) return false;
  const int L = (int)kept->get_pattern_length();
  const float s1 = IUPACPattern::calculate_s(kept->get_pwm(), p->get_pwm(), bg.getV()[0], 0, 0, L);
  const float s2 = IUPACPattern::calculate_s(kept->get_comp_pwm(), p->get_pwm(), bg.getV()[0], 0, 0, L);
  return s1 > factor * L || s2 > factor * L;
}
}  // namespace

void run_erase_rounds(Peng& peng, PengParameters& params, std::vector<IUPACPattern*>& result, SequenceSet& set,
                      const ScanInput& in, BackgroundModel& bg, bool both_strands, double pvalue, int rounds,
                      float merge_bit_factor_threshold, const std::string& path, const uint32_t* initial_valid,
                      const ScanSubset* subset) {
  using pengk_host::check;
  using pengk_host::DeviceBuffer;
  pengk_host::Lap lap("  erase: ");
  pengk_ctx* ctx = pengk_host::context();
  const int W = (int)params.max_pattern_length;
  const int both = both_strands ? 1 : 0;
  const size_t n_local = subset ? subset->n : in.n_local;
  const int64_t* d_offs = subset ? subset->d_offs : in.d_offs.get();
  const uint32_t* d_lens = subset ? subset->d_lens : in.d_lens.get();
  const float* bg0 = bg.getV()[0];
  const char* dump_dir = pengk_host::rank() == 0 ? std::getenv("PENGK_DUMP_TABLES") : nullptr;

  std::vector<Round> report(1);
  report[0].seeds = peng.last_seeds;
  report[0].windows = peng.last_windows;
  std::vector<IUPACPattern*> prev(result);  // the motifs whose sites are masked next
  // validity words: the round reads `cur` (round 2: the input's own, or what --mask-low-complexity left of them) and writes `next`
  DeviceBuffer<uint32_t> va((size_t)in.n_words), vb((size_t)in.n_words);
  const uint32_t* cur = initial_valid ? initial_valid : in.d_valid.get();
  if (subset) {  // (the words of the sequences outside the subset are never written: zero, not whatever the buffer held)
    check(pengk_memset(ctx, va.get(), 0, (size_t)in.n_words * sizeof(uint32_t)), "pengk_memset");
    check(pengk_memset(ctx, vb.get(), 0, (size_t)in.n_words * sizeof(uint32_t)), "pengk_memset");
  }
  uint32_t* next = va.get();
  DeviceBuffer<uint64_t> d_tot;
  DeviceBuffer<uint64_t> d_words, d_items, d_seq_base(n_local), d_seq_item(n_local);
  pengk_host::PackedInput masked;
  unsigned long long erased_so_far = 0;

  for (int r = 1;; ++r) {  // r: the round whose motifs `prev` holds
    Round& rd = report[r - 1];
    if (prev.empty()) break;  // (the round ran and reported nothing: its one line says so)
    const int n_motifs = (int)prev.size();
    std::vector<int32_t> S, len, thr(n_motifs);
    motif_log_odds(prev, bg0, S, len, "erase");
    for (int m = 0; m < n_motifs; ++m) {
      int32_t lo = 0, hi = 0;
      const int32_t* Sm = &S[(size_t)m * PENGK_MAX_MOTIF_LEN * 4];
      check(pengk_score_tail_pvalues(Sm, len[m], bg0, &lo, &hi, nullptr), "pengk_score_tail_pvalues");
      std::vector<double> tail((size_t)(hi - lo) + 1);
      check(pengk_score_tail_pvalues(Sm, len[m], bg0, &lo, &hi, tail.data()), "pengk_score_tail_pvalues");
      check(pengk_score_threshold(tail.data(), lo, hi, pvalue, &thr[m]), "pengk_score_threshold");
    }
    // the mask of these motifs over what this round searched; site and erased counts summed over the ranks
    d_tot.resize((size_t)n_motifs + 1);
    check(pengk_memset(ctx, d_tot.get(), 0, ((size_t)n_motifs + 1) * sizeof(uint64_t)), "pengk_memset");
    check(pengk_mask_sites(ctx, in.d_words.get(), cur, d_offs, d_lens, n_local, n_motifs, S.data(), len.data(),
                           both, thr.data(), next, d_tot.get(), d_tot.get() + n_motifs),
          "pengk_mask_sites");
    std::vector<long long> tot((size_t)n_motifs + 1, 0);
    d_tot.download((uint64_t*)tot.data(), (size_t)n_motifs + 1);
    SequenceSet::allreduceSum(tot.data(), tot.size());
    const unsigned long long erased = (unsigned long long)tot[n_motifs];
    for (int m = 0; m < n_motifs; ++m) {
      MotifLine ml;
      ml.id = prev[m]->get_pattern_string();
      ml.w = len[m];
      ml.thr = thr[m];
      ml.sites = (unsigned long long)tot[m];
      rd.motifs.push_back(ml);
    }
    if (dump_dir) {  // test hook: what round r + 1's mask is made with (behind the last round: would have been)
      const std::string sub = std::string(dump_dir) + "/round" + std::to_string(r + 1);
      mkdir(sub.c_str(), 0777);
      dump_file(sub + "/erase_S.i32", S.data(), S.size() * sizeof(int32_t));
      dump_file(sub + "/erase_len.i32", len.data(), len.size() * sizeof(int32_t));
      dump_file(sub + "/erase_thr.i32", thr.data(), thr.size() * sizeof(int32_t));
      if (initial_valid) {  // (--mask-low-complexity: the validity words that round is searched on)
        std::vector<uint32_t> v((size_t)in.n_words);
        check(pengk_memcpy_d2h(ctx, v.data(), next, v.size() * sizeof(uint32_t)), "pengk_memcpy_d2h");
        dump_file(sub + "/erase_valid.u32", v.data(), v.size() * sizeof(uint32_t));
      }
    }
    lap("thresholds + mask");
    if (r > rounds || rd.seeds == 0 || erased == 0) break;
    erased_so_far += erased;

    // the masked set in the count layout, attached in place of the input's
    pengk_packed pk;
    check(pengk_pack_scan_sizes(ctx, next, d_offs, d_lens, n_local, W, 0, d_seq_base.get(), d_seq_item.get(), &pk),
          "pengk_pack_scan_sizes");
    d_words.resize(pk.n_words);
    d_items.resize(pk.n_items + 1);
    check(pengk_pack_scan(ctx, in.d_words.get(), next, d_offs, d_lens, n_local, W, 0, d_seq_base.get(),
                          d_seq_item.get(), d_words.get(), pk.n_words, d_items.get(), pk.n_items),
          "pengk_pack_scan");
    masked.W = W;
    masked.item_windows = pk.item_windows;
    masked.d_words = d_words.get();
    masked.d_items = d_items.get();
    masked.n_words = pk.n_words;
    masked.n_items = pk.n_items;
    masked.n_windows = pk.n_windows;
    masked.max_bin_bound = pk.max_bin_bound;
    masked.all_whole = pk.all_whole;
    pengk_host::override_packed_input(&set, &masked);
    pengk_host::set_dump_subdir("round" + std::to_string(r + 1) + "/");
    lap("pack");

    std::cout << std::endl
              << "erase round " << (r + 1) << ": " << erased << " bases under the sites of " << n_motifs << " motif"
              << (n_motifs == 1 ? "" : "s") << " masked (" << erased_so_far << " in all)" << std::endl;
    std::vector<IUPACPattern*> found;
    peng.process(params, found);
    peng.filter_redundancy(merge_bit_factor_threshold, found);
    check(pengk_synchronize(ctx), "pengk_synchronize");
    pengk_host::override_packed_input(nullptr, nullptr);
    pengk_host::set_dump_subdir("");
    lap("process");

    Round nr;
    nr.seeds = peng.last_seeds;
    nr.windows = peng.last_windows;
    nr.erased_before = erased_so_far;
    report.push_back(nr);
    prev.clear();
    for (IUPACPattern* p : found) {
      bool drop = false;
      for (IUPACPattern* k : result)
        if (redundant(k, p, bg, merge_bit_factor_threshold)) {
          drop = true;
          break;
        }
      if (drop) {
        std::cout << "erase: " << p->get_pattern_string() << " repeats an earlier motif, dropped" << std::endl;
        delete p;
      } else {
        prev.push_back(p);
      }
    }
    result.insert(result.end(), prev.begin(), prev.end());
    // this round's output is the next one's input
    cur = next;
    next = next == va.get() ? vb.get() : va.get();
  }

  if (pengk_host::rank() == 0) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) {
      std::cerr << "Error: cannot write " << path << std::endl;
      exit(1);
    }
    fprintf(f, "#round\tmotif_id\twidth\tthreshold\tsites\tround_seeds\tround_windows\tround_bases_erased\n");
    for (size_t r = 0; r < report.size(); ++r) {
      const Round& rd = report[r];
      if (rd.motifs.empty())
        fprintf(f, "%zu\t-\t0\t-\t0\t%zu\t%zu\t%llu\n", r + 1, rd.seeds, rd.windows, rd.erased_before);
      for (const MotifLine& m : rd.motifs)
        fprintf(f, "%zu\t%s\t%d\t%s\t%llu\t%zu\t%zu\t%llu\n", r + 1, m.id.c_str(), m.w, score_str(m.thr).c_str(), m.sites, rd.seeds,
                rd.windows, rd.erased_before);
    }
    fclose(f);
  }
}
