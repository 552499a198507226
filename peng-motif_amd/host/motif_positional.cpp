#include "motif_positional.h"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <vector>

#include "device.h"

std::string positional_word_string(uint32_t key, int width) {
  static const char kLetters[] = "ACGT";
  std::string s;
  for (int c = 0; c < width; ++c) s += kLetters[(key >> (2 * (width - 1 - c))) & 3u];
  return s;
}

void write_positional(const ScanInput& in, const uint32_t* d_valid, const ScanSubset* training, bool both_strands,
                      const PositionalSettings& ps, const char* path) {
  using pengk_host::check;
  using pengk_host::DeviceBuffer;
  static const char* const kAnchor[3] = {"start", "end", "center"};
  pengk_host::Lap lap("  positional: ");
  pengk_ctx* ctx = pengk_host::context();
  const size_t NK = (size_t)1 << (2 * ps.width), N = (size_t)ps.bins * NK;
  const size_t n_local = training ? training->n : in.n_local;

  const size_t NP = ps.composition_null ? (size_t)ps.bins * 16 : 0;  // the pair table, behind the word table in one buffer
  std::vector<uint64_t> tab(N + NP, 0);
  if (n_local) {
    DeviceBuffer<uint64_t> d_tab(N + NP);
    check(pengk_memset(ctx, d_tab.get(), 0, (N + NP) * sizeof(uint64_t)), "pengk_memset");
    check(pengk_position_count(ctx, in.d_words.get(), d_valid ? d_valid : in.d_valid.get(), training ? training->d_offs : in.d_offs.get(),
                               training ? training->d_lens : in.d_lens.get(), n_local, ps.width, ps.anchor, ps.bin_size, ps.bins,
                               both_strands ? 1 : 0, d_tab.get()),
          "pengk_position_count");
    if (NP)
      check(pengk_position_pairs(ctx, in.d_words.get(), d_valid ? d_valid : in.d_valid.get(), training ? training->d_offs : in.d_offs.get(),
                                 training ? training->d_lens : in.d_lens.get(), n_local, ps.width, ps.anchor, ps.bin_size, ps.bins,
                                 both_strands ? 1 : 0, d_tab.get() + N),
            "pengk_position_pairs");
    d_tab.download(tab.data(), N + NP);
  }
  if (pengk_host::world() > 1) check(pengk_comm_host_allreduce_u64(tab.data(), N + NP), "pengk_comm_host_allreduce_u64");
  const uint64_t* pairs = NP ? tab.data() + N : nullptr;
  lap("count");

  std::vector<pengk_position_word> rep(256);
  uint64_t n = 0;
  check(pengk_position_summary_null(tab.data(), pairs, ps.width, ps.bins, both_strands ? 1 : 0, ps.min_count, ps.evalue, rep.data(),
                                    rep.size(), &n),
        "pengk_position_summary_null");
  if (n > rep.size()) {
    rep.resize(n);
    check(pengk_position_summary_null(tab.data(), pairs, ps.width, ps.bins, both_strands ? 1 : 0, ps.min_count, ps.evalue, rep.data(),
                                      rep.size(), &n),
          "pengk_position_summary_null");
  }
  rep.resize(n);
  size_t families = 0;
  for (const pengk_position_word& w : rep) families += w.is_head;
  uint64_t counted = 0;
  for (size_t k = 0; k < N; ++k) counted += tab[k];
  lap("summary");

  std::cout << "positional (width " << ps.width << ", " << ps.bins << " bins of " << ps.bin_size << " from the " << kAnchor[ps.anchor]
            << ", " << (both_strands ? "both strands" : "plus strand") << ", " << counted << " words"
            << (pairs ? ", composition null" : "") << "): " << rep.size()
            << " at E-value <= " << ps.evalue << " in " << families << (families == 1 ? " family" : " families");
  if (!rep.empty())
    std::cout << "; the first: " << positional_word_string(rep[0].key, ps.width) << " in bin " << rep[0].bin << ", " << rep[0].count
              << " times";
  std::cout << std::endl;

  if (pengk_host::rank() != 0) return;
  std::string o = std::string("rank\tword\tbin\tcount\ttotal\tbin_positions\texpected\t") + (pairs ? "flat_expected\t" : "") +
                  "enrichment\tlog10_pvalue\tlog10_evalue\tbins_significant\tfamily\tis_head\tprofile\n";
  char buf[256];
  for (size_t k = 0; k < rep.size(); ++k) {
    const pengk_position_word& w = rep[k];
    snprintf(buf, sizeof buf, "%zu\t%s\t%u\t%llu\t%llu\t%llu\t%.2f\t", k + 1, positional_word_string(w.key, ps.width).c_str(), w.bin,
             (unsigned long long)w.count, (unsigned long long)w.total, (unsigned long long)w.bin_positions, w.expected);
    o += buf;
    if (pairs) {  // what the flat null expects: the word's count times the bin's share of all words
      snprintf(buf, sizeof buf, "%.2f\t", (double)w.total * ((double)w.bin_positions / (double)counted));
      o += buf;
    }
    snprintf(buf, sizeof buf, "%.3f\t%.3f\t%.3f\t%u\t%u\t%u\t", (double)w.count / w.expected, w.log10_pvalue, w.log10_evalue,
             w.bins_significant, w.family, w.is_head);
    o += buf;
    for (int b = 0; b < ps.bins; ++b) {  // the key's whole profile
      if (b) o += ',';
      o += std::to_string((unsigned long long)tab[(size_t)b * NK + w.key]);
    }
    o += '\n';
  }
  FILE* f = fopen(path, "wb");
  const bool ok = f && fwrite(o.data(), 1, o.size(), f) == o.size();
  if (!f || (fclose(f) != 0) || !ok) {
    std::cerr << "Error: writing " << path << " failed" << std::endl;
    exit(1);
  }
  lap("written");
}
