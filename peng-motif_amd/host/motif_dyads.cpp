#include "motif_dyads.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>

#include "device.h"

std::string dyad_string(uint32_t key, uint32_t gap) {
  static const char kLetters[] = "ACGT";
  std::string s;
  for (int c = 0; c < 3; ++c) s += kLetters[(key >> (10 - 2 * c)) & 3u];
  s.append(gap, 'n');
  for (int c = 0; c < 3; ++c) s += kLetters[(key >> (4 - 2 * c)) & 3u];
  return s;
}

void write_dyads(SequenceSet& set, const ScanInput& in, const uint32_t* d_valid, const ScanSubset* training, BackgroundModel& bg,
                 bool both_strands, const DyadSettings& ds, RefineSettings rs, const char* path, const char* motifs_path) {
  using pengk_host::check;
  using pengk_host::DeviceBuffer;
  pengk_host::Lap lap("  dyads: ");
  pengk_ctx* ctx = pengk_host::context();
  const size_t n_gaps = (size_t)ds.max_gap + 1, N = n_gaps * 4096 + 64;
  const size_t n_local = training ? training->n : in.n_local;

  // both tables in one buffer: counts | mono
  std::vector<uint64_t> tab(N, 0);
  if (n_local) {
    DeviceBuffer<uint64_t> d_tab(N);
    check(pengk_memset(ctx, d_tab.get(), 0, N * sizeof(uint64_t)), "pengk_memset");
    check(pengk_dyad_count(ctx, in.d_words.get(), d_valid ? d_valid : in.d_valid.get(), training ? training->d_offs : in.d_offs.get(),
                           training ? training->d_lens : in.d_lens.get(), n_local, ds.max_gap, both_strands ? 1 : 0, d_tab.get(),
                           d_tab.get() + n_gaps * 4096),
          "pengk_dyad_count");
    d_tab.download(tab.data(), N);
  }
  if (pengk_host::world() > 1) check(pengk_comm_host_allreduce_u64(tab.data(), N), "pengk_comm_host_allreduce_u64");
  lap("count");
  const uint64_t* counts = tab.data();
  const uint64_t* mono = tab.data() + n_gaps * 4096;

  // (every rank holds the summed tables and makes the same report: the refinement below is collective)
  std::vector<pengk_dyad> rep(256);
  uint64_t n = 0;
  check(pengk_dyad_summary(counts, mono, ds.max_gap, both_strands ? 1 : 0, ds.min_count, ds.evalue, rep.data(), rep.size(), &n),
        "pengk_dyad_summary");
  if (n > rep.size()) {
    rep.resize(n);
    check(pengk_dyad_summary(counts, mono, ds.max_gap, both_strands ? 1 : 0, ds.min_count, ds.evalue, rep.data(), rep.size(), &n),
          "pengk_dyad_summary");
  }
  rep.resize(n);
  size_t families = 0;
  for (const pengk_dyad& d : rep) families += d.is_head;
  uint64_t triplets = 0;
  for (int x = 0; x < 64; ++x) triplets += mono[x];
  lap("summary");

  std::cout << "dyads (gaps 0.." << ds.max_gap << ", " << (both_strands ? "both strands" : "plus strand") << ", " << triplets
            << " triplets): " << rep.size() << " at E-value <= " << ds.evalue << " in " << families
            << (families == 1 ? " family" : " families");
  if (!rep.empty()) std::cout << "; the first: " << dyad_string(rep[0].key, rep[0].gap) << ", " << rep[0].count << " times";
  std::cout << std::endl;

  if (pengk_host::rank() == 0) {
    std::string o = "rank\tdyad\tgap\tcount\tpositions\texpected\tenrichment\tlog10_pvalue\tlog10_evalue\tother_gaps_mean\tfamily\tis_head\n";
    char buf[256];
    for (size_t k = 0; k < rep.size(); ++k) {
      const pengk_dyad& d = rep[k];
      snprintf(buf, sizeof buf, "%zu\t%s\t%u\t%llu\t%llu\t%.2f\t%.3f\t%.3f\t%.3f\t%.2f\t%u\t%u\n", k + 1,
               dyad_string(d.key, d.gap).c_str(), d.gap, (unsigned long long)d.count, (unsigned long long)d.positions, d.expected,
               (double)d.count / d.expected, d.log10_pvalue, d.log10_evalue, d.other_gaps_mean, d.family, d.is_head);
      o += buf;
    }
    FILE* f = fopen(path, "wb");
    const bool ok = f && fwrite(o.data(), 1, o.size(), f) == o.size();
    if (!f || (fclose(f) != 0) || !ok) {
      std::cerr << "Error: writing " << path << " failed" << std::endl;
      exit(1);
    }
    lap("written");
  }
  if (!motifs_path) return;

  // the first family heads as matrices, through the rounds of --refine over the whole input
  const float* bg0 = bg.getV()[0];
  std::vector<std::vector<float>> start;
  std::vector<std::string> names;
  for (const pengk_dyad& d : rep) {
    if (!d.is_head) continue;
    if ((int)start.size() >= ds.top) break;
    const std::string s = dyad_string(d.key, d.gap);
    std::vector<float> pwm(s.size() * 4);
    for (size_t j = 0; j < s.size(); ++j)
      for (int a = 0; a < 4; ++a) pwm[j * 4 + a] = s[j] == 'n' ? bg0[a] : (s[j] == "ACGT"[a] ? 0.85f : 0.05f);
    start.push_back(pwm);
    names.push_back(s);
  }
  rs.pvalue = ds.pvalue;
  const std::vector<RefinedMotif> mot = refine_matrices(start, set, in, bg, both_strands, rs);
  lap("motifs: rounds");
  if (pengk_host::rank() != 0) return;
  write_refined_meme(mot, names, bg0, motifs_path);
  lap("motifs: written");
}
