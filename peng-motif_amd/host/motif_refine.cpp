#include "motif_refine.h"

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>

#include "device.h"
#include "shared/Alphabet.h"

std::vector<RefinedMotif> refine_matrices(const std::vector<std::vector<float>>& start, SequenceSet& set, const ScanInput& in,
                                          BackgroundModel& bg, bool both_strands, const RefineSettings& rs) {
  using pengk_host::check;
  using pengk_host::DeviceBuffer;
  typedef RefinedMotif Refined;
  const int n_motifs = (int)start.size();
  const size_t n_local = in.n_local;
  const float* bg0 = bg.getV()[0];
  const size_t ROW = (size_t)PENGK_MAX_MOTIF_LEN * 4, BINS = (size_t)PENGK_MAX_MOTIF_LEN * 5;

  // round 0 starts from the matrices as they are given (as --sites and --centrality scan the found PWMs)
  std::vector<Refined> mot(n_motifs);
  std::vector<int32_t> S((size_t)std::max(n_motifs, 1) * ROW, 0), len(std::max(n_motifs, 1), 0);
  for (int m = 0; m < n_motifs; ++m) {
    mot[m].w = mot[m].w0 = (int)(start[m].size() / 4);
    mot[m].pwm = start[m];
  }

  pengk_ctx* ctx = pengk_host::context();
  const bool device = n_motifs && n_local;
  DeviceBuffer<int32_t> d_best(device ? (size_t)n_motifs * n_local : 1);
  DeviceBuffer<uint64_t> d_site(device ? (size_t)n_motifs * n_local : 1);
  DeviceBuffer<uint64_t> d_counts(std::max<size_t>(n_motifs, 1) * BINS);
  std::vector<int32_t> thr(std::max(n_motifs, 1), 0);
  std::vector<long long> counts((size_t)n_motifs * BINS);
  for (int t = 0; t < rs.iterations; ++t) {
    bool any = false;
    for (int m = 0; m < n_motifs; ++m) any |= mot[m].active;
    if (!any) break;
    // every motif is scanned in every round, under its index: the tie-break's key holds it.  One that has stopped
    // gets a threshold no score reaches.
    for (int m = 0; m < n_motifs; ++m) {
      const Refined& r = mot[m];
      int32_t* Sm = &S[(size_t)m * ROW];
      len[m] = r.w;
      for (int j = 0; j < r.w; ++j)
        for (int a = 0; a < 4; ++a) Sm[(size_t)j * 4 + a] = log_odds(r.pwm[(size_t)j * 4 + a], bg0[a]);
      if (!r.active) {
        thr[m] = INT32_MAX;
        continue;
      }
      int32_t lo = 0, hi = 0;
      check(pengk_score_tail_pvalues(Sm, r.w, bg0, &lo, &hi, nullptr), "pengk_score_tail_pvalues");
      std::vector<double> tail((size_t)(hi - lo) + 1);
      check(pengk_score_tail_pvalues(Sm, r.w, bg0, &lo, &hi, tail.data()), "pengk_score_tail_pvalues");
      check(pengk_score_threshold(tail.data(), lo, hi, rs.pvalue, &thr[m]), "pengk_score_threshold");
    }
    std::fill(counts.begin(), counts.end(), 0);
    if (device) {
      check(pengk_memset(ctx, d_counts.get(), 0, (size_t)n_motifs * BINS * sizeof(uint64_t)), "pengk_memset");
      check(pengk_motif_best_sites(ctx, in.d_words.get(), in.d_valid.get(), in.d_offs.get(), in.d_lens.get(), n_local,
                                   set.getLocalBase(), n_motifs, S.data(), len.data(), both_strands ? 1 : 0, d_best.get(),
                                   d_site.get()),
            "pengk_motif_best_sites");
      check(pengk_site_profiles(ctx, in.d_words.get(), in.d_valid.get(), in.d_offs.get(), in.d_lens.get(), n_local, n_motifs,
                                d_best.get(), d_site.get(), len.data(), thr.data(), rs.flank, d_counts.get()),
            "pengk_site_profiles");
      d_counts.download((uint64_t*)counts.data(), counts.size());
    }
    SequenceSet::allreduceSum(counts.data(), counts.size());  // (integers: the ranks' sum is exact)
    for (int m = 0; m < n_motifs; ++m) {
      Refined& r = mot[m];
      if (!r.active) continue;
      const uint64_t* k = (const uint64_t*)counts.data() + (size_t)m * BINS;
      float pwm[PENGK_MAX_MOTIF_LEN * 4];
      int32_t first = 0, last = 0;
      uint64_t sites = 0;
      check(pengk_profile_refine(k, r.w, rs.flank, bg0, rs.min_ic, nullptr, nullptr, pwm, &first, &last, &sites),
            "pengk_profile_refine");
      if (sites == 0 || last == first) {  // no site, or no column worth keeping: the matrix it had
        r.active = false;
        continue;
      }
      const int F = std::min(rs.flank, (PENGK_MAX_MOTIF_LEN - r.w) / 2);
      const int a = -r.left - F + first, b = -r.left - F + last;  // in the found PWM's columns
      std::vector<long long> kept(counts.begin() + (size_t)m * BINS + (size_t)first * 5,
                                  counts.begin() + (size_t)m * BINS + (size_t)last * 5);
      if (r.have_prev && a == r.prev_first && b == r.prev_last && kept == r.prev_counts) r.active = false;  // (the same matrix)
      r.have_prev = true;
      r.prev_first = a;
      r.prev_last = b;
      r.prev_counts.swap(kept);
      r.w = last - first;
      r.pwm.assign(pwm, pwm + (size_t)r.w * 4);
      r.left = -a;
      r.right = b - r.w0;
      r.rounds += 1;
      r.sites = (long long)sites;
    }
  }
  return mot;
}

void write_refined_meme(const std::vector<RefinedMotif>& mot, const std::vector<std::string>& names, const float* bg0,
                        const std::string& path) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) {
    std::cerr << "Unable to open output file (" << path << ")!" << std::endl;
    exit(1);
  }
  // (the header of Peng::printShortMeme, and its 8-decimal rows)
  const char* alphabet = Alphabet::getAlphabet();
  std::ostringstream head;
  head << "MEME version 4" << std::endl << std::endl;
  head << "ALPHABET= " << alphabet << std::endl << std::endl;
  head << "Background letter frequencies" << std::endl;
  for (size_t i = 0; i < strlen(alphabet); ++i) head << (i ? " " : "") << alphabet[i] << " " << bg0[i];
  head << std::endl << std::endl;
  std::string o = head.str();
  char line[256];
  for (size_t m = 0; m < mot.size(); ++m) {
    const RefinedMotif& r = mot[m];
    snprintf(line, sizeof line, "letter-probability matrix: alength= 4 w= %d nsites= %lld iterations= %d left= %d right= %d\n", r.w,
             r.sites, r.rounds, r.left, r.right);
    o += "MOTIF " + names[m] + "\n" + line;
    for (int j = 0; j < r.w; ++j) {
      const float* q = &r.pwm[(size_t)j * 4];
      snprintf(line, sizeof line, "%.8f %.8f %.8f %.8f\n", (double)q[0], (double)q[1], (double)q[2], (double)q[3]);
      o += line;
    }
    o += "\n";
  }
  const bool ok = fwrite(o.data(), 1, o.size(), f) == o.size();
  if ((fclose(f) != 0) || !ok) {
    std::cerr << "Error: writing " << path << " failed" << std::endl;
    exit(1);
  }
}

void write_refined_motifs(const std::vector<IUPACPattern*>& pats, SequenceSet& set, const ScanInput& in, BackgroundModel& bg,
                          bool both_strands, const RefineSettings& rs, const std::string& path) {
  pengk_host::Lap lap("  refine: ");
  const float* bg0 = bg.getV()[0];
  std::vector<int32_t> S, len;
  motif_log_odds(pats, bg0, S, len, "motif refinement");  // (a motif wider than PENGK_MAX_MOTIF_LEN ends the program here)
  std::vector<std::vector<float>> start(pats.size());
  std::vector<std::string> names(pats.size());
  for (size_t m = 0; m < pats.size(); ++m) {
    start[m].resize((size_t)len[m] * 4);
    for (int j = 0; j < len[m]; ++j)
      for (int a = 0; a < 4; ++a) start[m][(size_t)j * 4 + a] = pats[m]->get_pwm()[j][a];
    names[m] = pats[m]->get_pattern_string();
  }
  const std::vector<RefinedMotif> mot = refine_matrices(start, set, in, bg, both_strands, rs);
  lap("rounds");
  if (pengk_host::rank() != 0) return;
  write_refined_meme(mot, names, bg0, path);
  lap("written");
}
