#include "motif_spacing.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <iostream>

#include "device.h"

void write_motif_spacing(const std::vector<IUPACPattern*>& all_pats, SequenceSet& set, const ScanInput& in, BackgroundModel& bg,
                         bool both_strands, double pvalue, int max_gap, int max_motifs, const std::string& path) {
  using pengk_host::check;
  using pengk_host::DeviceBuffer;
  pengk_host::Lap lap("  spacing: ");
  const std::vector<IUPACPattern*> pats(all_pats.begin(), all_pats.begin() + std::min<size_t>(all_pats.size(), (size_t)max_motifs));
  const int n_motifs = (int)pats.size();
  const size_t n_local = in.n_local;
  const float* bg0 = bg.getV()[0];
  std::vector<int32_t> S, len;
  motif_log_odds(pats, bg0, S, len, "motif spacing");
  // thresholds: the smallest integer score whose tail p-value is at most `pvalue` (hi + 1: no site), as --centrality
  std::vector<int32_t> thr(std::max(n_motifs, 1), 0);
  uint32_t wmax = 1;
  for (int m = 0; m < n_motifs; ++m) {
    const int32_t* Sm = &S[(size_t)m * PENGK_MAX_MOTIF_LEN * 4];
    int32_t lo = 0, hi = 0;
    check(pengk_score_tail_pvalues(Sm, len[m], bg0, &lo, &hi, nullptr), "pengk_score_tail_pvalues");
    std::vector<double> tail((size_t)(hi - lo) + 1);
    check(pengk_score_tail_pvalues(Sm, len[m], bg0, &lo, &hi, tail.data()), "pengk_score_tail_pvalues");
    check(pengk_score_threshold(tail.data(), lo, hi, pvalue, &thr[m]), "pengk_score_threshold");
    wmax = std::max(wmax, (uint32_t)len[m]);
  }

  // the considered records (Wmax <= L <= max_len) and the longest record within the limit over all ranks
  long long n_ok = 0;
  uint64_t lmax = 1;
  for (size_t c = 0; c < set.nChunks(); ++c) {
    const SequenceChunk& ch = set.chunk(c);
    for (size_t k = 0; k < ch.n; ++k) {
      const uint64_t L = (uint64_t)(ch.offs[k + 1] - ch.offs[k]);
      if (L > PENGK_CENTRALITY_MAX_LEN) continue;
      lmax = std::max(lmax, L);
      if (L >= wmax) ++n_ok;
    }
  }
  const int R = pengk_host::world();
  if (R > 1) {
    std::vector<uint64_t> all(R);
    check(pengk_comm_host_allgather(&lmax, all.data(), sizeof(uint64_t)), "pengk_comm_host_allgather");
    lmax = *std::max_element(all.begin(), all.end());
  }
  const uint32_t max_len = (uint32_t)lmax;
  const uint32_t G = (uint32_t)max_gap;
  const size_t nb = 4 * ((size_t)G + 1) + 2, nl = (size_t)max_len + 1;
  const size_t pairs = (size_t)n_motifs * (size_t)std::max(n_motifs - 1, 0) / 2;
  lap("thresholds + lengths");

  // gap bins, length bins, n_m per motif, then the considered records: summed over the ranks
  const size_t o_len = pairs * nb, o_mot = o_len + pairs * nl, nh = o_mot + (size_t)n_motifs;
  std::vector<long long> hist(nh + 1, 0);
  if (n_motifs >= 2 && n_local) {
    pengk_ctx* ctx = pengk_host::context();
    DeviceBuffer<int32_t> d_best((size_t)n_motifs * n_local);
    DeviceBuffer<uint64_t> d_site((size_t)n_motifs * n_local);
    DeviceBuffer<uint64_t> d_hist(nh);
    check(pengk_memset(ctx, d_hist.get(), 0, nh * sizeof(uint64_t)), "pengk_memset");
    check(pengk_motif_best_sites(ctx, in.d_words.get(), in.d_valid.get(), in.d_offs.get(), in.d_lens.get(), n_local,
                                 set.getLocalBase(), n_motifs, S.data(), len.data(), both_strands ? 1 : 0, d_best.get(),
                                 d_site.get()),
          "pengk_motif_best_sites");
    check(pengk_spacing_histograms(ctx, n_motifs, d_best.get(), d_site.get(), in.d_lens.get(), n_local, len.data(), thr.data(), G,
                                   wmax, max_len, d_hist.get(), d_hist.get() + o_len, d_hist.get() + o_mot),
          "pengk_spacing_histograms");
    d_hist.download((uint64_t*)hist.data(), nh);
  }
  hist[nh] = n_ok;
  lap("best sites + histograms");
  SequenceSet::allreduceSum(hist.data(), hist.size());  // (integers: the ranks' sum is exact)
  if (pengk_host::rank() != 0) return;

  FILE* f = fopen(path.c_str(), "wb");
  if (!f) {
    std::cerr << "Unable to open output file (" << path << ")!" << std::endl;
    exit(1);
  }
  static const char* const kClass[4] = {"same_downstream", "same_upstream", "opposite_downstream", "opposite_upstream"};
  std::string o =
      "#motif_a\tid_a\tmotif_b\tid_b\tsequences\tsites_a\tsites_b\tboth\texpected_both\tlog10_pvalue_both\toverlapping\tapart\t"
      "far\torientation\tgap\tcount\texpected\tenrichment\tlog10_pvalue\tlog10_evalue\tgaps\n";
  char buf[512];
  const uint64_t* H = (const uint64_t*)hist.data();
  const uint64_t n = H[nh];
  for (int b = 1; b < n_motifs; ++b)
    for (int a = 0; a < b; ++a) {
      const size_t q = (size_t)b * (b - 1) / 2 + a;
      const uint64_t* hg = H + q * nb;
      pengk_spacing s;
      check(pengk_spacing_summary(hg, H + o_len + q * nl, G, max_len, len[a], len[b], both_strands ? 4 : 2, n, H[o_mot + a],
                                  H[o_mot + b], (int)pairs, &s),
            "pengk_spacing_summary");
      snprintf(buf, sizeof buf, "%d\t%s\t%d\t%s\t%llu\t%llu\t%llu\t%llu\t%.2f\t%.3f\t%llu\t%llu\t%llu", a + 1,
               pats[a]->get_pattern_string().c_str(), b + 1, pats[b]->get_pattern_string().c_str(), (unsigned long long)n,
               (unsigned long long)H[o_mot + a], (unsigned long long)H[o_mot + b], (unsigned long long)s.both, s.expected_both,
               s.log10_pvalue_both, (unsigned long long)s.overlapping, (unsigned long long)s.apart, (unsigned long long)s.far);
      o += buf;
      if (s.apart == 0) {
        o += "\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\n";
        continue;
      }
      snprintf(buf, sizeof buf, "\t%s\t%u\t%llu\t%.2f\t%.3f\t%.3f\t%.3f\t", kClass[s.orientation], s.gap, (unsigned long long)s.count,
               s.expected, (double)s.count / s.expected, s.log10_pvalue, s.log10_evalue);
      o += buf;
      for (uint32_t g = 0; g <= G; ++g) {
        if (g) o += ',';
        o += std::to_string(hg[(size_t)s.orientation * (G + 1) + g]);
      }
      o += '\n';
    }
  const bool ok = fwrite(o.data(), 1, o.size(), f) == o.size();
  if ((fclose(f) != 0) || !ok) {
    std::cerr << "Error: writing " << path << " failed" << std::endl;
    exit(1);
  }
  lap("summary + written");
}
