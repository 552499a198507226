#include "motif_centrality.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <iostream>

#include "device.h"

void write_motif_centrality(const std::vector<IUPACPattern*>& pats, SequenceSet& set, const ScanInput& in, BackgroundModel& bg,
                            bool both_strands, double pvalue, const std::string& path) {
  using pengk_host::check;
  using pengk_host::DeviceBuffer;
  pengk_host::Lap lap("  centrality: ");
  const int n_motifs = (int)pats.size();
  const size_t n_local = in.n_local;
  const float* bg0 = bg.getV()[0];
  std::vector<int32_t> S, len;
  motif_log_odds(pats, bg0, S, len, "motif centrality");
  // thresholds: the smallest integer score whose tail p-value is at most `pvalue` (hi + 1: no site), as --sites
  std::vector<int32_t> thr(std::max(n_motifs, 1), 0);
  for (int m = 0; m < n_motifs; ++m) {
    const int32_t* Sm = &S[(size_t)m * PENGK_MAX_MOTIF_LEN * 4];
    int32_t lo = 0, hi = 0;
    check(pengk_score_tail_pvalues(Sm, len[m], bg0, &lo, &hi, nullptr), "pengk_score_tail_pvalues");
    std::vector<double> tail((size_t)(hi - lo) + 1);
    check(pengk_score_tail_pvalues(Sm, len[m], bg0, &lo, &hi, tail.data()), "pengk_score_tail_pvalues");
    check(pengk_score_threshold(tail.data(), lo, hi, pvalue, &thr[m]), "pengk_score_threshold");
  }

  // the considered records (w <= L <= PENGK_CENTRALITY_MAX_LEN) by width, and the longest of them over all ranks: the
  // histograms' range
  std::vector<long long> shorter(PENGK_MAX_MOTIF_LEN + 1, 0);  // records of L < 64 bases by L
  long long n_ok = 0;
  uint64_t lmax = 1;
  for (size_t c = 0; c < set.nChunks(); ++c) {
    const SequenceChunk& ch = set.chunk(c);
    for (size_t k = 0; k < ch.n; ++k) {
      const uint64_t L = (uint64_t)(ch.offs[k + 1] - ch.offs[k]);
      if (L > PENGK_CENTRALITY_MAX_LEN) continue;
      ++n_ok;
      lmax = std::max(lmax, L);
      if (L < (uint64_t)PENGK_MAX_MOTIF_LEN) ++shorter[L];
    }
  }
  const int R = pengk_host::world();
  if (R > 1) {
    std::vector<uint64_t> all(R);
    check(pengk_comm_host_allgather(&lmax, all.data(), sizeof(uint64_t)), "pengk_comm_host_allgather");
    lmax = *std::max_element(all.begin(), all.end());
  }
  const uint32_t max_len = (uint32_t)lmax;
  const size_t nd = 2 * (size_t)max_len + 1, nl = (size_t)max_len + 1;
  lap("thresholds + lengths");

  // per motif: offset bins, length bins, then one counter per motif (the considered records): summed over the ranks
  const size_t nh = (size_t)n_motifs * (nd + nl);
  std::vector<long long> hist(nh + n_motifs, 0);
  if (n_motifs && n_local) {
    pengk_ctx* ctx = pengk_host::context();
    DeviceBuffer<int32_t> d_best((size_t)n_motifs * n_local);
    DeviceBuffer<uint64_t> d_site((size_t)n_motifs * n_local);
    DeviceBuffer<uint64_t> d_hist(nh);
    check(pengk_memset(ctx, d_hist.get(), 0, nh * sizeof(uint64_t)), "pengk_memset");
    check(pengk_motif_best_sites(ctx, in.d_words.get(), in.d_valid.get(), in.d_offs.get(), in.d_lens.get(), n_local,
                                 set.getLocalBase(), n_motifs, S.data(), len.data(), both_strands ? 1 : 0, d_best.get(),
                                 d_site.get()),
          "pengk_motif_best_sites");
    check(pengk_centrality_histograms(ctx, n_motifs, d_best.get(), d_site.get(), in.d_lens.get(), n_local, len.data(), thr.data(),
                                      max_len, d_hist.get(), d_hist.get() + (size_t)n_motifs * nd),
          "pengk_centrality_histograms");
    d_hist.download((uint64_t*)hist.data(), nh);
  }
  for (int m = 0; m < n_motifs; ++m) {
    long long n = n_ok;
    for (int L = 0; L < len[m]; ++L) n -= shorter[L];
    hist[nh + m] = n;
  }
  lap("best sites + histograms");
  SequenceSet::allreduceSum(hist.data(), hist.size());  // (integers: the ranks' sum is exact)
  if (pengk_host::rank() != 0) return;

  FILE* f = fopen(path.c_str(), "wb");
  if (!f) {
    std::cerr << "Unable to open output file (" << path << ")!" << std::endl;
    exit(1);
  }
  std::string o =
      "#motif_index\tmotif_id\twidth\tsequences\tsites\tcenter_distance\tsites_in_window\texpected_in_window\tenrichment\t"
      "log10_pvalue\tlog10_evalue\toffsets\n";
  char b[256];
  for (int m = 0; m < n_motifs; ++m) {
    const uint64_t* hd = (const uint64_t*)hist.data() + (size_t)m * nd;
    const uint64_t* hl = (const uint64_t*)hist.data() + (size_t)n_motifs * nd + (size_t)m * nl;
    pengk_centrality c;
    check(pengk_centrality_summary(hd, hl, max_len, len[m], n_motifs, &c), "pengk_centrality_summary");
    snprintf(b, sizeof b, "%d\t%s\t%d\t%lld\t%llu", m + 1, pats[m]->get_pattern_string().c_str(), len[m], hist[nh + m],
             (unsigned long long)c.sites);
    o += b;
    if (c.sites == 0) {
      o += "\tNA\tNA\tNA\tNA\tNA\tNA\tNA\n";
      continue;
    }
    snprintf(b, sizeof b, "\t%u%s\t%llu\t%.2f\t%.3f\t%.3f\t%.3f\t", c.window / 2, (c.window & 1) ? ".5" : "",
             (unsigned long long)c.in_window, c.expected, (double)c.in_window / c.expected, c.log10_pvalue, c.log10_evalue);
    o += b;
    for (int64_t d = -(int64_t)c.max_offset; d <= (int64_t)c.max_offset; ++d) {
      if (d > -(int64_t)c.max_offset) o += ',';
      o += std::to_string(hd[max_len + d]);
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
