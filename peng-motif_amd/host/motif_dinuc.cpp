#include "motif_dinuc.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <iostream>

#include "device.h"

namespace {
void write_file(const std::string& path, const std::string& o) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) {
    std::cerr << "Unable to open output file (" << path << ")!" << std::endl;
    exit(1);
  }
  const bool ok = fwrite(o.data(), 1, o.size(), f) == o.size();
  if ((fclose(f) != 0) || !ok) {
    std::cerr << "Error: writing " << path << " failed" << std::endl;
    exit(1);
  }
}
}  // namespace

void write_motif_dinuc(const std::vector<IUPACPattern*>& pats, SequenceSet& set, const ScanInput& in, BackgroundModel& bg,
                       bool both_strands, const DinucSettings& ds, const std::string& report_path,
                       const std::string& models_path, Negatives* shared) {
  using pengk_host::check;
  using pengk_host::DeviceBuffer;
  pengk_host::Lap lap("  dinuc: ");
  const int n_motifs = (int)pats.size();
  const size_t n_local = in.n_local;
  const int both = both_strands ? 1 : 0;
  const float* bg0 = bg.getV()[0];
  float bg1[16];
  for (int a = 0; a < 4; ++a)
    for (int b = 0; b < 4; ++b) bg1[4 * a + b] = ds.bg_order >= 1 ? bg.getV()[1][4 * a + b] : bg0[b];
  const size_t ML = PENGK_MAX_MOTIF_LEN, B1 = ML * 5, B2 = ML * 17;

  // the found PWMs' log-odds and thresholds (as --sites, --centrality and --refine scan them)
  std::vector<int32_t> S, len, thr(std::max(n_motifs, 1), 0);
  motif_log_odds(pats, bg0, S, len, "first-order models");
  for (int m = 0; m < n_motifs; ++m) {
    const int32_t* Sm = &S[(size_t)m * ML * 4];
    int32_t lo = 0, hi = 0;
    check(pengk_score_tail_pvalues(Sm, len[m], bg0, &lo, &hi, nullptr), "pengk_score_tail_pvalues");
    std::vector<double> tail((size_t)(hi - lo) + 1);
    check(pengk_score_tail_pvalues(Sm, len[m], bg0, &lo, &hi, tail.data()), "pengk_score_tail_pvalues");
    check(pengk_score_threshold(tail.data(), lo, hi, ds.pvalue, &thr[m]), "pengk_score_threshold");
  }

  // single and pair profiles of the best sites, summed over the ranks
  pengk_ctx* ctx = pengk_host::context();
  const bool device = n_motifs && n_local;
  std::vector<long long> counts((size_t)n_motifs * (B1 + B2), 0);
  const size_t n_neg = shared ? shared->n(in) : n_local;  // (a control set brings its own number of sequences)
  DeviceBuffer<int32_t> d_best((size_t)std::max(n_motifs, 1) * std::max<size_t>(std::max(n_local, n_neg), 1));
  if (device) {
    DeviceBuffer<uint64_t> d_site((size_t)n_motifs * n_local);
    DeviceBuffer<uint64_t> d_counts(counts.size());
    check(pengk_memset(ctx, d_counts.get(), 0, counts.size() * sizeof(uint64_t)), "pengk_memset");
    check(pengk_motif_best_sites(ctx, in.d_words.get(), in.d_valid.get(), in.d_offs.get(), in.d_lens.get(), n_local,
                                 set.getLocalBase(), n_motifs, S.data(), len.data(), both, d_best.get(), d_site.get()),
          "pengk_motif_best_sites");
    check(pengk_site_profiles(ctx, in.d_words.get(), in.d_valid.get(), in.d_offs.get(), in.d_lens.get(), n_local, n_motifs,
                              d_best.get(), d_site.get(), len.data(), thr.data(), ds.flank, d_counts.get()),
          "pengk_site_profiles");
    check(pengk_site_pair_profiles(ctx, in.d_words.get(), in.d_valid.get(), in.d_offs.get(), in.d_lens.get(), n_local, n_motifs,
                                   d_best.get(), d_site.get(), len.data(), thr.data(), ds.flank,
                                   d_counts.get() + (size_t)n_motifs * B1),
          "pengk_site_pair_profiles");
    d_counts.download((uint64_t*)counts.data(), counts.size());
  }
  SequenceSet::allreduceSum(counts.data(), counts.size());  // (integers: the ranks' sum is exact)
  lap("best sites + profiles");

  // the models
  struct Model {
    int W = 0, F = 0;
    uint64_t sites = 0;
    std::vector<double> q0, q1, mi;
  };
  std::vector<Model> mod(n_motifs);
  std::vector<int32_t> wide(std::max(n_motifs, 1), 1), S0((size_t)std::max(n_motifs, 1) * 4, 0);
  std::vector<int32_t> D[2];  // D0, D1
  for (auto& d : D) d.assign((size_t)std::max(n_motifs, 1) * ML * 16, 0);
  for (int m = 0; m < n_motifs; ++m) {
    Model& r = mod[m];
    r.F = std::min(ds.flank, (PENGK_MAX_MOTIF_LEN - len[m]) / 2);
    r.W = wide[m] = len[m] + 2 * r.F;
    r.q0.resize((size_t)r.W * 4);
    r.q1.resize((size_t)r.W * 16);
    r.mi.resize(r.W);
    check(pengk_dinuc_model((const uint64_t*)counts.data() + (size_t)m * B1,
                            (const uint64_t*)counts.data() + (size_t)n_motifs * B1 + (size_t)m * B2, len[m], ds.flank, bg0, bg1,
                            ds.alpha, r.q0.data(), r.q1.data(), r.mi.data(), &S0[(size_t)m * 4], &D[1][(size_t)m * ML * 16],
                            &D[0][(size_t)m * ML * 16], &r.sites),
          "pengk_dinuc_model");
  }

  // both models over the input and over the negatives of --score-motifs
  Negatives own;
  if (!shared) build_negatives(set, in, bg, ds.bg_order, ds.seed, ds.shuffled, &own);
  Negatives& neg = shared ? *shared : own;
  std::vector<double> auc((size_t)2 * std::max(n_motifs, 1), 0.0);
  for (int k = 0; k < 2; ++k) {
    std::vector<int32_t> lo(std::max(n_motifs, 1), 0), hi(std::max(n_motifs, 1), 0);
    std::vector<uint64_t> hoffs(n_motifs + 1, 0);
    for (int m = 0; m < n_motifs; ++m) {
      const int32_t* s0 = &S0[(size_t)m * 4];
      lo[m] = std::min(std::min(s0[0], s0[1]), std::min(s0[2], s0[3]));
      hi[m] = std::max(std::max(s0[0], s0[1]), std::max(s0[2], s0[3]));
      for (int c = 1; c < wide[m]; ++c) {
        const int32_t* d = &D[k][((size_t)m * ML + c) * 16];
        lo[m] += *std::min_element(d, d + 16);
        hi[m] += *std::max_element(d, d + 16);
      }
      hoffs[m + 1] = hoffs[m] + (uint64_t)(hi[m] - lo[m] + 2);
    }
    const uint64_t nh = std::max<uint64_t>(hoffs[n_motifs], 1);
    DeviceBuffer<uint64_t> d_hist(2 * nh);
    check(pengk_memset(ctx, d_hist.get(), 0, 2 * nh * sizeof(uint64_t)), "pengk_memset");
    check(pengk_motif_scan_dinuc(ctx, in.d_words.get(), in.d_valid.get(), in.d_offs.get(), in.d_lens.get(), n_local, n_motifs,
                                 S0.data(), D[k].data(), wide.data(), both, d_best.get()),
          "pengk_motif_scan_dinuc");
    check(pengk_score_histograms(ctx, n_motifs, d_best.get(), n_local, lo.data(), hi.data(), hoffs.data(), d_hist.get()),
          "pengk_score_histograms");
    check(pengk_motif_scan_dinuc(ctx, neg.words(), neg.valid_or_null(), neg.offs(in), neg.lens(in), n_neg, n_motifs, S0.data(),
                                 D[k].data(), wide.data(), both, d_best.get()),
          "pengk_motif_scan_dinuc");
    check(pengk_score_histograms(ctx, n_motifs, d_best.get(), n_neg, lo.data(), hi.data(), hoffs.data(), d_hist.get() + nh),
          "pengk_score_histograms");
    std::vector<long long> hist(2 * nh);
    d_hist.download((uint64_t*)hist.data(), 2 * nh);
    SequenceSet::allreduceSum(hist.data(), hist.size());  // (integers: the ranks' sum is exact)
    for (int m = 0; m < n_motifs; ++m) {
      double occur = 0.0;
      check(pengk_score_summary((const uint64_t*)hist.data() + hoffs[m], (const uint64_t*)hist.data() + nh + hoffs[m],
                                hoffs[m + 1] - hoffs[m], &auc[(size_t)2 * m + k], &occur),
            "pengk_score_summary");
    }
  }
  lap("models + scans + histograms");
  if (pengk_host::rank() != 0) return;

  std::string o = "motif\tindex\twidth\tflank\tsites\tauc_order0\tauc_order1\tauc_gain\tmi_total\tmi_max\tmi_max_pair\n";
  char line[512];
  for (int m = 0; m < n_motifs; ++m) {
    const Model& r = mod[m];
    double a0 = 0.0, a1 = 0.0, total = 0.0, best = 0.0;
    int pair = 0;
    if (r.sites) {
      a0 = auc[(size_t)2 * m];
      a1 = auc[(size_t)2 * m + 1];
      for (int c = 1; c < r.W; ++c) {
        total += r.mi[c];
        if (c == 1 || r.mi[c] > best) {  // (the smaller column wins ties)
          best = r.mi[c];
          pair = c - r.F + 1;
        }
      }
    }
    snprintf(line, sizeof line, "%s\t%d\t%d\t%d\t%llu\t%.6f\t%.6f\t%.6f\t%.6f\t%.6f\t%d\n", pats[m]->get_pattern_string().c_str(),
             m + 1, r.W, r.F, (unsigned long long)r.sites, a0, a1, a1 - a0, total, best, pair);
    o += line;
  }
  write_file(report_path, o);
  if (!models_path.empty()) {
    snprintf(line, sizeof line, "# first-order motif models: alpha= %g bg_order= %d\n", ds.alpha, ds.bg_order >= 1 ? 1 : 0);
    o = line;
    for (int m = 0; m < n_motifs; ++m) {
      const Model& r = mod[m];
      snprintf(line, sizeof line, " w= %d nsites= %llu left= %d right= %d\n", r.W, (unsigned long long)r.sites, r.F, r.F);
      o += "MOTIF " + pats[m]->get_pattern_string() + line;
      for (int c = 0; c < r.W; ++c) {
        for (int b = 0; b < 4; ++b) {
          snprintf(line, sizeof line, "%s%.8f", b ? " " : "", r.q0[(size_t)c * 4 + b]);
          o += line;
        }
        o += "\n";
        for (int x = 0; x < 16; ++x) {
          snprintf(line, sizeof line, "%s%.8f", x ? " " : "", r.q1[(size_t)c * 16 + x]);
          o += line;
        }
        o += "\n";
      }
      o += "\n";
    }
    write_file(models_path, o);
  }
  lap("written");
}
