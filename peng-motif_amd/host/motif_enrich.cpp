#include "motif_enrich.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>

#include "device.h"

void enrich_log_odds(const MemeMotif& t, const float* bg0, int32_t* S) {
  for (int j = 0; j < t.w; ++j) {
    const double* r = &t.rows[(size_t)j * 4];
    const double sum = ((r[0] + r[1]) + r[2]) + r[3];
    for (int a = 0; a < 4; ++a) {
      const double p = (r[a] / sum + 0.01 * (double)bg0[a]) / 1.01;
      S[j * 4 + a] = log_odds((float)p, bg0[a]);
    }
  }
}

void write_motif_enrich(const std::vector<MemeMotif>& db, const ScanInput& in, Negatives& neg, BackgroundModel& bg,
                        bool both_strands, const EnrichSettings& es, const std::string& path) {
  using pengk_host::check;
  using pengk_host::DeviceBuffer;
  pengk_host::Lap lap("  enrich: ");
  const int n_db = (int)db.size();
  const size_t n_local = in.n_local;
  const size_t ML = PENGK_MAX_MOTIF_LEN;
  const float* bg0 = bg.getV()[0];

  // log-odds, thresholds (the smallest score with a tail at or below es.pvalue; hi + 1: no bin) and their tails
  std::vector<int32_t> S((size_t)std::max(n_db, 1) * ML * 4, 0), len(std::max(n_db, 1), 0), thr(std::max(n_db, 1), 0),
      hi(std::max(n_db, 1), 0), lo(std::max(n_db, 1), 0);
  std::vector<std::vector<double>> tails(n_db);  // tail[k]: of score thr + k
  std::vector<uint64_t> hoffs(n_db + 1, 0);
  for (int m = 0; m < n_db; ++m) {
    int32_t* Sm = &S[(size_t)m * ML * 4];
    len[m] = db[m].w;
    enrich_log_odds(db[m], bg0, Sm);
    check(pengk_score_tail_pvalues(Sm, len[m], bg0, &lo[m], &hi[m], nullptr), "pengk_score_tail_pvalues");
    std::vector<double> tail((size_t)(hi[m] - lo[m]) + 1);
    check(pengk_score_tail_pvalues(Sm, len[m], bg0, &lo[m], &hi[m], tail.data()), "pengk_score_tail_pvalues");
    check(pengk_score_threshold(tail.data(), lo[m], hi[m], es.pvalue, &thr[m]), "pengk_score_threshold");
    tails[m].assign(tail.begin() + (thr[m] - lo[m]), tail.end());
    hoffs[m + 1] = hoffs[m] + (uint64_t)(hi[m] - thr[m] + 1);
  }
  lap("log-odds + thresholds");

  // per set: the motifs' bins, then their scored counters
  const uint64_t nh = hoffs[n_db], per_set = nh + (uint64_t)n_db;
  std::vector<uint64_t> hist(std::max<uint64_t>(2 * per_set, 1), 0);
  const size_t n_neg = neg.n(in);  // (a control set brings its own number of sequences)
  if (n_db && (n_local || n_neg)) {
    pengk_ctx* ctx = pengk_host::context();
    DeviceBuffer<uint64_t> d_hist(2 * per_set);
    check(pengk_memset(ctx, d_hist.get(), 0, 2 * per_set * sizeof(uint64_t)), "pengk_memset");
    const int both = both_strands ? 1 : 0;
    check(pengk_motif_enrich(ctx, in.d_words.get(), in.d_valid.get(), in.d_offs.get(), in.d_lens.get(), n_local, n_db, S.data(),
                             len.data(), both, thr.data(), hi.data(), hoffs.data(), d_hist.get(), d_hist.get() + nh),
          "pengk_motif_enrich");
    check(pengk_motif_enrich(ctx, neg.words(), neg.valid_or_null(), neg.offs(in), neg.lens(in), n_neg, n_db, S.data(), len.data(),
                             both, thr.data(), hi.data(), hoffs.data(), d_hist.get() + per_set, d_hist.get() + per_set + nh),
          "pengk_motif_enrich");
    d_hist.download(hist.data(), 2 * per_set);
  }
  lap("scans + histograms");
  if (pengk_host::world() > 1) check(pengk_comm_host_allreduce_u64(hist.data(), hist.size()), "pengk_comm_host_allreduce_u64");
  if (pengk_host::rank() != 0) return;

  std::vector<pengk_enrichment> e(n_db);
  for (int m = 0; m < n_db; ++m)
    check(pengk_enrich_summary(hist.data() + hoffs[m], hist.data() + per_set + hoffs[m], hoffs[m + 1] - hoffs[m], thr[m],
                               hist[nh + m], hist[per_set + nh + m], &e[m]),
          "pengk_enrich_summary");
  // the order of the file: adjusted p-value, then p-value, then database order
  std::vector<int> order(n_db);
  for (int m = 0; m < n_db; ++m) order[m] = m;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
    if (e[a].log10_adj_pvalue != e[b].log10_adj_pvalue) return e[a].log10_adj_pvalue < e[b].log10_adj_pvalue;
    return e[a].log10_pvalue < e[b].log10_pvalue;
  });
  // Benjamini-Hochberg over the database's adjusted p-values, in log10: from the last rank down a running minimum of
  // log10_adj + log10(n_db) - log10(rank)
  const double ln = std::log10((double)std::max(n_db, 1));
  std::vector<double> lq(n_db, 0.0);
  double mn = 0.0;
  for (int k = n_db; k-- > 0;) {
    mn = std::min(mn, e[order[k]].log10_adj_pvalue + ln - std::log10((double)(k + 1)));
    lq[k] = mn;
  }
  lap("summaries");

  std::string o =
      "rank\tmotif_id\talt_id\twidth\tthreshold\tthreshold_pvalue\tpos_hits\tpos_scored\tneg_hits\tneg_scored\tenrichment\t"
      "log10_pvalue\tlog10_adj_pvalue\tlog10_evalue\tq_value\n";
  const double max_le = std::log10(es.evalue);
  std::vector<char> line(512);
  for (int k = 0; k < n_db; ++k) {
    const int m = order[k];
    const double le = e[m].log10_adj_pvalue + ln;
    if (!(le <= max_le)) continue;
    const int32_t t = e[m].threshold;
    const double tp = t <= hi[m] ? tails[m][(size_t)(t - thr[m])] : 0.0;
    line.resize(db[m].id.size() + db[m].alt.size() + 384);
    snprintf(line.data(), line.size(), "%d\t%s\t%s\t%d\t%s%d.%02d\t%.3g\t%llu\t%llu\t%llu\t%llu\t%.3f\t%.3f\t%.3f\t%.3f\t%.3g\n", k + 1,
             db[m].id.c_str(), db[m].alt.empty() ? "." : db[m].alt.c_str(), db[m].w, t < 0 ? "-" : "", std::abs(t) / 100,
             std::abs(t) % 100, tp, (unsigned long long)e[m].pos_hits, (unsigned long long)hist[nh + m],
             (unsigned long long)e[m].neg_hits, (unsigned long long)hist[per_set + nh + m], e[m].enrichment, e[m].log10_pvalue,
             e[m].log10_adj_pvalue, le, std::pow(10.0, lq[k]));
    o += line.data();
  }
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
  lap("written");
}
