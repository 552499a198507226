#include "motif_compare.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>

#include "device.h"

void write_motif_compare(const std::vector<IUPACPattern*>& pats, const std::vector<MemeMotif>& db, bool both_strands,
                         const CompareSettings& cs, const std::string& path) {
  using pengk_host::check;
  pengk_host::Lap lap("  compare: ");
  const int n_q = (int)pats.size(), n_t = (int)db.size();
  const size_t ML = PENGK_MAX_MOTIF_LEN;

  // quantised columns of both sides (host, once per motif)
  std::vector<int16_t> QX((size_t)std::max(n_q, 1) * ML * 4, 0), TX((size_t)std::max(n_t, 1) * ML * 4, 0);
  std::vector<int32_t> qlen(std::max(n_q, 1), 0), tlen(std::max(n_t, 1), 0);
  for (int m = 0; m < n_q; ++m) {
    const int w = (int)pats[m]->get_pattern_length();
    if (w > PENGK_MAX_MOTIF_LEN) {
      std::cerr << "Error: motif comparison: motif width " << w << " above " << PENGK_MAX_MOTIF_LEN << std::endl;
      exit(1);
    }
    qlen[m] = w;
    float** pwm = pats[m]->get_pwm();
    std::vector<double> rows((size_t)w * 4);
    for (int j = 0; j < w; ++j)
      for (int a = 0; a < 4; ++a) rows[(size_t)j * 4 + a] = (double)pwm[j][a];
    check(pengk_compare_quantize(rows.data(), w, &QX[(size_t)m * ML * 4]), "pengk_compare_quantize");
  }
  for (int t = 0; t < n_t; ++t) {
    tlen[t] = db[t].w;
    check(pengk_compare_quantize(db[t].rows.data(), db[t].w, &TX[(size_t)t * ML * 4]), "pengk_compare_quantize");
  }
  if (const char* dump = std::getenv("PENGK_COMPARE_QUERIES")) {
    if (FILE* f = fopen(dump, "wb")) {
      for (int m = 0; m < n_q; ++m) {
        fprintf(f, "%d %d %s\n", m + 1, qlen[m], pats[m]->get_pattern_string().c_str());
        for (int j = 0; j < qlen[m]; ++j) {
          const int16_t* r = &QX[((size_t)m * ML + j) * 4];
          fprintf(f, "%d %d %d %d\n", (int)r[0], (int)r[1], (int)r[2], (int)r[3]);
        }
      }
      fclose(f);
    }
  }
  lap("quantised");

  std::vector<int32_t> align((size_t)std::max(n_q, 1) * n_t * 5, 0);
  std::vector<double> p((size_t)std::max(n_q, 1) * n_t, 1.0);
  if (n_q)
    check(pengk_compare_motifs(pengk_host::context(), n_q, QX.data(), qlen.data(), n_t, TX.data(), tlen.data(),
                               both_strands ? 1 : 0, cs.min_overlap, align.data(), p.data()),
          "pengk_compare_motifs");
  lap("nulls + tails + alignments");

  std::string o = "motif\tiupac\ttarget\ttarget_width\toffset\torientation\toverlap\tscore\tn_offsets\tp_offset\tp_value\te_value\tq_value\n";
  std::vector<double> pm(n_t), ev(n_t), qv(n_t);
  std::vector<int32_t> noff(n_t);
  std::vector<int> order(n_t);
  std::vector<char> line(512);
  for (int m = 0; m < n_q; ++m) {
    const int32_t* al = &align[(size_t)m * n_t * 5];
    const double* pq = &p[(size_t)m * n_t];
    for (int t = 0; t < n_t; ++t) noff[t] = al[(size_t)t * 5 + 4];
    check(pengk_compare_summary(pq, noff.data(), n_t, pm.data(), ev.data(), qv.data()), "pengk_compare_summary");
    for (int t = 0; t < n_t; ++t) order[t] = t;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return pm[a] < pm[b]; });
    const std::string iupac = pats[m]->get_pattern_string();
    for (int t : order) {
      if (!(ev[t] <= cs.evalue)) continue;
      const int32_t* a = al + (size_t)t * 5;
      line.resize(iupac.size() + db[t].id.size() + 256);
      snprintf(line.data(), line.size(), "%d\t%s\t%s\t%d\t%d\t%s\t%d\t%d\t%d\t%.6e\t%.6e\t%.6e\t%.6e\n", m + 1, iupac.c_str(),
               db[t].id.c_str(), db[t].w, a[0], a[1] ? "-" : "+", a[2], a[3], a[4], pq[t], pm[t], ev[t], qv[t]);
      o += line.data();
    }
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
