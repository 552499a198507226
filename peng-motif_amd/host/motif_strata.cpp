#include "motif_strata.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <memory>

#include "Global.h"
#include "device.h"

namespace {
const StratifiedNull* g_null = nullptr;

void write_or_die(const std::string& path, const void* p, size_t bytes, const char* what) {
  FILE* f = fopen(path.c_str(), "wb");
  const bool ok = f && fwrite(p, 1, bytes, f) == bytes;
  if (!f || (fclose(f) != 0) || !ok) {
    std::cerr << "Error: " << what << ": cannot write " << path << std::endl;
    exit(1);
  }
}
}  // namespace

namespace pengk_host {
void set_stratified_null(const StratifiedNull* null) { g_null = null; }
const StratifiedNull* stratified_null() { return g_null; }
}  // namespace pengk_host

void build_stratified_null(const ScanInput& in, const uint32_t* d_valid, const ScanSubset* training, SequenceSet* model_set, int W,
                           BackgroundModel& bg, const StratifiedSettings& st, StratifiedNull* out) {
  using pengk_host::check;
  using pengk_host::DeviceBuffer;
  pengk_host::Lap lap("  stratified background: ");
  pengk_ctx* ctx = pengk_host::context();
  const int G = st.gc_bins;

  // the source set M: another file's sequences in a scan layout of their own, else the input's
  std::unique_ptr<ScanInput> own;
  if (model_set) {
    own.reset(new ScanInput);
    build_scan_input(*model_set, own.get());
  }
  const ScanInput& src = own ? *own : in;

  // tab: the counted set's sequences per stratum (256) | its windows (G) | M's counters (G x 84)
  const size_t N_HIST = 256, N = N_HIST + (size_t)G + (size_t)G * 84;
  DeviceBuffer<uint64_t> d_tab(N + N_HIST);  // (behind them M's own 256 stratum counts, which nobody reads)
  check(pengk_memset(ctx, d_tab.get(), 0, (N + N_HIST) * sizeof(uint64_t)), "pengk_memset");
  uint64_t* d_hist = d_tab.get();
  uint64_t* d_windows = d_hist + N_HIST;
  uint64_t* d_bg = d_windows + G;

  const size_t n_counted = training ? training->n : in.n_local;
  const int64_t* c_offs = training ? training->d_offs : in.d_offs.get();
  const uint32_t* c_lens = training ? training->d_lens : in.d_lens.get();
  DeviceBuffer<uint16_t> d_stratum(std::max<size_t>(n_counted, 1)), d_src_stratum(std::max<size_t>(src.n_local, 1));
  DeviceBuffer<uint64_t> d_unused((size_t)G * 84);  // (the counted set's own counters: only its windows are asked for)
  check(pengk_memset(ctx, d_unused.get(), 0, (size_t)G * 84 * sizeof(uint64_t)), "pengk_memset");
  // the stratum is the sequence's own (its letters and validity as read); the windows are what round 1 can count
  check(pengk_seq_strata(ctx, in.d_words.get(), in.d_valid.get(), c_offs, c_lens, n_counted, G, 0, d_stratum.get(), d_hist),
        "pengk_seq_strata");
  check(pengk_strata_bg_count(ctx, in.d_words.get(), d_valid ? d_valid : in.d_valid.get(), c_offs, c_lens, n_counted, d_stratum.get(), G,
                              W, d_unused.get(), d_windows),
        "pengk_strata_bg_count");
  check(pengk_seq_strata(ctx, src.d_words.get(), src.d_valid.get(), src.d_offs.get(), src.d_lens.get(), src.n_local, G, 0,
                         d_src_stratum.get(), d_tab.get() + N),
        "pengk_seq_strata");
  check(pengk_strata_bg_count(ctx, src.d_words.get(), src.d_valid.get(), src.d_offs.get(), src.d_lens.get(), src.n_local,
                              d_src_stratum.get(), G, W, d_bg, nullptr),
        "pengk_strata_bg_count");
  std::vector<uint64_t> tab(N);
  d_tab.download(tab.data(), N);
  if (pengk_host::world() > 1) check(pengk_comm_host_allreduce_u64(tab.data(), N), "pengk_comm_host_allreduce_u64");
  lap("strata + counters");

  const uint64_t* hist = tab.data();
  const uint64_t* windows = hist + N_HIST;
  const uint64_t* counters = windows + G;
  float global_V[84] = {0};
  for (int o = 0, at = 0; o <= 2; at += 1 << (2 * (o + 1)), ++o)
    if (o <= bg.getOrder())
      for (int y = 0; y < (1 << (2 * (o + 1))); ++y) global_V[at + y] = bg.getV()[o][y];

  out->G = G;
  out->V.assign((size_t)G * 84, 0.0f);
  out->windows.assign(windows, windows + G);
  std::vector<uint64_t> bases(G, 0);
  std::vector<char> is_own(G, 0);
  uint64_t total_windows = 0;
  int n_own = 0, in_use = 0;
  for (int s = 0; s < G; ++s) {
    for (int y = 0; y < 4; ++y) bases[s] += counters[(size_t)s * 84 + y];
    is_own[s] = bases[s] >= st.min_bases;
    float* V = out->V.data() + (size_t)s * 84;
    if (is_own[s]) {
      long long n84[84];
      for (int y = 0; y < 84; ++y) n84[y] = (long long)counters[(size_t)s * 84 + y];
      BackgroundModel::modelOf(n84, bg.getOrder(), Global::bgModelAlpha, Global::interpolateBG, V);
    } else {
      std::copy(global_V, global_V + 84, V);
    }
    total_windows += windows[s];
    if (windows[s]) {
      ++in_use;
      n_own += is_own[s];
    }
  }
  if (total_windows == 0) Global::exitWithError("--stratified-background: the counted input holds no window of valid bases");
  lap("models");

  std::cout << "stratified background: " << G << " GC bin" << (G == 1 ? "" : "s") << ", " << in_use << " in use, " << n_own
            << " with a model of their own (at least " << st.min_bases << " bases), " << total_windows << " windows" << std::endl;
  if (pengk_host::rank() != 0) return;
  if (st.report_path) {
    std::string o = "stratum\tgc_lo\tgc_hi\tinput_sequences\tinput_windows\tmodel_bases\tmodel_used\tp_A\tp_C\tp_G\tp_T\n";
    char line[320];
    for (int s = 0; s < G; ++s) {
      const float* V = out->V.data() + (size_t)s * 84;
      snprintf(line, sizeof line, "%d\t%.3f\t%.3f\t%llu\t%llu\t%llu\t%s\t%.6f\t%.6f\t%.6f\t%.6f\n", s, (double)s / G, (double)(s + 1) / G,
               (unsigned long long)hist[s], (unsigned long long)windows[s], (unsigned long long)bases[s], is_own[s] ? "own" : "global",
               (double)V[0], (double)V[1], (double)V[2], (double)V[3]);
      o += line;
    }
    write_or_die(st.report_path, o.data(), o.size(), "--stratified-report");
  }
  if (const char* dir = std::getenv("PENGK_DUMP_TABLES")) {  // test hook: beside what BasePattern leaves there
    const std::string d(dir);
    write_or_die(d + "/strata_V.f32", out->V.data(), out->V.size() * sizeof(float), "PENGK_DUMP_TABLES");
    write_or_die(d + "/strata_windows.u64", out->windows.data(), out->windows.size() * sizeof(uint64_t), "PENGK_DUMP_TABLES");
  }
}
