#include "motif_match.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <vector>

#include "Global.h"
#include "device.h"

namespace {
constexpr int NS = 256;  // strata: 16 length bins x up to 16 GC bins

void write_or_die(const std::string& path, const void* p, size_t bytes, const char* what) {
  FILE* f = fopen(path.c_str(), "wb");
  const bool ok = f && fwrite(p, 1, bytes, f) == bytes;
  if (!f || (fclose(f) != 0) || !ok) {
    std::cerr << "Error: " << what << ": cannot write " << path << std::endl;
    exit(1);
  }
}

// the smallest length of half-octave h = 2 floor(log2 L) + (the bit of L below its top bit)
unsigned long long first_length(int h) { return h >= 2 ? (unsigned long long)(2 + (h & 1)) << ((h >> 1) - 1) : 1ull; }

std::string render_report(const uint64_t* h_in, const uint64_t* h_ctrl, const uint64_t* quota, int G, bool use_length) {
  std::string o = "length_min\tlength_max\tgc_min\tgc_max\tinput\tcontrol\tkept\n";
  char line[256];
  for (int s = 0; s < NS; ++s) {
    if (!h_in[s] && !h_ctrl[s]) continue;
    const int lb = s / G, g = s % G;
    const unsigned long long lo = use_length && lb ? first_length(lb + 10) : 1ull;
    std::string hi = "inf";
    if (use_length && lb < 15) hi = std::to_string(first_length(lb + 11) - 1);
    snprintf(line, sizeof line, "%llu\t%s\t%.3f\t%.3f\t%llu\t%llu\t%llu\n", lo, hi.c_str(), (double)g / G, (double)(g + 1) / G,
             (unsigned long long)h_in[s], (unsigned long long)h_ctrl[s], (unsigned long long)quota[s]);
    o += line;
  }
  return o;
}
}  // namespace

void build_control_negatives(SequenceSet& control, const ScanInput& in, const MatchSettings& ms, Negatives* out) {
  using pengk_host::check;
  using pengk_host::DeviceBuffer;
  pengk_host::Lap lap("  control: ");
  pengk_ctx* ctx = pengk_host::context();
  const int world = pengk_host::world(), rank = pengk_host::rank();
  out->shuffled = false;
  out->control.reset(new ScanInput);
  build_scan_input(control, out->control.get());
  const ScanInput& ctl = *out->control;
  const size_t n_ctrl = ctl.n_local;
  const bool match = ms.gc || ms.length;
  const char* mode = ms.gc && ms.length ? "gc,length" : ms.gc ? "gc" : ms.length ? "length" : "none";
  const char* dump_dir = rank == 0 ? std::getenv("PENGK_DUMP_TABLES") : nullptr;

  if (!match) {  // the whole control: no stratum kernel runs
    uint64_t total = n_ctrl;
    if (world > 1) check(pengk_comm_host_allreduce_u64(&total, 1), "pengk_comm_host_allreduce_u64");
    if (total == 0) Global::exitWithError("--score-negatives control: the control set holds no sequence");
    std::cout << "control negatives: matched by none: kept " << total << " of " << total << " control sequences" << std::endl;
    return;
  }

  // strata of the input and of the control, their histograms side by side
  const int G = ms.gc ? ms.gc_bins : 1;
  DeviceBuffer<uint16_t> d_in_stratum(std::max<size_t>(in.n_local, 1)), d_stratum(std::max<size_t>(n_ctrl, 1));
  DeviceBuffer<uint64_t> d_hist(2 * NS);
  check(pengk_memset(ctx, d_hist.get(), 0, 2 * NS * sizeof(uint64_t)), "pengk_memset");
  check(pengk_seq_strata(ctx, in.d_words.get(), in.d_valid.get(), in.d_offs.get(), in.d_lens.get(), in.n_local, G,
                         ms.length ? 1 : 0, d_in_stratum.get(), d_hist.get()),
        "pengk_seq_strata");
  check(pengk_seq_strata(ctx, ctl.d_words.get(), ctl.d_valid.get(), ctl.d_offs.get(), ctl.d_lens.get(), n_ctrl, G,
                         ms.length ? 1 : 0, d_stratum.get(), d_hist.get() + NS),
        "pengk_seq_strata");
  std::vector<uint64_t> hist(2 * NS), rank0(NS, 0);
  d_hist.download(hist.data(), 2 * NS);
  lap("strata");
  if (world > 1) {
    // every rank's control histogram: the sequences of a stratum that the earlier ranks hold; then the sums
    std::vector<uint64_t> all((size_t)world * NS);
    check(pengk_comm_host_allgather(hist.data() + NS, all.data(), NS * sizeof(uint64_t)), "pengk_comm_host_allgather");
    for (int r = 0; r < rank; ++r)
      for (int s = 0; s < NS; ++s) rank0[s] += all[(size_t)r * NS + s];
    check(pengk_comm_host_allreduce_u64(hist.data(), hist.size()), "pengk_comm_host_allreduce_u64");
  }
  const uint64_t* h_in = hist.data();
  const uint64_t* h_ctrl = hist.data() + NS;
  std::vector<uint64_t> quota(NS, 0);
  uint64_t shortfall = 0;
  check(pengk_match_quotas(h_in, h_ctrl, ms.ratio, quota.data(), &shortfall), "pengk_match_quotas");
  uint64_t total_ctrl = 0, total_kept = 0, in_use = 0;
  for (int s = 0; s < NS; ++s) {
    total_ctrl += h_ctrl[s];
    total_kept += quota[s];
    in_use += h_in[s] ? 1 : 0;
  }
  if (total_kept == 0)
    Global::exitWithError("--score-negatives control: no control sequence matches the input (--control-match " + std::string(mode) +
                          "); try --control-match none");

  out->d_sel_offs.resize(std::max<size_t>(n_ctrl, 1));
  out->d_sel_lens.resize(std::max<size_t>(n_ctrl, 1));
  out->d_sel_index.resize(std::max<size_t>(n_ctrl, 1));
  const DeviceBuffer<uint32_t>& d_index = out->d_sel_index;
  uint64_t n_sel = 0;
  check(pengk_select_strata(ctx, d_stratum.get(), n_ctrl, h_ctrl, quota.data(), rank0.data(), ctl.d_offs.get(), ctl.d_lens.get(),
                            out->d_sel_offs.get(), out->d_sel_lens.get(), d_index.get(), &n_sel),
        "pengk_select_strata");
  out->selected = true;
  out->n_sel = (size_t)n_sel;
  lap("quotas + selection");

  std::cout << "control negatives: matched by " << mode << " (" << G << " GC bin" << (G == 1 ? "" : "s") << ", ratio " << ms.ratio
            << "): " << in_use << " strat" << (in_use == 1 ? "um" : "a") << " in use, kept " << total_kept << " of " << total_ctrl
            << " control sequences, shortfall " << shortfall << std::endl;
  if (rank != 0) return;
  if (!ms.report_path.empty()) {
    const std::string o = render_report(h_in, h_ctrl, quota.data(), G, ms.length);
    write_or_die(ms.report_path, o.data(), o.size(), "--control-match-report");
  }
  if (dump_dir) {  // test hook: the counts, the quotas and this rank's kept sequences (global indices)
    const std::string d(dump_dir);
    write_or_die(d + "/match_input.u64", h_in, NS * sizeof(uint64_t), "PENGK_DUMP_TABLES");
    write_or_die(d + "/match_control.u64", h_ctrl, NS * sizeof(uint64_t), "PENGK_DUMP_TABLES");
    write_or_die(d + "/match_quota.u64", quota.data(), NS * sizeof(uint64_t), "PENGK_DUMP_TABLES");
    std::vector<uint32_t> idx(std::max<size_t>(n_sel, 1));
    if (n_sel) d_index.download(idx.data(), n_sel);
    std::vector<uint64_t> kept(n_sel);
    for (size_t k = 0; k < n_sel; ++k) kept[k] = control.getLocalBase() + idx[k];
    write_or_die(d + "/match_kept.u64", kept.data(), kept.size() * sizeof(uint64_t), "PENGK_DUMP_TABLES");
  }
}
