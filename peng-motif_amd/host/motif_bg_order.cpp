#include "motif_bg_order.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <string>

#include "Global.h"
#include "device.h"

namespace {
const HighOrderNull* g_null = nullptr;

size_t at(int k) { return (size_t)(((1u << (2 * (k + 1))) - 4u) / 3u); }  // 0, 4, 20, 84, 340, 1364, 5460
}  // namespace

namespace pengk_host {
void set_high_order_null(const HighOrderNull* null) { g_null = null; }
const HighOrderNull* high_order_null() { return g_null; }
}  // namespace pengk_host

void build_high_order_null(const ScanInput& in, SequenceSet* model_set, const HighOrderSettings& hs, HighOrderNull* out) {
  using pengk_host::check;
  using pengk_host::DeviceBuffer;
  pengk_host::Lap lap("  high-order background: ");
  pengk_ctx* ctx = pengk_host::context();
  const int K = hs.order;

  // the source set: another file's sequences in a scan layout of their own, else the input's
  std::unique_ptr<ScanInput> own;
  if (model_set) {
    own.reset(new ScanInput);
    build_scan_input(*model_set, own.get());
  }
  const ScanInput& src = own ? *own : in;

  const size_t N = at(K + 1);
  DeviceBuffer<uint64_t> d_bg(N);
  check(pengk_memset(ctx, d_bg.get(), 0, N * sizeof(uint64_t)), "pengk_memset");
  check(pengk_bg_count_order(ctx, src.d_words.get(), src.d_valid.get(), src.d_offs.get(), src.d_lens.get(), src.n_local, K, d_bg.get()),
        "pengk_bg_count_order");
  std::vector<uint64_t> n(N);
  d_bg.download(n.data(), N);
  if (pengk_host::world() > 1) check(pengk_comm_host_allreduce_u64(n.data(), N), "pengk_comm_host_allreduce_u64");
  lap("counters");

  uint64_t bases = 0;
  for (int y = 0; y < 4; ++y) bases += n[y];
  if (bases == 0) Global::exitWithError("--high-order-background: the background set holds no valid base");
  float alpha[6];
  for (int k = 0; k <= K; ++k) alpha[k] = k <= 2 ? Global::bgModelAlpha[k] : hs.alpha;
  out->K = K;
  out->V.assign(N, 0.0f);
  check(pengk_bg_model_order(n.data(), K, alpha, Global::interpolateBG ? 1 : 0, out->V.data()), "pengk_bg_model_order");
  lap("model");

  // the contexts of order k are the k-mers: the counters of order k - 1 (order 0 has one context, every base)
  std::vector<std::vector<uint64_t>> contexts(K + 1);
  contexts[0].assign(1, bases);
  for (int k = 1; k <= K; ++k) contexts[k].assign(n.begin() + at(k - 1), n.begin() + at(k));
  auto seen = [](const std::vector<uint64_t>& c) { return (size_t)std::count_if(c.begin(), c.end(), [](uint64_t v) { return v != 0; }); };
  char line[320];
  snprintf(line, sizeof line, "high-order background: order %d, alpha %g, %llu model bases, %zu of %zu contexts seen", K, (double)hs.alpha,
           (unsigned long long)bases, seen(contexts[K]), contexts[K].size());
  std::cout << line << std::endl;
  if (pengk_host::rank() != 0 || !hs.report_path) return;
  std::string o = "order\tcontexts\tcontexts_seen\tmin_count\tmedian_count\n";
  for (int k = 0; k <= K; ++k) {
    std::vector<uint64_t> c = contexts[k];
    std::sort(c.begin(), c.end());
    snprintf(line, sizeof line, "%d\t%zu\t%zu\t%llu\t%llu\n", k, c.size(), seen(c), (unsigned long long)c.front(),
             (unsigned long long)c[(c.size() - 1) / 2]);
    o += line;
  }
  FILE* f = fopen(hs.report_path, "wb");
  const bool ok = f && fwrite(o.data(), 1, o.size(), f) == o.size();
  if (!f || (fclose(f) != 0) || !ok) {
    std::cerr << "Error: --high-order-report: cannot write " << hs.report_path << std::endl;
    exit(1);
  }
}
