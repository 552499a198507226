// motif_bg_order -- --high-order-background K: a Markov null of order 3 .. 5 for the k-mer sweep (INTEGRATION.md 7u;
// include/pengk.h, "a Markov null of order 3 .. 5 for the sweep").  The (k+1)-mers of orders 0 .. K of the model's source set
// are counted on the device (pengk_bg_count_order), the model is calculateV continued to order K (pengk_bg_model_order: the
// run's alpha and interpolation at orders 0 .. 2, --high-order-alpha above), and the sweep puts its probabilities into the
// slot of the run's order (pengk_pattern_stats_order).  This project's own definitions.
#ifndef PENGK_HOST_MOTIF_BG_ORDER_H_
#define PENGK_HOST_MOTIF_BG_ORDER_H_

#include <vector>

#include "motif_score.h"

struct HighOrderSettings {
  int order = 0;                      // --high-order-background: 3 .. 5
  float alpha = 1.0f;                 // --high-order-alpha: orders 3 .. K
  const char* report_path = nullptr;  // --high-order-report
};

struct HighOrderNull {
  int K = 0;
  std::vector<float> V;  // orders 0 .. K back to back, (4^(K+2) - 4) / 3 floats
};

// Builds the null.  Source set: `model_set` when it is another set than the input (--background-sequences), else all of
// `in` as it was read -- no mask, no hold-out.  The counters are summed over the ranks.  Rank 0 writes the report and one
// stdout line.  Ends the program when the source set holds no valid base.  Collective in a multi-rank run.
void build_high_order_null(const ScanInput& in, SequenceSet* model_set, const HighOrderSettings& hs, HighOrderNull* out);

namespace pengk_host {
// from now on BasePattern sweeps against this null (every round of --erase keeps round 1's); nullptr ends that
void set_high_order_null(const HighOrderNull* null);
const HighOrderNull* high_order_null();
}  // namespace pengk_host

#endif
