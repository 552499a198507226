// motif_strata -- --stratified-background: a GC-stratified null for the k-mer sweep (include/pengk.h,
// "a GC-stratified null for the sweep").  The sequences of the counted input and of the model's source set are put into
// GC bins (pengk_seq_strata), every bin gets a background model of its own from the source set's sequences of that bin
// (pengk_strata_bg_count, BackgroundModel::modelOf with the run's order, alpha and interpolation), and the sweep scores a
// k-mer against the mean of the bins' Markov probabilities weighted by the windows the counted input holds in each
// (pengk_pattern_stats_strata).  This project's own definitions, not promised to give HOMER's numbers.
#ifndef PENGK_HOST_MOTIF_STRATA_H_
#define PENGK_HOST_MOTIF_STRATA_H_

#include <string>
#include <vector>

#include "motif_score.h"
#include "shared/BackgroundModel.h"

struct StratifiedSettings {
  int gc_bins = 10;                      // --stratified-gc-bins: 1 .. 16
  unsigned long long min_bases = 10000;  // --stratified-min-bases: a stratum with fewer model bases takes the global model
  const char* report_path = nullptr;     // --stratified-report
};

struct StratifiedNull {
  int G = 0;
  std::vector<float> V;           // G x 84: the stratum's own model, or the global one
  std::vector<uint64_t> windows;  // G: the W-windows of valid bases the counted set holds in the stratum, over all ranks
};

// Builds the null.  Counted set: this rank's records of `in` -- the subset `training` when given (--holdout) -- whose strata
// follow from the sequences as they are and whose windows are taken behind the validity words d_valid when given (the
// low-complexity mask).  Source set: `model_set` when it is another set than the input (--background-sequences), else all
// of `in` as it is.  Counters and windows are summed over the ranks; a stratum whose order-0 counters sum below
// st.min_bases takes bg's V.  Rank 0 writes the report and one stdout line.  Ends the program when the counted set holds
// no window.  Collective in a multi-rank run.
void build_stratified_null(const ScanInput& in, const uint32_t* d_valid, const ScanSubset* training, SequenceSet* model_set, int W,
                           BackgroundModel& bg, const StratifiedSettings& st, StratifiedNull* out);

namespace pengk_host {
// from now on BasePattern sweeps against this null (every round of --erase keeps round 1's); nullptr ends that
void set_stratified_null(const StratifiedNull* null);
const StratifiedNull* stratified_null();
}  // namespace pengk_host

#endif
