// motif_holdout -- --holdout: a share of the input is set aside on the device before anything is counted, the motifs are
// found on the rest, and every motif is tested on the share it never saw, as STREME reports its p-values from the 10 % it
// holds out.  Every other significance this program prints is computed on the sequences the motif was fitted to
// (include/pengk.h, "a hold-out share").
#ifndef PENGK_HOST_MOTIF_HOLDOUT_H_
#define PENGK_HOST_MOTIF_HOLDOUT_H_

#include <memory>
#include <string>
#include <vector>

#include "motif_score.h"

// The two shares of one set (this rank's records): [0] training, [1] hold-out.
struct SplitSet {
  pengk_host::DeviceBuffer<int64_t> d_offs[2];
  pengk_host::DeviceBuffer<uint32_t> d_lens[2], d_index[2];
  size_t n[2] = {0, 0};
  ScanSubset share(int c) const {
    ScanSubset s;
    s.d_offs = d_offs[c].get();
    s.d_lens = d_lens[c].get();
    s.n = n[c];
    return s;
  }
};

struct HoldoutSettings {
  double fraction = 0.1;
  unsigned long long threshold = 0;  // (uint64_t)(fraction * 2^32)
  unsigned long long seed = 1;
  double pvalue = 1e-3;
};

struct Holdout {
  SplitSet input;
  pengk_host::DeviceBuffer<uint64_t> d_words, d_items;  // the training share in the count layout
  pengk_host::PackedInput packed;
  bool attached = false;
  std::unique_ptr<ScanInput> control_scan;              // --discriminative: the control set, split by the same rule
  SplitSet control;
  pengk_host::DeviceBuffer<uint64_t> d_cwords, d_citems;
  pengk_host::PackedInput control_packed;
  bool control_attached = false;
  unsigned long long n_train = 0, n_hold = 0;           // the input's two shares, summed over the ranks
};

// pengk_split_sequences over `scan` (the input's scan layout; global indices from input.getLocalBase() on), then
// pengk_pack_scan_sizes / pengk_pack_scan of the training share at pattern length W under the validity words `valid`
// (nullptr: the input's own; --mask-low-complexity: what the mask left); one stdout line.  control != nullptr
// (--discriminative): the same for the control set, whose scan layout is built here, split over its own indices, under
// control_valid.  Attaches the results (override_packed_input / override_control_input) and makes the input count as its
// training sequences (override_sequence_count); the caller ends all three.  Collective in a multi-rank run.
void split_holdout(SequenceSet& input, const ScanInput& scan, const uint32_t* valid, SequenceSet* control,
                   const uint32_t* control_valid, int W, const HoldoutSettings& hs, Holdout* out);

// The report: every motif of pats (in their order) scored on the four sets -- training and hold-out share of the input and
// of the negatives (`neg`: sampled or shuffled ones share the input's two pairs; a control set is split here, by its
// sequences' indices in the control file) -- with pengk_motif_enrich from the score threshold of hs.pvalue upward, the
// histograms summed over the ranks, pengk_holdout_summary, one line per motif (rank 0 writes).  Collective.
void write_motif_holdout(const std::vector<IUPACPattern*>& pats, const ScanInput& in, const Holdout& ho, Negatives& neg,
                         SequenceSet* control, BackgroundModel& bg, bool both_strands, const HoldoutSettings& hs,
                         const std::string& path);

#endif
