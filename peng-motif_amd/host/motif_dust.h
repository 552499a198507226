// motif_dust -- --mask-low-complexity: poly-A tracts, (CA)n and their like are masked on the device before round 1 counts
// anything, as dustmasker / sdust / RepeatMasker's simple-repeat pass are run in front of other discovery tools.  Such
// words exceed an order-2 expectation more than any motif and otherwise take the seed places and the
// --max-optimized-patterns places (include/pengk.h, "masking low-complexity stretches").
#ifndef PENGK_HOST_MOTIF_DUST_H_
#define PENGK_HOST_MOTIF_DUST_H_

#include <memory>
#include <string>
#include <vector>

#include "motif_score.h"

// One masked set in the count layout: what pengk_host::override_packed_input / override_control_input hand to BasePattern.
struct MaskedSet {
  pengk_host::DeviceBuffer<uint32_t> d_valid;            // the scan layout's validity words behind the mask
  pengk_host::DeviceBuffer<uint64_t> d_words, d_items;   // the count layout of what is left
  pengk_host::PackedInput packed;
  unsigned long long bases_masked = 0, bases_valid = 0, seqs_touched = 0, seqs = 0;  // summed over the ranks
};

struct LowComplexityMask {
  MaskedSet input;
  bool attached = false;                   // a base of the input was masked (on any rank): round 1 counts input.packed
  std::unique_ptr<ScanInput> control_scan; // --discriminative: the control set, masked by the same rule
  MaskedSet control;
  bool control_attached = false;
  // the input's validity words that --erase starts from (nullptr: the input's own)
  const uint32_t* erase_valid() const { return attached ? input.d_valid.get() : nullptr; }
};

// pengk_mask_low_complexity over `scan` (the input's scan layout) at `threshold`, then pengk_pack_scan_sizes /
// pengk_pack_scan of the masked validity at pattern length W; one stdout line.  control != nullptr: the same for the
// control set, whose scan layout is built here.  report_path != nullptr: the BED-like TSV of the input's masked runs
// (rank 0 writes; the other ranks' lines arrive in rank order, with global sequence indices).  Attaches the results
// (override_packed_input / override_control_input) unless nothing was masked; the caller ends that.
// Collective in a multi-rank run.
void mask_low_complexity(SequenceSet& input, const ScanInput& scan, SequenceSet* control, int W, int threshold,
                         const char* report_path, LowComplexityMask* out);

// the maximal runs of set bits of a ^ b per sequence as "index<TAB>start<TAB>end\n" lines (half-open, in order); index =
// index0 + the sequence's place.  offs / lens: the scan layout's (offs in bases, a multiple of 32 each).  Plain host code.
std::string masked_runs_tsv(const uint32_t* a, const uint32_t* b, const int64_t* offs, const uint32_t* lens, size_t n_seq,
                            unsigned long long index0);

#endif
