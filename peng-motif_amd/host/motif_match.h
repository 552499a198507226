// motif_match -- --score-negatives control: the sequences of the --background-sequences file as the negatives of
// --score-motifs, --dinuc and --enrich, drawn from that control in proportion to the input's GC content and length
// (include/pengk.h, "a control set matched to the input").  This project's own definitions; HOMER and
// BiasAway match their backgrounds the same way.
#ifndef PENGK_HOST_MOTIF_MATCH_H_
#define PENGK_HOST_MOTIF_MATCH_H_

#include <cstdint>
#include <string>

#include "motif_score.h"

struct MatchSettings {
  bool gc = true, length = true;  // --control-match; both false: the whole control, no stratum kernel runs
  int gc_bins = 10;               // --control-match-gc-bins
  uint64_t ratio = 1;             // --control-ratio
  std::string report_path;        // --control-match-report, or empty
};

// Builds the control's scan layout (this rank's records of `control`, which must still hold its byte codes), stratifies
// the input (`in`) and the control on the device, sums the histograms over the ranks, gathers the ranks' control
// histograms for the stable ranks of this shard, computes the quotas and selects.  out: the negatives in a layout of their
// own.  One line on stdout; the report; the counts, quotas and kept indices under PENGK_DUMP_TABLES.  No control sequence
// kept over all ranks ends the run with exit status 4.  Collective in a multi-rank run.
void build_control_negatives(SequenceSet& control, const ScanInput& in, const MatchSettings& ms, Negatives* out);

#endif
