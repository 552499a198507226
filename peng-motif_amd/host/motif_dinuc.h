// motif_dinuc -- --dinuc: a first-order model of every found motif from its best sites, and what it gains over the
// zeroth-order model from the same sites.  The first step beyond the PWM: the reference's wrapper
// hands the PWMs to BaMMmotif so that higher-order models can be learned from them (include/pengk.h, "first-order motif
// models").
#ifndef PENGK_HOST_MOTIF_DINUC_H_
#define PENGK_HOST_MOTIF_DINUC_H_

#include <string>
#include <vector>

#include "iupac_pattern.h"
#include "motif_score.h"
#include "shared/BackgroundModel.h"
#include "shared/SequenceSet.h"

struct DinucSettings {
  double pvalue = 1e-4;  // --dinuc-pvalue: a best site counts at this p-value or below
  int flank = 0;         // --dinuc-flank: columns modelled on either side (clamped per motif to PENGK_MAX_MOTIF_LEN)
  double alpha = 20.0;   // --dinuc-alpha: the weight of the zeroth-order model in the interpolated conditionals
  int bg_order = 2;      // --bg-model-order: the negatives' sampling model; >= 1: the first-order background is V[1]
  uint64_t seed = 1;     // --score-seed
  bool shuffled = false; // --score-negatives shuffled
};

// Models pats (in their order: the MEME file's) over this rank's records of `set`; the counts and the histograms are
// summed over the ranks, rank 0 writes.  Per motif: the threshold at ds.pvalue of its found PWM's log-odds, the best site
// per sequence (pengk_motif_best_sites), the single and pair profiles with ds.flank, pengk_dinuc_model; then two
// pengk_motif_scan_dinuc passes (D0, D1) over the input and over the negatives of score_motifs (build_negatives), their
// histograms and AUCs.  report_path: the TSV; models_path: the models file, or empty.  shared: those negatives, already
// built (see score_motifs), else NULL.  Collective in a multi-rank run.
void write_motif_dinuc(const std::vector<IUPACPattern*>& pats, SequenceSet& set, const ScanInput& in, BackgroundModel& bg,
                       bool both_strands, const DinucSettings& ds, const std::string& report_path,
                       const std::string& models_path, Negatives* shared = nullptr);

#endif
