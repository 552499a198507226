// motif_score -- the second user-facing step of the reference's wrapper scripts/shoot_peng.py (which runs BaMMmotif2's
// FDR tool and an R script over peng_motif's output): every motif scored by how well it separates the input sequences
// from as many sequences sampled from the background model, on the device (include/pengk.h, "motif scoring").
// zoops_score / occur keep the wrapper's field names; the metric is this project's own.
#ifndef PENGK_HOST_MOTIF_SCORE_H_
#define PENGK_HOST_MOTIF_SCORE_H_

#include <cstdint>
#include <vector>

#include "iupac_pattern.h"
#include "shared/BackgroundModel.h"
#include "shared/SequenceSet.h"

struct MotifScore {
  double zoops_score = 0.0;  // AUC of the best window scores, input against sampled sequences
  double occur = 0.0;        // share of input sequences with a site, estimated at 1 % false positives
};

// Scores pats (in their order) over this rank's records of `set` and the negatives of their global indices; the
// histograms are summed over the ranks, so every rank gets the scores of the whole input.  K: the order of the
// sampling model (--bg-model-order), V from bg.  Collective in a multi-rank run.
std::vector<MotifScore> score_motifs(const std::vector<IUPACPattern*>& pats, SequenceSet& set, BackgroundModel& bg, int K,
                                     bool both_strands, uint64_t seed);

#endif
