// motif_dyads -- --dyads: pairs of trinucleotides a fixed number of unconstrained bases apart, counted on the device over
// what round 1 counts, tested against the product of the triplet frequencies and folded into families (INTEGRATION.md 7q;
// include/pengk.h, "spaced dyads").  The bipartite sites of dimeric factors, which no contiguous word of the k-mer table
// holds.  This project's own definitions, not RSAT's numbers.
#ifndef PENGK_HOST_MOTIF_DYADS_H_
#define PENGK_HOST_MOTIF_DYADS_H_

#include <string>

#include "motif_refine.h"
#include "motif_score.h"
#include "shared/BackgroundModel.h"
#include "shared/SequenceSet.h"

struct DyadSettings {
  int max_gap = 20;                  // --dyads-max-gap: the largest spacer counted, 0 .. PENGK_DYAD_MAX_GAP
  double evalue = 0.01;              // --dyads-evalue: a dyad is reported at this E-value or below
  unsigned long long min_count = 5;  // --dyads-min-count
  int top = 5;                       // --dyads-top: family heads refined into motifs
  double pvalue = 1e-3;              // --dyads-pvalue: site threshold of the refinement (an exact six-letter match has
                                     // p = 4^-6 = 2.4e-4: at --refine's 1e-4 the first round would find no site)
};

// the dyad as a string over ACGTn of length 6 + gap
std::string dyad_string(uint32_t key, uint32_t gap);

// pengk_dyad_count over this rank's records of `in` -- behind the validity words d_valid when given (the low-complexity
// mask), over the subset `training` when given (--holdout) --, the tables summed over the ranks, pengk_dyad_summary, and
// the TSV at `path` (rank 0; one stdout line).  motifs_path: the first `top` family heads as matrices of width 6 + gap
// (0.85 on a letter, 0.05 elsewhere; spacer columns the order-0 background) through the rounds of --refine
// (refine_matrices, with rs.pvalue = ds.pvalue) over the whole input, written as MEME under the dyad strings.  Collective
// in a multi-rank run.
void write_dyads(SequenceSet& set, const ScanInput& in, const uint32_t* d_valid, const ScanSubset* training, BackgroundModel& bg,
                 bool both_strands, const DyadSettings& ds, RefineSettings rs, const char* path, const char* motifs_path);

#endif
