// motif_refine -- --refine: the found motifs re-estimated and extended from their sites.  The step
// MEME, HOMER and STREME end with, and BaMMmotif2 runs downstream of peng_motif: back to the sequences, which see the
// flanks that the k-mer table cannot (include/pengk.h, "motif refinement").
#ifndef PENGK_HOST_MOTIF_REFINE_H_
#define PENGK_HOST_MOTIF_REFINE_H_

#include <string>
#include <vector>

#include "iupac_pattern.h"
#include "motif_score.h"
#include "shared/BackgroundModel.h"
#include "shared/SequenceSet.h"

struct RefineSettings {
  double pvalue = 1e-4;  // --refine-pvalue: a best site counts at this p-value or below
  int flank = 8;         // --refine-flank: columns looked at on either side (clamped per motif to PENGK_MAX_MOTIF_LEN)
  int iterations = 3;    // --refine-iterations
  double min_ic = 0.25;  // --refine-min-ic: bits the outermost kept columns need
};

// Refines pats (in their order: the MEME file's; the patterns themselves stay as they are) over this rank's records of
// `set` (scan layout `in`) and writes them to `path` as a MEME file.  Per round and motif: integer log-odds and the
// threshold at `pvalue` under the order-0 background V[0] of bg, the best window strand of every sequence, the base
// counts of the columns [-F, w + F) of those at or above the threshold, summed over the ranks, and from them the new
// matrix and its kept columns (pengk_profile_refine).  A motif stops when a round repeats the kept range and its counts,
// finds no site or keeps no column.  Rank 0 writes.  Collective in a multi-rank run.
void write_refined_motifs(const std::vector<IUPACPattern*>& pats, SequenceSet& set, const ScanInput& in, BackgroundModel& bg,
                          bool both_strands, const RefineSettings& rs, const std::string& path);

#endif
