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

// One motif as the rounds leave it.
struct RefinedMotif {
  std::vector<float> pwm;  // w x 4, the matrix of the next round
  int w = 0;
  int w0 = 0;               // the width it started with
  int left = 0, right = 0;  // columns gained on either side of the starting matrix (negative: trimmed)
  int rounds = 0;           // rounds that gave a matrix
  long long sites = 0;      // sequences with a site in the last of them
  bool active = true;
  bool have_prev = false;
  int prev_first = 0, prev_last = 0;  // the last round's kept range, in the starting matrix's columns
  std::vector<long long> prev_counts;
};
// The rounds described below from any starting matrices (start[m]: w x 4 probabilities, 1 <= w <= PENGK_MAX_MOTIF_LEN):
// what --refine runs on the found PWMs and --dyads-motifs on the family heads.  Collective in a multi-rank run.
std::vector<RefinedMotif> refine_matrices(const std::vector<std::vector<float>>& start, SequenceSet& set, const ScanInput& in,
                                          BackgroundModel& bg, bool both_strands, const RefineSettings& rs);
// ... and the MEME file of the result under the given motif names (the caller's rank 0 calls it)
void write_refined_meme(const std::vector<RefinedMotif>& mot, const std::vector<std::string>& names, const float* bg0,
                        const std::string& path);

// Refines pats (in their order: the MEME file's; the patterns themselves stay as they are) over this rank's records of
// `set` (scan layout `in`) and writes them to `path` as a MEME file.  Per round and motif: integer log-odds and the
// threshold at `pvalue` under the order-0 background V[0] of bg, the best window strand of every sequence, the base
// counts of the columns [-F, w + F) of those at or above the threshold, summed over the ranks, and from them the new
// matrix and its kept columns (pengk_profile_refine).  A motif stops when a round repeats the kept range and its counts,
// finds no site or keeps no column.  Rank 0 writes.  Collective in a multi-rank run.
void write_refined_motifs(const std::vector<IUPACPattern*>& pats, SequenceSet& set, const ScanInput& in, BackgroundModel& bg,
                          bool both_strands, const RefineSettings& rs, const std::string& path);

#endif
