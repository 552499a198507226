// motif_centrality -- --centrality: which found motifs sit at the centres of the input sequences.
// What MEME-suite's CentriMo would add after peng_motif on ChIP-seq peaks, on the device (include/pengk.h, "central
// enrichment").
#ifndef PENGK_HOST_MOTIF_CENTRALITY_H_
#define PENGK_HOST_MOTIF_CENTRALITY_H_

#include <string>
#include <vector>

#include "iupac_pattern.h"
#include "motif_score.h"
#include "shared/BackgroundModel.h"
#include "shared/SequenceSet.h"

// Writes the central-enrichment test of pats (in their order: the MEME file's) over this rank's records of `set` (scan
// layout `in`) to `path`: per motif the best window strand of every sequence of 1..PENGK_CENTRALITY_MAX_LEN bases whose
// score reaches the threshold at p-value `pvalue` under the order-0 background V[0] of bg, its offset from the centre,
// and a binomial test of the window around the centre that holds the most surprising share of them.  The histograms
// are summed over the ranks; rank 0 writes.  Collective in a multi-rank run.
void write_motif_centrality(const std::vector<IUPACPattern*>& pats, SequenceSet& set, const ScanInput& in, BackgroundModel& bg,
                            bool both_strands, double pvalue, const std::string& path);

#endif
