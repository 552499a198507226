// motif_spacing -- --spacing: which pairs of found motifs occur in the same sequences more often than chance, and
// whether they keep a fixed distance and orientation there.  What MEME-suite's SpaMo would add
// after peng_motif on ChIP-seq peaks, on the device (include/pengk.h, "motif pair spacing").
#ifndef PENGK_HOST_MOTIF_SPACING_H_
#define PENGK_HOST_MOTIF_SPACING_H_

#include <string>
#include <vector>

#include "iupac_pattern.h"
#include "motif_score.h"
#include "shared/BackgroundModel.h"
#include "shared/SequenceSet.h"

// Writes the pair test of the first max_motifs of pats (in their order: the MEME file's) over this rank's records of
// `set` (scan layout `in`) to `path`: per motif the best window strand of every considered sequence whose score reaches
// the threshold at p-value `pvalue` under the order-0 background V[0] of bg; per pair a binomial test of the sequences
// that hold both and of the most surprising (orientation, gap <= max_gap) among those where the two do not overlap.
// The histograms are summed over the ranks; rank 0 writes.  Collective in a multi-rank run.
void write_motif_spacing(const std::vector<IUPACPattern*>& pats, SequenceSet& set, const ScanInput& in, BackgroundModel& bg,
                         bool both_strands, double pvalue, int max_gap, int max_motifs, const std::string& path);

#endif
