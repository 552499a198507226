// motif_sites -- --sites: every occurrence of the found motifs in the input, with an exact p-value.
// What FIMO or BaMMmotif2's scanner would add after peng_motif, on the device (include/pengk.h, "motif sites").
#ifndef PENGK_HOST_MOTIF_SITES_H_
#define PENGK_HOST_MOTIF_SITES_H_

#include <string>
#include <vector>

#include "iupac_pattern.h"
#include "motif_score.h"
#include "shared/BackgroundModel.h"
#include "shared/SequenceSet.h"

// Writes the sites of pats (in their order: the MEME file's) over this rank's records of `set` (scan layout `in`) to
// `path`: every window strand whose score reaches the motif's threshold at p-value `pvalue` under the order-0
// background V[0] of bg.  Rank 0 writes; the other ranks send it their lines.  Collective in a multi-rank run.
// qvalues (--sites-qvalue): a q_value column, Benjamini-Hochberg over each motif's sites with all its
// scored window strands as the number of tests, from histograms summed over the ranks; qvalue_max > 0
// (--sites-qvalue-max): only the sites with a q-value at or below it.  Without qvalues the calls and the file are those
// of --sites alone.
void write_motif_sites(const std::vector<IUPACPattern*>& pats, SequenceSet& set, const ScanInput& in, BackgroundModel& bg,
                       bool both_strands, double pvalue, bool qvalues, double qvalue_max, const std::string& path);

#endif
