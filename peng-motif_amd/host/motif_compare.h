// motif_compare -- --compare: which known motif is this?  The found motifs against a MEME-format database, with a p-value
// per match from a null built over the whole database (include/pengk.h, "motif comparison").  Stands in
// for a Tomtom run on the MEME output; the definitions are this project's own and the numbers are not Tomtom's.
#ifndef PENGK_HOST_MOTIF_COMPARE_H_
#define PENGK_HOST_MOTIF_COMPARE_H_

#include <string>
#include <vector>

#include "iupac_pattern.h"
#include "meme_db.h"

struct CompareSettings {
  double evalue = 1.0;  // --compare-evalue: only matches with an E-value at or below it are written
  int min_overlap = 5;  // --compare-min-overlap: columns an alignment must span (at most the narrower motif's width)
};

// Compares pats (in their order: the MEME file's) with db and writes the TSV: per motif its matches by p_value ascending,
// then database order.  Needs neither the sequences nor their scan layout; in a multi-rank run rank 0 alone calls it.
// PENGK_COMPARE_QUERIES=FILE (diagnostic): the quantised query matrices the run used -- per motif a line "index width
// iupac", then its rows (the PWMs of the MEME / JSON files are rounded to 8 decimals and do not give them back).
void write_motif_compare(const std::vector<IUPACPattern*>& pats, const std::vector<MemeMotif>& db, bool both_strands,
                         const CompareSettings& cs, const std::string& path);

#endif
