// motif_positional -- --positional: the words of 4..7 letters counted per position bin on the device over what round 1
// counts (overlapping repeats of a word once), each word's count in a bin tested against its count everywhere and the
// bin's share of all words, shifted neighbours folded into families (include/pengk.h, "positional
// words").  Words that keep one position whether or not they are over-represented.  This project's own definitions, not
// RSAT's numbers.
#ifndef PENGK_HOST_MOTIF_POSITIONAL_H_
#define PENGK_HOST_MOTIF_POSITIONAL_H_

#include <string>

#include "motif_score.h"

struct PositionalSettings {
  int width = 6;                     // --positional-width: PENGK_POSITION_MIN_K .. PENGK_POSITION_MAX_K
  int anchor = 2;                    // --positional-anchor: 0 start, 1 end, 2 center
  int bin_size = 10;                 // --positional-bin-size
  int bins = 20;                     // --positional-bins: 1 .. PENGK_POSITION_MAX_BINS
  double evalue = 0.01;              // --positional-evalue: a word is reported at this E-value or below
  unsigned long long min_count = 5;  // --positional-min-count
  bool composition_null = false;     // --positional-null composition: pengk_position_pairs and pengk_position_summary_null
};

// the word as letters, first base first
std::string positional_word_string(uint32_t key, int width);

// pengk_position_count over this rank's records of `in` -- behind the validity words d_valid when given (the low-complexity
// mask), over the subset `training` when given (--holdout) --, the table summed over the ranks, pengk_position_summary, and
// the TSV at `path` (rank 0; one stdout line).  Under the composition null the pair table is counted over the same share
// behind the same validity, summed likewise, and the TSV gets the column flat_expected behind expected.
// Collective in a multi-rank run.
void write_positional(const ScanInput& in, const uint32_t* d_valid, const ScanSubset* training, bool both_strands,
                      const PositionalSettings& ps, const char* path);

#endif
