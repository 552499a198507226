// motif_erase -- --erase: after a search, the sites of the motifs it reported are masked on the device and what is left
// is searched again, as MEME, STREME and HOMER do.  One strong factor otherwise fills the --max-optimized-patterns places
// with shifted pieces of its own site (include/pengk.h, "erasing sites and packing on the device").
#ifndef PENGK_HOST_MOTIF_ERASE_H_
#define PENGK_HOST_MOTIF_ERASE_H_

#include <string>
#include <vector>

#include "motif_score.h"
#include "peng.h"

// Round 1 has run: `result` holds its motifs (after filter_redundancy), peng.last_seeds / last_windows its figures.
// Up to `rounds` further rounds: the previous round's motifs -> integer log-odds and thresholds at `pvalue` (as --sites)
// -> pengk_mask_sites over the current validity words of `in` -> pengk_pack_scan -> peng.process on the masked stream
// (pengk_host::override_packed_input) with the same parameters and background model.  A later-round motif that the
// redundancy filter would drop against an earlier one is dropped; what stays is appended to `result`.  No further round
// when the previous one reported no motif or erased no base.  `path`: the report, one line per round and motif (rank 0).
// initial_valid: the validity words round 1 was searched on when they are not the input's own (--mask-low-complexity: what
// that mask took stays out of every round).
// subset (--holdout): the sequences of `in` that are masked, packed and searched -- the training share -- in place of all of
// them; the validity words of the others stay zero.
// Collective in a multi-rank run: every rank masks and packs its own records, the counts are summed as in round 1.
void run_erase_rounds(Peng& peng, PengParameters& params, std::vector<IUPACPattern*>& result, SequenceSet& set,
                      const ScanInput& in, BackgroundModel& bg, bool both_strands, double pvalue, int rounds,
                      float merge_bit_factor_threshold, const std::string& path, const uint32_t* initial_valid = nullptr,
                      const ScanSubset* subset = nullptr);

#endif
