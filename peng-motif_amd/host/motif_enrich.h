// motif_enrich -- --enrich: which motifs of a MEME database are enriched in the input against its negatives (the
// question SEA and AME answer in MEME-suite; the definitions are this project's own).  Unlike
// --compare it reads the sequences, and it never looks at the found motifs: a factor whose motif the de-novo search did
// not report is found all the same (include/pengk.h, "database enrichment").
#ifndef PENGK_HOST_MOTIF_ENRICH_H_
#define PENGK_HOST_MOTIF_ENRICH_H_

#include <string>
#include <vector>

#include "meme_db.h"
#include "motif_score.h"
#include "shared/BackgroundModel.h"
#include "shared/SequenceSet.h"

struct EnrichSettings {
  double pvalue = 1e-3;  // --enrich-pvalue: the lowest site threshold tried has this tail p-value or less
  double evalue = 10.0;  // --enrich-evalue: only motifs with an E-value at or below it are written
};

// The log-odds of one database motif against bg0, into S (w x 4): row r becomes p_a = (r_a / sum(r) + 0.01 bg0_a) / 1.01
// in double (sum = ((r_0 + r_1) + r_2) + r_3), rounded to float, then log_odds(p_a, bg0_a) of motif_score.h.
void enrich_log_odds(const MemeMotif& t, const float* bg0, int32_t* S);

// Tests db (in its order) over this rank's records (`in`) and over `neg`, the negatives of --score-motifs
// (build_negatives): per motif the threshold at es.pvalue, pengk_motif_enrich over both sets -- nothing of size motifs x
// sequences is allocated --, the histograms and scored counts summed over the ranks, pengk_enrich_summary, the E-value
// and Benjamini-Hochberg q-value over the database; rank 0 writes the TSV.  Collective in a multi-rank run.
void write_motif_enrich(const std::vector<MemeMotif>& db, const ScanInput& in, Negatives& neg, BackgroundModel& bg,
                        bool both_strands, const EnrichSettings& es, const std::string& path);

#endif
