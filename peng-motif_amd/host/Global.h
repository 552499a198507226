// Global -- command-line state of the peng_motif mirror (same static fields, flags, defaults and exit
// codes as the reference's src/Global.h / src/Global.cpp:77-314).
#ifndef PENGK_HOST_GLOBAL_H_
#define PENGK_HOST_GLOBAL_H_

#include <string>
#include <vector>

#include "meme_db.h"
#include "shared/SequenceSet.h"

enum class Strand { PLUS_STRAND, BOTH_STRANDS };

enum class OPTIMIZATION_SCORE { kLogPval = 0, kExpCounts = 1, MutualInformation };

const std::string VERSION_NUMBER("1.0.0");

class Global {
 public:
  static char* alphabetType;
  static char* outputFilename;               // -o  short MEME
  static char* jsonFilename;                 // -j  JSON
  static char* inputSequenceFilename;        // positional
  static char* backgroundSequenceFilename;   // --background-sequences
  static SequenceSet* inputSequenceSet;
  static SequenceSet* backgroundSequenceSet;

  static OPTIMIZATION_SCORE optScoreType;    // --optimization_score
  static float enrich_pseudocount_factor;    // --enrich_pseudocount_factor

  static int patternLength;                  // -w (even)
  static float zscoreThreshold;              // -t
  static size_t countThreshold;              // --count-threshold
  static Strand strand;                      // --strand

  static bool useEm;                         // --no-em
  static float emSaturationFactor;           // -a
  static float emMinThreshold;               // --em-threshold
  static int emMaxIterations;                // --em-max-iterations

  static bool useMerging;                    // --no-merging
  static float mergeBitfactorThreshold;      // -b
  static size_t max_merged_length;           // --max_merged_length

  static bool useAdvPWM;                     // --use-default-pwm
  static int pseudoCounts;                   // --pseudo-counts

  static int bgModelOrder;                   // --bg-model-order
  static int maxOptBgModelOrder;
  static bool interpolateBG;
  static std::vector<float> bgModelAlpha;

  static int nr_threads;                     // --threads (accepted; the device path ignores it)
  static int verbosity;                      // -v
  static int device;                         // --device (new: HIP device index, default 0)

  static bool filter_neighbors;              // --no-neighbor-filtering
  static unsigned minimum_processed_motifs;  // --minimum-processed-patterns
  static int maximum_optimized_patterns;     // --max-optimized-patterns

  static bool scoreMotifs;                   // --score-motifs (new: scripts/shoot_peng.py's scoring step, on the device)
  static unsigned long long scoreSeed;       // --score-seed
  static bool scoreNegativesShuffled;        // --score-negatives shuffled (new: every sequence's own dinucleotide-preserving shuffle)
  static char* sitesFilename;                // --sites (new: every motif occurrence with its p-value)
  static double sitesPvalue;                 // --sites-pvalue
  static bool sitesQvalue;                   // --sites-qvalue (new: a q-value column in the sites file)
  static double sitesQvalueMax;              // --sites-qvalue-max (0: every site at --sites-pvalue)
  static char* centralityFilename;           // --centrality (new: central enrichment of the motifs)
  static double centralityPvalue;            // --centrality-pvalue
  static char* refineFilename;               // --refine (new: the motifs re-estimated from their sites)
  static double refinePvalue;                // --refine-pvalue
  static int refineFlank;                    // --refine-flank
  static int refineIterations;               // --refine-iterations
  static double refineMinIC;                 // --refine-min-ic
  static char* dinucFilename;                // --dinuc (new: first-order models of the motifs from their sites)
  static char* dinucModelsFilename;          // --dinuc-models
  static double dinucPvalue;                 // --dinuc-pvalue
  static int dinucFlank;                     // --dinuc-flank
  static double dinucAlpha;                  // --dinuc-alpha
  static char* compareFilename;              // --compare (new: the found motifs against a MEME motif database)
  static char* compareDbFilename;            // --compare-db
  static double compareEvalue;               // --compare-evalue
  static int compareMinOverlap;              // --compare-min-overlap
  static std::vector<MemeMotif> compareDb;   // ... the database, read before the sequences are
  static char* enrichFilename;               // --enrich (new: the motifs of a MEME database tested for enrichment in the input)
  static char* enrichDbFilename;             // --enrich-db
  static double enrichPvalue;                // --enrich-pvalue
  static double enrichEvalue;                // --enrich-evalue
  static std::vector<MemeMotif> enrichDb;    // ... the database, read before the sequences are
  static char* spacingFilename;              // --spacing (new: co-occurrence and preferred gap of motif pairs)
  static double spacingPvalue;               // --spacing-pvalue
  static int spacingMaxGap;                  // --spacing-max-gap
  static int spacingMotifs;                  // --spacing-motifs

  static char* eraseFilename;                // --erase (new: mask the found motifs' sites and search again)
  static int eraseRounds;                    // --erase-rounds: further rounds, 1..8
  static double erasePvalue;                 // --erase-pvalue
  static bool maskLowComplexity;             // --mask-low-complexity (new: symmetric-DUST masking in front of round 1)
  static int maskThreshold;                  // --mask-threshold: 1..1000 (DUST's 20)
  static char* maskReportFilename;           // --mask-report: the masked runs, BED-like
  static char* holdoutFilename;              // --holdout (new: motifs are found on one share of the input and tested on the rest)
  static double holdoutFraction;             // --holdout-fraction: the share set aside, in (0, 0.5]
  static unsigned long long holdoutThreshold; // ... as the split's threshold: (uint64_t)(fraction * 2^32)
  static unsigned long long holdoutSeed;     // --holdout-seed
  static double holdoutPvalue;               // --holdout-pvalue: the floor of the score thresholds tried
  static char* dyadsFilename;                // --dyads (new: spaced trinucleotide pairs counted on the device)
  static int dyadsMaxGap;                    // --dyads-max-gap: 0..PENGK_DYAD_MAX_GAP
  static double dyadsEvalue;                 // --dyads-evalue
  static unsigned long long dyadsMinCount;   // --dyads-min-count
  static char* dyadsMotifsFilename;          // --dyads-motifs: the refined family heads as MEME
  static int dyadsTop;                       // --dyads-top: family heads refined
  static double dyadsPvalue;                 // --dyads-pvalue: site threshold of that refinement
  static char* positionalFilename;           // --positional (new: words with a position bias counted on the device)
  static int positionalWidth;                // --positional-width: PENGK_POSITION_MIN_K..PENGK_POSITION_MAX_K
  static int positionalAnchor;               // --positional-anchor: 0 start, 1 end, 2 center
  static int positionalBinSize;              // --positional-bin-size
  static int positionalBins;                 // --positional-bins: 1..PENGK_POSITION_MAX_BINS
  static double positionalEvalue;            // --positional-evalue
  static unsigned long long positionalMinCount;  // --positional-min-count
  static bool positionalCompositionNull;     // --positional-null composition (new: each word held to its bin's letters)
  static bool stratifiedBackground;          // --stratified-background (new: a GC-stratified null for the k-mer sweep)
  static int stratifiedGcBins;               // --stratified-gc-bins: 1..16
  static unsigned long long stratifiedMinBases;  // --stratified-min-bases: a stratum with fewer model bases takes the global model
  static char* stratifiedReportFilename;     // --stratified-report
  static int highOrderBackground;            // --high-order-background K (new: an order 3..5 Markov null for the k-mer sweep); 0: off
  static float highOrderAlpha;               // --high-order-alpha: the alpha of orders 3..K
  static char* highOrderReportFilename;      // --high-order-report
  static bool discriminative;                // --discriminative (new: the k-mer sweep held to the control set's counts)
  static double discriminativePseudocount;   // --discriminative-pseudocount
  static bool scoreNegativesControl;         // --score-negatives control (new: the --background-sequences file as negatives, matched to the input)
  static bool controlMatchGc;                // --control-match: gc,length | gc | length | none
  static bool controlMatchLength;
  static int controlMatchGcBins;             // --control-match-gc-bins, 1..16
  static unsigned long long controlRatio;    // --control-ratio: control sequences per input sequence, 1 or above
  static char* controlMatchReportFilename;   // --control-match-report

  static void init(int nargs, char* args[]);
  static void destruct();
  static void exitWithError(const std::string& msg);  // a logger line (rank 0) and exit status 4, as for a bad flag

 private:
  static void readArguments(int nargs, char* args[]);
  static void readCompareDb();
  static void readEnrichDb();
  static void printHelp();
};

#endif
