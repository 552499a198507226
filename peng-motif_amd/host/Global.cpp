#include "Global.h"

#include "device.h"

#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <ctime>
#include <iostream>
#include <string>
#include <sys/time.h>

char* Global::alphabetType = (char*)"STANDARD";
char* Global::outputFilename = nullptr;
char* Global::jsonFilename = nullptr;
char* Global::inputSequenceFilename = nullptr;
char* Global::backgroundSequenceFilename = nullptr;
SequenceSet* Global::inputSequenceSet = nullptr;
SequenceSet* Global::backgroundSequenceSet = nullptr;
OPTIMIZATION_SCORE Global::optScoreType = OPTIMIZATION_SCORE::MutualInformation;
float Global::enrich_pseudocount_factor = 0.005f;
int Global::patternLength = 10;
Strand Global::strand = Strand::BOTH_STRANDS;
bool Global::useEm = true;
float Global::emSaturationFactor = 1E4;
float Global::emMinThreshold = 0.08f;
int Global::emMaxIterations = 10;
bool Global::useMerging = true;
int Global::pseudoCounts = 10;
bool Global::useAdvPWM = true;
float Global::zscoreThreshold = 10;
size_t Global::countThreshold = 3;
float Global::mergeBitfactorThreshold = 0.4f;
size_t Global::max_merged_length = 14;
bool Global::interpolateBG = true;
int Global::bgModelOrder = 2;
int Global::maxOptBgModelOrder = 2;
std::vector<float> Global::bgModelAlpha(3, 1.0f);
int Global::verbosity = 2;
int Global::nr_threads = 1;
int Global::device = 0;
bool Global::filter_neighbors = true;
unsigned Global::minimum_processed_motifs = 0;
int Global::maximum_optimized_patterns = 50;
bool Global::scoreMotifs = false;
unsigned long long Global::scoreSeed = 1;
bool Global::scoreNegativesShuffled = false;
char* Global::sitesFilename = nullptr;
double Global::sitesPvalue = 1e-4;
bool Global::sitesQvalue = false;
double Global::sitesQvalueMax = 0.0;
char* Global::centralityFilename = nullptr;
double Global::centralityPvalue = 1e-4;
char* Global::refineFilename = nullptr;
double Global::refinePvalue = 1e-4;
int Global::refineFlank = 8;
int Global::refineIterations = 3;
double Global::refineMinIC = 0.25;
char* Global::dinucFilename = nullptr;
char* Global::dinucModelsFilename = nullptr;
double Global::dinucPvalue = 1e-4;
int Global::dinucFlank = 0;
double Global::dinucAlpha = 20.0;
char* Global::compareFilename = nullptr;
char* Global::compareDbFilename = nullptr;
double Global::compareEvalue = 1.0;
int Global::compareMinOverlap = 5;
std::vector<MemeMotif> Global::compareDb;
char* Global::enrichFilename = nullptr;
char* Global::enrichDbFilename = nullptr;
double Global::enrichPvalue = 1e-3;
double Global::enrichEvalue = 10.0;
std::vector<MemeMotif> Global::enrichDb;
char* Global::spacingFilename = nullptr;
double Global::spacingPvalue = 1e-4;
int Global::spacingMaxGap = 150;
int Global::spacingMotifs = 16;
char* Global::eraseFilename = nullptr;
int Global::eraseRounds = 1;
double Global::erasePvalue = 1e-4;
bool Global::maskLowComplexity = false;
int Global::maskThreshold = 20;
char* Global::maskReportFilename = nullptr;
char* Global::holdoutFilename = nullptr;
double Global::holdoutFraction = 0.1;
unsigned long long Global::holdoutThreshold = 0;
unsigned long long Global::holdoutSeed = 1;   // (--score-seed's default)
double Global::holdoutPvalue = 1e-3;          // (--enrich-pvalue's default)
char* Global::dyadsFilename = nullptr;
int Global::dyadsMaxGap = 20;
double Global::dyadsEvalue = 0.01;
unsigned long long Global::dyadsMinCount = 5;
char* Global::dyadsMotifsFilename = nullptr;
int Global::dyadsTop = 5;
double Global::dyadsPvalue = 1e-3;  // (an exact six-letter match has p = 4^-6 = 2.4e-4: --refine's 1e-4 would find no site)
char* Global::positionalFilename = nullptr;
int Global::positionalWidth = 6;
int Global::positionalAnchor = 2;  // center
int Global::positionalBinSize = 10;
int Global::positionalBins = 20;
double Global::positionalEvalue = 0.01;
unsigned long long Global::positionalMinCount = 5;
bool Global::positionalCompositionNull = false;
bool Global::stratifiedBackground = false;
int Global::stratifiedGcBins = 10;
unsigned long long Global::stratifiedMinBases = 10000;
char* Global::stratifiedReportFilename = nullptr;
int Global::highOrderBackground = 0;
float Global::highOrderAlpha = 1.0f;
char* Global::highOrderReportFilename = nullptr;
bool Global::discriminative = false;
double Global::discriminativePseudocount = 1.0;
bool Global::scoreNegativesControl = false;
bool Global::controlMatchGc = true;
bool Global::controlMatchLength = true;
int Global::controlMatchGcBins = 10;
unsigned long long Global::controlRatio = 1;
char* Global::controlMatchReportFilename = nullptr;

namespace {
void exit_log(const std::string& msg);  // (a logger line at level ERROR; below)
}

void Global::init(int nargs, char* args[]) {
  readArguments(nargs, args);
  readCompareDb();  // (a database that cannot be used ends the run before the input is read)
  readEnrichDb();
  Alphabet::init(alphabetType);
  pengk_host::start_context();  // the device runtime starts while the FASTA files are read
  pengk_host::start_sharded_ingest();  // multi-GPU run: every rank reads its own byte range of the files
  // (the scoring, the sites, the centrality, the refinement, the spacing, the first-order models and the database
  // enrichment scan the input after the motifs are found)
  pengk_host::keep_host_codes(scoreMotifs || sitesFilename || centralityFilename || refineFilename || spacingFilename ||
                              dinucFilename || enrichFilename || eraseFilename || maskLowComplexity || holdoutFilename ||
                              dyadsFilename || positionalFilename || stratifiedBackground || highOrderBackground);
  // both strands are handled inside the count; sequences are always read single stranded
  // ... and every chunk of the input set is packed and sent to the device while the rest is still being read
  pengk_host::begin_streaming_pack(patternLength);
  inputSequenceSet = new SequenceSet(inputSequenceFilename, true);
  pengk_host::finish_streaming_pack(inputSequenceSet);
  // Without --background-sequences the reference reads the input file a second time (src/Global.cpp:66-75) and so
  // prints that file's warnings twice; the set is shared here, its warnings are replayed.
  if (backgroundSequenceFilename) {
    backgroundSequenceSet = new SequenceSet(backgroundSequenceFilename, true);
  } else {
    backgroundSequenceSet = inputSequenceSet;
    std::cerr << inputSequenceSet->diagnostics() << std::flush;
  }
}

void Global::exitWithError(const std::string& msg) {
  if (pengk_host::rank() == 0) exit_log(msg);
  exit(4);
}

void Global::destruct() {
  if (backgroundSequenceSet != inputSequenceSet) delete backgroundSequenceSet;
  delete inputSequenceSet;
  inputSequenceSet = backgroundSequenceSet = nullptr;
}

namespace {
// A line of the reference's logger (src/log.h:42-57, 119-130; only its argument parser uses it): "- HH:MM:SS.mmm LEVEL: "
// in front, and -- every call site ends its message with std::endl, the logger adds its own -- an empty line behind.
void log_line(const char* level, const std::string& msg) {
  char clock[11];
  time_t t;
  time(&t);
  tm r = {};
  strftime(clock, sizeof clock, "%X", localtime_r(&t, &r));
  struct timeval tv;
  gettimeofday(&tv, nullptr);
  fprintf(stderr, "- %s.%03ld %s: %s\n\n", clock, (long)tv.tv_usec / 1000, level, msg.c_str());
  fflush(stderr);
}
void exit_log(const std::string& msg) { log_line("ERROR", msg); }
// value of an option that needs one; exits with 4 like the reference when it is missing
const char* need(int& i, int nargs, char* args[], void (*help)()) {
  const char* opt = args[i];
  if (++i >= nargs) {
    help();
    log_line("ERROR", std::string("No expression following ") + opt);
    exit(4);
  }
  return args[i];
}
}  // namespace

void Global::readCompareDb() {
  if (!compareDbFilename) return;
  std::string err;
  if (!read_meme_db(compareDbFilename, PENGK_MAX_MOTIF_LEN, &compareDb, &err)) {
    if (pengk_host::rank() == 0) log_line("ERROR", "--compare-db: " + err);
    exit(4);
  }
}

void Global::readEnrichDb() {
  if (!enrichDbFilename) return;
  std::string err;
  if (!read_meme_db(enrichDbFilename, PENGK_MAX_MOTIF_LEN, &enrichDb, &err)) {
    if (pengk_host::rank() == 0) log_line("ERROR", "--enrich-db: " + err);
    exit(4);
  }
}

void Global::readArguments(int nargs, char* args[]) {
  if (nargs > 1 && !strcmp(args[1], "-h")) {
    printHelp();
    exit(0);
  }
  if (nargs > 1 && (!strcmp(args[1], "-version") || !strcmp(args[1], "--version"))) {
    std::cout << "peng_motif version " << VERSION_NUMBER << std::endl;
    exit(0);
  }
  if (nargs < 2) {
    fprintf(stderr, "Error: Arguments are missing! \n");
    printHelp();
    exit(-1);
  }
  inputSequenceFilename = args[1];
  const char* holdout_option = nullptr;  // the last option given that only means something with --holdout
  const char* mask_option = nullptr;  // the last option given that only means something with --mask-low-complexity
  const char* dyads_option = nullptr;  // ... with --dyads
  const char* positional_option = nullptr;  // ... with --positional
  const char* stratified_option = nullptr;  // ... with --stratified-background
  const char* high_order_option = nullptr;  // ... with --high-order-background
  for (int i = 2; i < nargs; i++) {
    const char* a = args[i];
    if (!strcmp(a, "-w")) {
      patternLength = std::stoi(need(i, nargs, args, printHelp));
      if (patternLength % 2 == 1) {
        log_line("ERROR", "Due to optimizations the pattern length has to be a multiple of 2");
        exit(4);
      }
    } else if (!strcmp(a, "--background-sequences")) {
      backgroundSequenceFilename = (char*)need(i, nargs, args, printHelp);
    } else if (!strcmp(a, "--optimization_score")) {
      const char* v = need(i, nargs, args, printHelp);
      if (!strcmp(v, "LOGPVAL")) optScoreType = OPTIMIZATION_SCORE::kLogPval;
      else if (!strcmp(v, "ENRICHMENT")) optScoreType = OPTIMIZATION_SCORE::kExpCounts;
      else if (!strcmp(v, "MUTUAL_INFO")) optScoreType = OPTIMIZATION_SCORE::MutualInformation;
      else {
        printHelp();
        log_line("ERROR", "Unknown expression following --optimization_score");
        exit(4);
      }
    } else if (!strcmp(a, "--enrich_pseudocount_factor")) {
      enrich_pseudocount_factor = std::stof(need(i, nargs, args, printHelp));
    } else if (!strcmp(a, "-v")) {
      verbosity = std::stoi(need(i, nargs, args, printHelp));
    } else if (!strcmp(a, "-o")) {
      outputFilename = (char*)need(i, nargs, args, printHelp);
    } else if (!strcmp(a, "-j")) {
      jsonFilename = (char*)need(i, nargs, args, printHelp);
    } else if (!strcmp(a, "-t")) {
      zscoreThreshold = std::stof(need(i, nargs, args, printHelp));
    } else if (!strcmp(a, "--count-threshold")) {
      countThreshold = std::stoi(need(i, nargs, args, printHelp));
    } else if (!strcmp(a, "-b")) {
      mergeBitfactorThreshold = std::stof(need(i, nargs, args, printHelp));
    } else if (!strcmp(a, "--use-default-pwm")) {
      useAdvPWM = false;
    } else if (!strcmp(a, "--pseudo-counts")) {
      pseudoCounts = std::stoi(need(i, nargs, args, printHelp));
    } else if (!strcmp(a, "--threads")) {
      nr_threads = std::stoi(need(i, nargs, args, printHelp));
    } else if (!strcmp(a, "--device")) {
      device = std::stoi(need(i, nargs, args, printHelp));
    } else if (!strcmp(a, "--no-em")) {
      useEm = false;
    } else if (!strcmp(a, "-a")) {
      emSaturationFactor = std::stof(need(i, nargs, args, printHelp));
    } else if (!strcmp(a, "--em-threshold")) {
      emMinThreshold = std::stof(need(i, nargs, args, printHelp));
    } else if (!strcmp(a, "--em-max-iterations")) {
      emMaxIterations = std::stoi(need(i, nargs, args, printHelp));
    } else if (!strcmp(a, "--no-merging")) {
      useMerging = false;
    } else if (!strcmp(a, "--max_merged_length")) {
      max_merged_length = std::stoi(need(i, nargs, args, printHelp));
    } else if (!strcmp(a, "--strand")) {
      const char* v = need(i, nargs, args, printHelp);
      if (!strcmp(v, "BOTH")) strand = Strand::BOTH_STRANDS;
      else if (!strcmp(v, "PLUS")) strand = Strand::PLUS_STRAND;
      else {
        printHelp();
        log_line("ERROR", "Unknown expression following --strand");
        exit(4);
      }
    } else if (!strcmp(a, "--bg-model-order")) {
      bgModelOrder = std::stoi(need(i, nargs, args, printHelp));
      if (bgModelOrder < 0 || bgModelOrder > 2) {
        log_line("ERROR", "background model orders above 2 are not supported");  // (not in the reference: its alpha vector has three entries, src/Global.cpp:49)
        exit(4);
      }
    } else if (!strcmp(a, "--no-neighbor-filtering")) {
      filter_neighbors = false;
    } else if (!strcmp(a, "--minimum-processed-patterns")) {
      minimum_processed_motifs = std::stoi(need(i, nargs, args, printHelp));
    } else if (!strcmp(a, "--max-optimized-patterns")) {
      maximum_optimized_patterns = std::stoi(need(i, nargs, args, printHelp));
    } else if (!strcmp(a, "--score-motifs")) {
      scoreMotifs = true;
    } else if (!strcmp(a, "--score-seed")) {
      scoreSeed = std::stoull(need(i, nargs, args, printHelp));
    } else if (!strcmp(a, "--score-negatives")) {
      const char* v = need(i, nargs, args, printHelp);
      if (!strcmp(v, "sampled")) scoreNegativesShuffled = scoreNegativesControl = false;
      else if (!strcmp(v, "shuffled")) scoreNegativesShuffled = true, scoreNegativesControl = false;
      else if (!strcmp(v, "control")) scoreNegativesShuffled = false, scoreNegativesControl = true;
      else {
        printHelp();
        log_line("ERROR", "Unknown expression following --score-negatives");
        exit(4);
      }
    } else if (!strcmp(a, "--sites")) {
      sitesFilename = (char*)need(i, nargs, args, printHelp);
    } else if (!strcmp(a, "--sites-pvalue")) {
      const char* v = need(i, nargs, args, printHelp);
      char* end = nullptr;
      sitesPvalue = std::strtod(v, &end);
      if (end == v || *end || !(sitesPvalue > 0.0 && sitesPvalue <= 1.0)) {
        printHelp();
        log_line("ERROR", "--sites-pvalue must be a number in (0, 1]");
        exit(4);
      }
    } else if (!strcmp(a, "--sites-qvalue")) {
      sitesQvalue = true;
    } else if (!strcmp(a, "--sites-qvalue-max")) {
      const char* v = need(i, nargs, args, printHelp);
      char* end = nullptr;
      sitesQvalueMax = std::strtod(v, &end);
      if (end == v || *end || !(sitesQvalueMax > 0.0 && sitesQvalueMax <= 1.0)) {
        printHelp();
        log_line("ERROR", "--sites-qvalue-max must be a number in (0, 1]");
        exit(4);
      }
      sitesQvalue = true;
    } else if (!strcmp(a, "--centrality")) {
      centralityFilename = (char*)need(i, nargs, args, printHelp);
    } else if (!strcmp(a, "--centrality-pvalue")) {
      const char* v = need(i, nargs, args, printHelp);
      char* end = nullptr;
      centralityPvalue = std::strtod(v, &end);
      if (end == v || *end || !(centralityPvalue > 0.0 && centralityPvalue <= 1.0)) {
        printHelp();
        log_line("ERROR", "--centrality-pvalue must be a number in (0, 1]");
        exit(4);
      }
    } else if (!strcmp(a, "--refine")) {
      refineFilename = (char*)need(i, nargs, args, printHelp);
    } else if (!strcmp(a, "--refine-pvalue")) {
      const char* v = need(i, nargs, args, printHelp);
      char* end = nullptr;
      refinePvalue = std::strtod(v, &end);
      if (end == v || *end || !(refinePvalue > 0.0 && refinePvalue <= 1.0)) {
        printHelp();
        log_line("ERROR", "--refine-pvalue must be a number in (0, 1]");
        exit(4);
      }
    } else if (!strcmp(a, "--refine-flank") || !strcmp(a, "--refine-iterations")) {
      const bool flank = a[9] == 'f';
      const char* v = need(i, nargs, args, printHelp);
      char* end = nullptr;
      const long n = std::strtol(v, &end, 10);
      if (end == v || *end || n < (flank ? 0 : 1) || n > 1000) {
        printHelp();
        log_line("ERROR", flank ? "--refine-flank must be an integer in [0, 1000]" : "--refine-iterations must be an integer in [1, 1000]");
        exit(4);
      }
      (flank ? refineFlank : refineIterations) = (int)n;
    } else if (!strcmp(a, "--refine-min-ic")) {
      const char* v = need(i, nargs, args, printHelp);
      char* end = nullptr;
      refineMinIC = std::strtod(v, &end);
      if (end == v || *end || !(refineMinIC >= 0.0 && refineMinIC <= 2.0)) {
        printHelp();
        log_line("ERROR", "--refine-min-ic must be a number of bits in [0, 2]");
        exit(4);
      }
    } else if (!strcmp(a, "--dinuc")) {
      dinucFilename = (char*)need(i, nargs, args, printHelp);
    } else if (!strcmp(a, "--dinuc-models")) {
      dinucModelsFilename = (char*)need(i, nargs, args, printHelp);
    } else if (!strcmp(a, "--dinuc-pvalue")) {
      const char* v = need(i, nargs, args, printHelp);
      char* end = nullptr;
      dinucPvalue = std::strtod(v, &end);
      if (end == v || *end || !(dinucPvalue > 0.0 && dinucPvalue <= 1.0)) {
        printHelp();
        log_line("ERROR", "--dinuc-pvalue must be a number in (0, 1]");
        exit(4);
      }
    } else if (!strcmp(a, "--dinuc-flank")) {
      const char* v = need(i, nargs, args, printHelp);
      char* end = nullptr;
      const long n = std::strtol(v, &end, 10);
      if (end == v || *end || n < 0 || n > 1000) {
        printHelp();
        log_line("ERROR", "--dinuc-flank must be an integer in [0, 1000]");
        exit(4);
      }
      dinucFlank = (int)n;
    } else if (!strcmp(a, "--dinuc-alpha")) {
      const char* v = need(i, nargs, args, printHelp);
      char* end = nullptr;
      dinucAlpha = std::strtod(v, &end);
      if (end == v || *end || !(dinucAlpha > 0.0 && dinucAlpha <= 1e300)) {
        printHelp();
        log_line("ERROR", "--dinuc-alpha must be a number above 0");
        exit(4);
      }
    } else if (!strcmp(a, "--compare")) {
      compareFilename = (char*)need(i, nargs, args, printHelp);
    } else if (!strcmp(a, "--compare-db")) {
      compareDbFilename = (char*)need(i, nargs, args, printHelp);
    } else if (!strcmp(a, "--compare-evalue")) {
      const char* v = need(i, nargs, args, printHelp);
      char* end = nullptr;
      compareEvalue = std::strtod(v, &end);
      if (end == v || *end || !(compareEvalue >= 0.0 && compareEvalue <= 1e300)) {
        printHelp();
        log_line("ERROR", "--compare-evalue must be a number, 0 or above");
        exit(4);
      }
    } else if (!strcmp(a, "--compare-min-overlap")) {
      const char* v = need(i, nargs, args, printHelp);
      char* end = nullptr;
      const long n = std::strtol(v, &end, 10);
      if (end == v || *end || n < 1 || n > PENGK_MAX_MOTIF_LEN) {
        printHelp();
        log_line("ERROR", "--compare-min-overlap must be an integer in [1, 64]");
        exit(4);
      }
      compareMinOverlap = (int)n;
    } else if (!strcmp(a, "--enrich")) {
      enrichFilename = (char*)need(i, nargs, args, printHelp);
    } else if (!strcmp(a, "--enrich-db")) {
      enrichDbFilename = (char*)need(i, nargs, args, printHelp);
    } else if (!strcmp(a, "--enrich-pvalue")) {
      const char* v = need(i, nargs, args, printHelp);
      char* end = nullptr;
      enrichPvalue = std::strtod(v, &end);
      if (end == v || *end || !(enrichPvalue > 0.0 && enrichPvalue <= 1.0)) {
        printHelp();
        log_line("ERROR", "--enrich-pvalue must be a number in (0, 1]");
        exit(4);
      }
    } else if (!strcmp(a, "--enrich-evalue")) {
      const char* v = need(i, nargs, args, printHelp);
      char* end = nullptr;
      enrichEvalue = std::strtod(v, &end);
      if (end == v || *end || !(enrichEvalue > 0.0 && enrichEvalue <= 1e300)) {
        printHelp();
        log_line("ERROR", "--enrich-evalue must be a number above 0");
        exit(4);
      }
    } else if (!strcmp(a, "--spacing")) {
      spacingFilename = (char*)need(i, nargs, args, printHelp);
    } else if (!strcmp(a, "--spacing-pvalue")) {
      const char* v = need(i, nargs, args, printHelp);
      char* end = nullptr;
      spacingPvalue = std::strtod(v, &end);
      if (end == v || *end || !(spacingPvalue > 0.0 && spacingPvalue <= 1.0)) {
        printHelp();
        log_line("ERROR", "--spacing-pvalue must be a number in (0, 1]");
        exit(4);
      }
    } else if (!strcmp(a, "--spacing-max-gap") || !strcmp(a, "--spacing-motifs")) {
      const bool gap = a[11] == 'a';
      const char* v = need(i, nargs, args, printHelp);
      char* end = nullptr;
      const long n = std::strtol(v, &end, 10);
      if (end == v || *end || n < (gap ? 0 : 2) || n > (gap ? PENGK_SPACING_MAX_GAP : PENGK_SPACING_MAX_MOTIFS)) {
        printHelp();
        log_line("ERROR", gap ? "--spacing-max-gap must be an integer in [0, 1024]" : "--spacing-motifs must be an integer in [2, 64]");
        exit(4);
      }
      (gap ? spacingMaxGap : spacingMotifs) = (int)n;
    } else if (!strcmp(a, "--erase")) {
      eraseFilename = (char*)need(i, nargs, args, printHelp);
    } else if (!strcmp(a, "--erase-rounds")) {
      const char* v = need(i, nargs, args, printHelp);
      char* end = nullptr;
      const long n = std::strtol(v, &end, 10);
      if (end == v || *end || n < 1 || n > 8) {
        printHelp();
        log_line("ERROR", "--erase-rounds must be an integer in [1, 8]");
        exit(4);
      }
      eraseRounds = (int)n;
    } else if (!strcmp(a, "--erase-pvalue")) {
      const char* v = need(i, nargs, args, printHelp);
      char* end = nullptr;
      erasePvalue = std::strtod(v, &end);
      if (end == v || *end || !(erasePvalue > 0.0 && erasePvalue <= 1.0)) {
        printHelp();
        log_line("ERROR", "--erase-pvalue must be a number in (0, 1]");
        exit(4);
      }
    } else if (!strcmp(a, "--mask-low-complexity")) {
      maskLowComplexity = true;
    } else if (!strcmp(a, "--mask-threshold")) {
      const char* v = need(i, nargs, args, printHelp);
      char* end = nullptr;
      const long n = std::strtol(v, &end, 10);
      if (end == v || *end || n < 1 || n > 1000) {
        printHelp();
        log_line("ERROR", "--mask-threshold must be an integer in [1, 1000]");
        exit(4);
      }
      maskThreshold = (int)n;
      mask_option = "--mask-threshold";
    } else if (!strcmp(a, "--mask-report")) {
      maskReportFilename = (char*)need(i, nargs, args, printHelp);
      mask_option = "--mask-report";
    } else if (!strcmp(a, "--holdout")) {
      holdoutFilename = (char*)need(i, nargs, args, printHelp);
    } else if (!strcmp(a, "--holdout-fraction")) {
      const char* v = need(i, nargs, args, printHelp);
      char* end = nullptr;
      holdoutFraction = std::strtod(v, &end);
      // (the threshold of the split: a fraction that rounds to no sequence at all is refused with the rest)
      if (end == v || *end || !(holdoutFraction > 0.0 && holdoutFraction <= 0.5) || (uint64_t)(holdoutFraction * 4294967296.0) == 0) {
        printHelp();
        log_line("ERROR", "--holdout-fraction must be a number in (0, 0.5], 2^-32 at the least");
        exit(4);
      }
      holdout_option = "--holdout-fraction";
    } else if (!strcmp(a, "--holdout-seed")) {
      const char* v = need(i, nargs, args, printHelp);
      char* end = nullptr;
      holdoutSeed = std::strtoull(v, &end, 10);
      if (end == v || *end || *v == '-') {
        printHelp();
        log_line("ERROR", "--holdout-seed must be an integer, 0 or above");
        exit(4);
      }
      holdout_option = "--holdout-seed";
    } else if (!strcmp(a, "--holdout-pvalue")) {
      const char* v = need(i, nargs, args, printHelp);
      char* end = nullptr;
      holdoutPvalue = std::strtod(v, &end);
      if (end == v || *end || !(holdoutPvalue > 0.0 && holdoutPvalue <= 1.0)) {
        printHelp();
        log_line("ERROR", "--holdout-pvalue must be a number in (0, 1]");
        exit(4);
      }
      holdout_option = "--holdout-pvalue";
    } else if (!strcmp(a, "--dyads")) {
      dyadsFilename = (char*)need(i, nargs, args, printHelp);
    } else if (!strcmp(a, "--dyads-motifs")) {
      dyadsMotifsFilename = (char*)need(i, nargs, args, printHelp);
      dyads_option = "--dyads-motifs";
    } else if (!strcmp(a, "--dyads-max-gap") || !strcmp(a, "--dyads-min-count") || !strcmp(a, "--dyads-top")) {
      const int which = !strcmp(a, "--dyads-max-gap") ? 0 : !strcmp(a, "--dyads-min-count") ? 1 : 2;
      static const char* const kName[3] = {"--dyads-max-gap", "--dyads-min-count", "--dyads-top"};
      static const char* const kRange[3] = {"--dyads-max-gap must be an integer in [0, 26]",
                                            "--dyads-min-count must be an integer in [1, 1000000000]",
                                            "--dyads-top must be an integer in [1, 64]"};
      const long long lo = which == 0 ? 0 : 1, hi = which == 0 ? PENGK_DYAD_MAX_GAP : which == 1 ? 1000000000ll : 64;
      const char* v = need(i, nargs, args, printHelp);
      char* end = nullptr;
      const long long n = std::strtoll(v, &end, 10);
      if (end == v || *end || n < lo || n > hi) {
        printHelp();
        log_line("ERROR", kRange[which]);
        exit(4);
      }
      if (which == 0) dyadsMaxGap = (int)n;
      else if (which == 1) dyadsMinCount = (unsigned long long)n;
      else dyadsTop = (int)n;
      dyads_option = kName[which];
    } else if (!strcmp(a, "--dyads-evalue") || !strcmp(a, "--dyads-pvalue")) {
      const bool ev = !strcmp(a, "--dyads-evalue");
      const char* v = need(i, nargs, args, printHelp);
      char* end = nullptr;
      const double x = std::strtod(v, &end);
      if (end == v || *end || !(x > 0.0) || (ev ? !(x <= 1e300) : !(x <= 1.0))) {
        printHelp();
        log_line("ERROR", ev ? "--dyads-evalue must be a positive number" : "--dyads-pvalue must be a number in (0, 1]");
        exit(4);
      }
      (ev ? dyadsEvalue : dyadsPvalue) = x;
      dyads_option = ev ? "--dyads-evalue" : "--dyads-pvalue";
    } else if (!strcmp(a, "--positional")) {
      positionalFilename = (char*)need(i, nargs, args, printHelp);
    } else if (!strcmp(a, "--positional-anchor")) {
      const char* v = need(i, nargs, args, printHelp);
      if (!strcmp(v, "start")) positionalAnchor = 0;
      else if (!strcmp(v, "end")) positionalAnchor = 1;
      else if (!strcmp(v, "center")) positionalAnchor = 2;
      else {
        printHelp();
        log_line("ERROR", "--positional-anchor must be start, end or center");
        exit(4);
      }
      positional_option = "--positional-anchor";
    } else if (!strcmp(a, "--positional-width") || !strcmp(a, "--positional-bin-size") || !strcmp(a, "--positional-bins") ||
               !strcmp(a, "--positional-min-count")) {
      const int which = !strcmp(a, "--positional-width") ? 0 : !strcmp(a, "--positional-bin-size") ? 1 : !strcmp(a, "--positional-bins") ? 2 : 3;
      static const char* const kName[4] = {"--positional-width", "--positional-bin-size", "--positional-bins", "--positional-min-count"};
      static const char* const kRange[4] = {"--positional-width must be an integer in [4, 7]",
                                            "--positional-bin-size must be an integer in [1, 65536]",
                                            "--positional-bins must be an integer in [1, 64]",
                                            "--positional-min-count must be an integer in [1, 1000000000]"};
      static const long long kLo[4] = {PENGK_POSITION_MIN_K, 1, 1, 1};
      static const long long kHi[4] = {PENGK_POSITION_MAX_K, PENGK_POSITION_MAX_BIN_SIZE, PENGK_POSITION_MAX_BINS, 1000000000ll};
      const char* v = need(i, nargs, args, printHelp);
      char* end = nullptr;
      const long long n = std::strtoll(v, &end, 10);
      if (end == v || *end || n < kLo[which] || n > kHi[which]) {
        printHelp();
        log_line("ERROR", kRange[which]);
        exit(4);
      }
      if (which == 0) positionalWidth = (int)n;
      else if (which == 1) positionalBinSize = (int)n;
      else if (which == 2) positionalBins = (int)n;
      else positionalMinCount = (unsigned long long)n;
      positional_option = kName[which];
    } else if (!strcmp(a, "--positional-evalue")) {
      const char* v = need(i, nargs, args, printHelp);
      char* end = nullptr;
      const double x = std::strtod(v, &end);
      if (end == v || *end || !(x > 0.0) || !(x <= 1e300)) {
        printHelp();
        log_line("ERROR", "--positional-evalue must be a positive number");
        exit(4);
      }
      positionalEvalue = x;
      positional_option = "--positional-evalue";
    } else if (!strcmp(a, "--positional-null")) {
      const char* v = need(i, nargs, args, printHelp);
      if (!strcmp(v, "flat")) positionalCompositionNull = false;
      else if (!strcmp(v, "composition")) positionalCompositionNull = true;
      else {
        printHelp();
        log_line("ERROR", "--positional-null must be flat or composition");
        exit(4);
      }
      positional_option = "--positional-null";
    } else if (!strcmp(a, "--stratified-background")) {
      stratifiedBackground = true;
    } else if (!strcmp(a, "--stratified-report")) {
      stratifiedReportFilename = (char*)need(i, nargs, args, printHelp);
      stratified_option = "--stratified-report";
    } else if (!strcmp(a, "--stratified-gc-bins") || !strcmp(a, "--stratified-min-bases")) {
      const bool bins = !strcmp(a, "--stratified-gc-bins");
      const char* v = need(i, nargs, args, printHelp);
      char* end = nullptr;
      const long long n = std::strtoll(v, &end, 10);
      if (end == v || *end || n < (bins ? 1 : 0) || n > (bins ? 16 : 1000000000000ll)) {
        printHelp();
        log_line("ERROR", bins ? "--stratified-gc-bins must be an integer in [1, 16]"
                               : "--stratified-min-bases must be an integer in [0, 1000000000000]");
        exit(4);
      }
      if (bins) stratifiedGcBins = (int)n;
      else stratifiedMinBases = (unsigned long long)n;
      stratified_option = bins ? "--stratified-gc-bins" : "--stratified-min-bases";
    } else if (!strcmp(a, "--high-order-background")) {
      const char* v = need(i, nargs, args, printHelp);
      char* end = nullptr;
      const long n = std::strtol(v, &end, 10);
      if (end == v || *end || n < 3 || n > 5) {
        printHelp();
        log_line("ERROR", "--high-order-background must be an integer in [3, 5]");
        exit(4);
      }
      highOrderBackground = (int)n;
    } else if (!strcmp(a, "--high-order-alpha")) {
      const char* v = need(i, nargs, args, printHelp);
      char* end = nullptr;
      const double x = std::strtod(v, &end);
      if (end == v || *end || !std::isfinite(x) || !(x > 0.0) || !((float)x > 0.0f) || !std::isfinite((float)x)) {
        printHelp();
        log_line("ERROR", "--high-order-alpha must be a finite number above 0");
        exit(4);
      }
      highOrderAlpha = (float)x;
      high_order_option = "--high-order-alpha";
    } else if (!strcmp(a, "--high-order-report")) {
      highOrderReportFilename = (char*)need(i, nargs, args, printHelp);
      high_order_option = "--high-order-report";
    } else if (!strcmp(a, "--discriminative")) {
      discriminative = true;
    } else if (!strcmp(a, "--discriminative-pseudocount")) {
      const char* v = need(i, nargs, args, printHelp);
      char* end = nullptr;
      discriminativePseudocount = std::strtod(v, &end);
      if (end == v || *end || !std::isfinite(discriminativePseudocount) || discriminativePseudocount < 0.0) {
        printHelp();
        log_line("ERROR", "--discriminative-pseudocount must be a finite number, 0 or above");
        exit(4);
      }
    } else if (!strcmp(a, "--control-match")) {
      const char* v = need(i, nargs, args, printHelp);
      if (!strcmp(v, "gc,length") || !strcmp(v, "length,gc")) controlMatchGc = controlMatchLength = true;
      else if (!strcmp(v, "gc")) controlMatchGc = true, controlMatchLength = false;
      else if (!strcmp(v, "length")) controlMatchGc = false, controlMatchLength = true;
      else if (!strcmp(v, "none")) controlMatchGc = controlMatchLength = false;
      else {
        printHelp();
        log_line("ERROR", "Unknown expression following --control-match");
        exit(4);
      }
    } else if (!strcmp(a, "--control-match-gc-bins")) {
      const char* v = need(i, nargs, args, printHelp);
      char* end = nullptr;
      const long g = std::strtol(v, &end, 10);
      if (end == v || *end || g < 1 || g > 16) {
        printHelp();
        log_line("ERROR", "--control-match-gc-bins must be an integer in 1..16");
        exit(4);
      }
      controlMatchGcBins = (int)g;
    } else if (!strcmp(a, "--control-ratio")) {
      const char* v = need(i, nargs, args, printHelp);
      char* end = nullptr;
      const long long r = std::strtoll(v, &end, 10);
      if (end == v || *end || r < 1 || r > 1000000) {
        printHelp();
        log_line("ERROR", "--control-ratio must be an integer in 1..1000000");
        exit(4);
      }
      controlRatio = (unsigned long long)r;
    } else if (!strcmp(a, "--control-match-report")) {
      controlMatchReportFilename = (char*)need(i, nargs, args, printHelp);
    } else if (!strcmp(a, "--version")) {
      std::cout << "peng_motif " << VERSION_NUMBER << std::endl;  // (src/Global.cpp:299-301: without the word)
      exit(0);
    } else if (!strcmp(a, "-h")) {
      printHelp();
      exit(0);
    } else {
      if (pengk_host::rank() == 0) log_line("WARNING", std::string("Ignoring unknown option ") + a);
    }
  }
  if (holdout_option && !holdoutFilename) {
    printHelp();
    log_line("ERROR", std::string(holdout_option) + " requires --holdout");
    exit(4);
  }
  holdoutThreshold = (unsigned long long)(holdoutFraction * 4294967296.0);
  if (dyads_option && !dyadsFilename) {
    printHelp();
    log_line("ERROR", std::string(dyads_option) + " requires --dyads");
    exit(4);
  }
  if (stratified_option && !stratifiedBackground) {
    printHelp();
    log_line("ERROR", std::string(stratified_option) + " requires --stratified-background");
    exit(4);
  }
  if (high_order_option && !highOrderBackground) {
    printHelp();
    log_line("ERROR", std::string(high_order_option) + " requires --high-order-background");
    exit(4);
  }
  if (highOrderBackground) {
    const char* why = nullptr;
    if (highOrderBackground >= patternLength) why = "--high-order-background must be below the pattern length (-w)";
    else if (stratifiedBackground) why = "--high-order-background cannot be combined with --stratified-background";
    else if (bgModelOrder != 2 || maxOptBgModelOrder != 2) why = "--high-order-background needs the default --bg-model-order 2";
    if (why) {
      printHelp();
      log_line("ERROR", why);
      exit(4);
    }
  }
  if (positional_option && !positionalFilename) {
    printHelp();
    log_line("ERROR", std::string(positional_option) + " requires --positional");
    exit(4);
  }
  if (mask_option && !maskLowComplexity) {
    printHelp();
    log_line("ERROR", std::string(mask_option) + " requires --mask-low-complexity");
    exit(4);
  }
  if (discriminative && !backgroundSequenceFilename) {
    printHelp();
    log_line("ERROR", "--discriminative requires --background-sequences (the control set)");
    exit(4);
  }
  if (scoreNegativesControl && !backgroundSequenceFilename) {
    printHelp();
    log_line("ERROR", "--score-negatives control requires --background-sequences (the control set)");
    exit(4);
  }
  if (dinucModelsFilename && !dinucFilename) {
    printHelp();
    log_line("ERROR", "--dinuc-models requires --dinuc");
    exit(4);
  }
  if (!compareFilename != !compareDbFilename) {
    printHelp();
    log_line("ERROR", compareFilename ? "--compare requires --compare-db" : "--compare-db requires --compare");
    exit(4);
  }
  if (!enrichFilename != !enrichDbFilename) {
    printHelp();
    log_line("ERROR", enrichFilename ? "--enrich requires --enrich-db" : "--enrich-db requires --enrich");
    exit(4);
  }
}

void Global::printHelp() {
  printf("\n");
  printf("SYNOPSIS:  peng_motif SEQFILE [OPTIONS]      (MI355X build: the k-mer count, z-score sweep,\n");
  printf("           IUPAC aggregation and EM run as HIP kernels through libpengk)\n\n");
  printf("  SEQFILE                        FASTA file with the input sequences\n");
  printf("  -o FILE                        write motifs in short MEME format\n");
  printf("  -j FILE                        write motifs as JSON\n");
  printf("  --background-sequences FILE    FASTA file for the background model (default: SEQFILE)\n");
  printf("  --discriminative               hold the k-mer enrichment to the counts of the --background-sequences file as\n");
  printf("                                 well: the expected count of a k-mer is the larger of what the background\n");
  printf("                                 model predicts and what that control set shows (requires --background-sequences)\n");
  printf("  --discriminative-pseudocount FLOAT   added to every control count, 0 or above (default 1)\n");
  printf("  --mask-low-complexity          mask low-complexity stretches (poly-A, (CA)n, triplet repeats) of the input on the\n");
  printf("                                 device before anything is counted: this program's statement of the symmetric DUST\n");
  printf("                                 criterion, window 64.  With --discriminative the control set is masked likewise;\n");
  printf("                                 the rounds of --erase start from the masked input; the reports scan the input as it is\n");
  printf("  --mask-threshold INT           score threshold of --mask-low-complexity, 1..1000 (default 20, DUST's)\n");
  printf("  --mask-report FILE             the masked runs: sequence index, start, end (half-open), tab-separated\n");
  printf("  --holdout FILE                 set a share of the input aside before anything is counted, find the motifs on the\n");
  printf("                                 rest and test each on the share it never saw.  FILE: one line per motif with its\n");
  printf("                                 hits on both shares and the hold-out p-value, the unbiased one.  Negatives as\n");
  printf("                                 --score-negatives says; with --discriminative the control set is split likewise;\n");
  printf("                                 every other report scans the whole input\n");
  printf("  --holdout-fraction FLOAT       the share set aside, in (0, 0.5] (default 0.1)\n");
  printf("  --holdout-seed INT             seed of the split (default 1)\n");
  printf("  --holdout-pvalue FLOAT         per-window p-value of the lowest score threshold tried, in (0, 1] (default 1e-3)\n");
  printf("  --dyads FILE                   count every pair of trinucleotides 0 .. --dyads-max-gap unconstrained bases apart over\n");
  printf("                                 what round 1 counts, test each against the product of the triplet frequencies\n");
  printf("                                 (binomial, E-value over all pairs and gaps) and fold shifted neighbours into\n");
  printf("                                 families: the bipartite sites of dimeric factors (CGG n11 CCG), which no\n");
  printf("                                 contiguous word holds.  FILE: one line per dyad, tab-separated\n");
  printf("  --dyads-max-gap INT            largest spacer counted, 0..26 (default 20)\n");
  printf("  --dyads-evalue FLOAT           a dyad is reported at this E-value or below (default 0.01)\n");
  printf("  --dyads-min-count INT          occurrences a dyad needs (default 5)\n");
  printf("  --dyads-motifs FILE            the first family heads refined from their sites as --refine does it, as MEME\n");
  printf("  --dyads-top INT                family heads refined, 1..64 (default 5)\n");
  printf("  --dyads-pvalue FLOAT           p-value threshold of a site in that refinement, in (0, 1] (default 1e-3)\n");
  printf("  --positional FILE              count the words of --positional-width letters per position bin over what round 1\n");
  printf("                                 counts (overlapping repeats of a word once), test each word's count in a bin against\n");
  printf("                                 its count everywhere and the bin's share of all words (binomial, E-value over all\n");
  printf("                                 words and bins) and fold shifted neighbours into families: words that keep one\n");
  printf("                                 position (a TATA box, a splice signal) whether or not they are over-represented.\n");
  printf("                                 FILE: one line per word, tab-separated\n");
  printf("  --positional-width INT         letters of a word, 4..7 (default 6)\n");
  printf("  --positional-anchor NAME       positions are measured from the start, the end or the center of a sequence\n");
  printf("                                 (center: the unsigned distance; default center)\n");
  printf("  --positional-bin-size INT      positions a bin holds, 1..65536 (default 10)\n");
  printf("  --positional-bins INT          bins counted from the anchor on, 1..64 (default 20); words further out are ignored\n");
  printf("  --positional-evalue FLOAT      a word is reported at this E-value or below (default 0.01)\n");
  printf("  --positional-min-count INT     occurrences a word needs in its bin (default 5)\n");
  printf("  --positional-null NAME         flat: a bin's share of a word is its share of all words (default).  composition: the\n");
  printf("                                 share is tilted by what the bin's own letters make of the word -- a first-order chain\n");
  printf("                                 from the first pairs of the bin's words, counted on the device --, for inputs whose\n");
  printf("                                 composition changes along the sequence (promoters, peaks); FILE gets the column\n");
  printf("                                 flat_expected\n");
  printf("  --stratified-background        score the k-mers against a GC-stratified null: the sequences are put into GC bins, every\n");
  printf("                                 bin gets a background model of its own (same order, alpha and interpolation) from the\n");
  printf("                                 background set's sequences of that bin, and a k-mer's probability is the mean of the\n");
  printf("                                 bins' Markov probabilities weighted by the windows the counted input holds in each.\n");
  printf("                                 For inputs of mixed composition, where G+C-rich and A+T-rich words are enriched\n");
  printf("                                 against one model.  The reports' log-odds and p-values keep the one model\n");
  printf("  --stratified-gc-bins INT       GC bins, 1..16 (default 10)\n");
  printf("  --stratified-min-bases INT     a bin whose model would be trained on fewer bases takes the global model (default 10000)\n");
  printf("  --stratified-report FILE       one line per bin, tab-separated: its GC range, sequences, windows, model bases,\n");
  printf("                                 the model used (own | global) and its four base probabilities\n");
  printf("  --high-order-background K      score the k-mers against a Markov null of order K, 3..5 and below -w, in place of the\n");
  printf("                                 order-2 model: counted on the device over the background set as it was read,\n");
  printf("                                 interpolated like the lower orders.  For large inputs, where words built of common\n");
  printf("                                 4-6-mers are enriched against an order-2 model.  A motif's own letters feed the\n");
  printf("                                 model, so its z-score falls with K.  The reports' log-odds and p-values keep the one\n");
  printf("                                 model; not with --stratified-background or another --bg-model-order than 2\n");
  printf("  --high-order-alpha FLOAT       pseudo-count weight of orders 3..K, above 0 (default 1)\n");
  printf("  --high-order-report FILE       one line per order 0..K, tab-separated: contexts, contexts seen, smallest and median\n");
  printf("                                 count of a context\n");
  printf("  --erase FILE                   after the search, mask the sites of the motifs found and search what is left\n");
  printf("                                 again; the later rounds' motifs are appended.  FILE: one line per round and motif\n");
  printf("  --erase-rounds INT             further rounds of --erase, 1..8 (default 1); a round that finds or erases\n");
  printf("                                 nothing is the last\n");
  printf("  --erase-pvalue FLOAT           p-value threshold of the sites that --erase masks, in (0, 1] (default 1e-4)\n");
  printf("  -w INT                         pattern length, even, 4..14 (default 10)\n");
  printf("  -t FLOAT                       z-score threshold for seed k-mers (default 10)\n");
  printf("  --count-threshold INT          minimum count of a seed k-mer (default 3)\n");
  printf("  --bg-model-order INT           background model order 0..2 (default 2)\n");
  printf("  --strand BOTH|PLUS             strands to search (default BOTH)\n");
  printf("  --optimization_score ENRICHMENT|LOGPVAL|MUTUAL_INFO   (default MUTUAL_INFO)\n");
  printf("  --enrich_pseudocount_factor F  pseudo count factor for ENRICHMENT (default 0.005)\n");
  printf("  --no-em                        skip the EM refinement\n");
  printf("  -a FLOAT                       EM saturation factor (default 1e4)\n");
  printf("  --em-threshold FLOAT           EM convergence threshold (default 0.08)\n");
  printf("  --em-max-iterations INT        (default 10)\n");
  printf("  --no-merging                   do not merge similar PWMs\n");
  printf("  -b FLOAT                       merge bit-factor threshold (default 0.4)\n");
  printf("  --max_merged_length INT        (default 14)\n");
  printf("  --use-default-pwm              simple PWM construction instead of the advanced one\n");
  printf("  --pseudo-counts INT            PWM pseudo counts (default 10)\n");
  printf("  --no-neighbor-filtering        keep Hamming-1 neighbours of selected seeds\n");
  printf("  --minimum-processed-patterns INT   (default 0)\n");
  printf("  --max-optimized-patterns INT       (default 50)\n");
  printf("  --score-motifs                 score every motif against as many sequences sampled from the background\n");
  printf("                                 model (zoops_score = AUC, occur) and rank the motifs by it\n");
  printf("  --score-seed INT               seed of the sampled or shuffled sequences (default 1)\n");
  printf("  --score-negatives STRING       sampled: the negatives of --score-motifs come from the background model;\n");
  printf("                                 shuffled: every input sequence shuffled with its own dinucleotide counts\n");
  printf("                                 kept, for inputs of mixed composition (default sampled)\n");
  printf("                                 control: the sequences of the --background-sequences file, drawn to match the\n");
  printf("                                 input (--control-match); the seed has no effect then\n");
  printf("  --control-match STRING         gc,length | gc | length | none: what the control sequences kept as negatives\n");
  printf("                                 are matched to the input by (default gc,length; none: the whole control)\n");
  printf("  --control-match-gc-bins INT    GC content bins of the match, 1..16 (default 10)\n");
  printf("  --control-ratio INT            control sequences wanted per input sequence, 1 or above (default 1)\n");
  printf("  --control-match-report FILE    write the match per stratum (TSV: length range, GC range, input, control, kept)\n");
  printf("  --sites FILE                   write every occurrence of the motifs (TSV: sequence, position, strand,\n");
  printf("                                 score, p-value) at p-value --sites-pvalue or below\n");
  printf("  --sites-pvalue FLOAT           p-value threshold of --sites, in (0, 1] (default 1e-4)\n");
  printf("  --sites-qvalue                 add a q_value column to --sites: Benjamini-Hochberg over each motif's sites,\n");
  printf("                                 with all its scored window strands as the number of tests\n");
  printf("  --sites-qvalue-max FLOAT       write only the sites with a q-value at or below this, in (0, 1] (implies\n");
  printf("                                 --sites-qvalue)\n");
  printf("  --centrality FILE              test every motif for enrichment at the sequence centres (TSV: best site\n");
  printf("                                 per sequence at p-value --centrality-pvalue or below, binomial test)\n");
  printf("  --centrality-pvalue FLOAT      p-value threshold of a best site, in (0, 1] (default 1e-4)\n");
  printf("  --refine FILE                  re-estimate every motif from its best site per sequence, flanks included,\n");
  printf("                                 and write the refined motifs (MEME) to FILE\n");
  printf("  --refine-pvalue FLOAT          p-value threshold of a best site, in (0, 1] (default 1e-4)\n");
  printf("  --refine-flank INT             columns looked at on either side of a motif (default 8)\n");
  printf("  --refine-iterations INT        at most this many rounds of sites -> matrix (default 3)\n");
  printf("  --refine-min-ic FLOAT          information (bits) an outermost kept column needs (default 0.25)\n");
  printf("  --spacing FILE                 test every pair of motifs for co-occurrence in the same sequences and for a\n");
  printf("                                 preferred gap and orientation (TSV: best site per sequence at p-value\n");
  printf("                                 --spacing-pvalue or below, binomial tests)\n");
  printf("  --spacing-pvalue FLOAT         p-value threshold of a best site, in (0, 1] (default 1e-4)\n");
  printf("  --spacing-max-gap INT          largest gap between two sites that gets a bin of its own, 0..1024 (default 150)\n");
  printf("  --spacing-motifs INT           only the first INT motifs take part, 2..64 (default 16)\n");
  printf("  --dinuc FILE                   build a first-order model of every motif from its best site per sequence and\n");
  printf("                                 report (TSV) the mutual information of adjacent columns and the AUC of the\n");
  printf("                                 first-order against the zeroth-order model (the negatives of --score-motifs)\n");
  printf("  --dinuc-models FILE            write the models themselves to FILE (requires --dinuc)\n");
  printf("  --dinuc-pvalue FLOAT           p-value threshold of a best site, in (0, 1] (default 1e-4)\n");
  printf("  --dinuc-flank INT              columns modelled on either side of a motif (default 0)\n");
  printf("  --dinuc-alpha FLOAT            weight of the zeroth-order model in the conditionals, above 0 (default 20)\n");
  printf("  --compare FILE                 compare every motif with the motifs of --compare-db and write its matches (TSV:\n");
  printf("                                 target, offset, orientation, overlap, score, p-, E- and q-value)\n");
  printf("  --compare-db FILE              the motif database, MEME format (requires --compare, and the reverse)\n");
  printf("  --compare-evalue FLOAT         only matches with an E-value at or below it are written (default 1)\n");
  printf("  --compare-min-overlap INT      columns an alignment must span, 1..64 (default 5)\n");
  printf("  --enrich FILE                  test every motif of --enrich-db for enrichment in the input against its negatives\n");
  printf("                                 (those of --score-motifs) and write the enriched ones (TSV: best-site threshold,\n");
  printf("                                 hits, Fisher's exact test, adjusted p-, E- and q-value)\n");
  printf("  --enrich-db FILE               the motif database, MEME format (requires --enrich, and the reverse)\n");
  printf("  --enrich-pvalue FLOAT          p-value of the lowest site threshold tried, in (0, 1] (default 1e-3)\n");
  printf("  --enrich-evalue FLOAT          only motifs with an E-value at or below it are written, above 0 (default 10)\n");
  printf("  --threads INT                  accepted for compatibility\n");
  printf("  --device INT                   HIP device index (default 0)\n");
  printf("  -v INT                         verbosity\n");
  printf("  --version, -h\n\n");
}
