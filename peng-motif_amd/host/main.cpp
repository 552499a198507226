// peng_motif -- command-line entry of the MI355X mirror: same flags, stdout trace, MEME / JSON output
// and exit codes as the reference's src/main.cpp; the hot loops run on the GPU through libpengk.
#include <algorithm>
#include <chrono>
#include <memory>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>

#include "Global.h"
#include "device.h"
#include "iupac_pattern.h"
#include "motif_score.h"
#include "motif_centrality.h"
#include "motif_compare.h"
#include "motif_dinuc.h"
#include "motif_dust.h"
#include "motif_dyads.h"
#include "motif_enrich.h"
#include "motif_erase.h"
#include "motif_holdout.h"
#include "motif_match.h"
#include "motif_positional.h"
#include "motif_bg_order.h"
#include "motif_strata.h"
#include "motif_refine.h"
#include "motif_spacing.h"
#include "motif_sites.h"
#include "peng.h"

namespace {
// PENGK_TIMING=1: wall-clock phase report on stderr (stdout stays the reference's trace)
struct PhaseClock {
  using clk = std::chrono::steady_clock;
  bool on = std::getenv("PENGK_TIMING") != nullptr;
  clk::time_point t0 = clk::now(), last = t0;
  void lap(const char* what) {
    if (!on) return;
    const auto now = clk::now();
    std::cerr << "[timing] " << what << ": " << std::chrono::duration<double>(now - last).count() << " s" << std::endl;
    last = now;
  }
  void total() {
    if (!on) return;
    std::cerr << "[timing] total: " << std::chrono::duration<double>(clk::now() - t0).count() << " s" << std::endl;
    // peak resident set of this process (a rank of a sharded run holds its part of the input only)
    if (FILE* f = std::fopen("/proc/self/status", "r")) {
      char line[256];
      while (std::fgets(line, sizeof line, f))
        if (std::strncmp(line, "VmHWM:", 6) == 0)
          std::cerr << "[timing] peak resident memory: " << std::atof(line + 6) / 1024.0 << " MiB" << std::endl;
        else if (std::strncmp(line, "VmRSS:", 6) == 0)  // (what is left for the kernel to take back when the process ends)
          std::cerr << "[timing] resident memory at the end: " << std::atof(line + 6) / 1024.0 << " MiB" << std::endl;
      std::fclose(f);
    }
    // how much of it sits on transparent huge pages: what the kernel has to take back page by page at exit is the rest
    if (FILE* f = std::fopen("/proc/self/smaps_rollup", "r")) {
      char line[256];
      while (std::fgets(line, sizeof line, f))
        if (std::strncmp(line, "AnonHugePages:", 14) == 0)
          std::cerr << "[timing] of it on transparent huge pages: " << std::atof(line + 14) / 1024.0 << " MiB" << std::endl;
      std::fclose(f);
    }
  }
};
}  // namespace

int main(int nargs, char** args) {
  PhaseClock clock;
  // multi-GPU run (one process per GPU under a launcher): every rank reads its byte range of the input, counts its
  // shard and follows the same deterministic control flow on the all-reduced tables; rank 0 alone reports and writes
  if (pengk_host::rank() != 0 && !std::freopen("/dev/null", "w", stdout)) return 1;
  Global::init(nargs, args);
  clock.lap("read FASTA (+ pack + upload, chunk by chunk)");
  // (the device context is being created on a helper thread since Global::init; nothing waits for it before the packed
  // sequences are ready for upload -- BasePattern's first device call -- and a machine without a gfx950 device fails
  // there, loudly: there is no CPU path)

  const int bg_model_order = std::max(Global::bgModelOrder, Global::maxOptBgModelOrder);
  // the input set doubles as the background set unless --background-sequences names another file: its (k+1)-mer
  // counters were taken by the packer while the file was read
  const pengk_host::PackedInput* packed = Global::backgroundSequenceSet == Global::inputSequenceSet
                                              ? pengk_host::packed_input(Global::inputSequenceSet, Global::patternLength)
                                              : nullptr;
  BackgroundModel* bgModel =
      packed ? new BackgroundModel(*Global::backgroundSequenceSet, bg_model_order, Global::bgModelAlpha, Global::interpolateBG,
                                   packed->bg_counts)
             : new BackgroundModel(*Global::backgroundSequenceSet, bg_model_order, Global::bgModelAlpha, Global::interpolateBG);

  clock.lap("background model");
  // (the masking, the erasing, the scoring, the sites, the centrality, the refinement, the spacing, the first-order models
  // and the database enrichment share one scan layout of the input)
  std::unique_ptr<ScanInput> scan;
  // --mask-low-complexity: round 1 (and with --discriminative its control count) sees the input behind the mask; the
  // background model above and every report below see the input as it is
  LowComplexityMask lc_mask;
  // (a pattern length outside the supported range skips the mask without a word: Peng::process ends such a run with the
  // reference's message a few lines below, as without the flag)
  if (Global::maskLowComplexity && Global::patternLength >= PENGK_MIN_W && Global::patternLength <= PENGK_MAX_W) {
    scan.reset(new ScanInput);
    build_scan_input(*Global::inputSequenceSet, scan.get());
    mask_low_complexity(*Global::inputSequenceSet, *scan, Global::discriminative ? Global::backgroundSequenceSet : nullptr,
                        Global::patternLength, Global::maskThreshold, Global::maskReportFilename, &lc_mask);
    clock.lap("low-complexity mask");
  }
  // --holdout: a share of the input (and with --discriminative of the control set) is set aside before anything is
  // counted; round 1 and the rounds of --erase see the training share, behind the mask if there is one; the background
  // model above and every other report below see the whole input
  Holdout holdout;
  HoldoutSettings holdout_settings;
  if (Global::holdoutFilename && Global::patternLength >= PENGK_MIN_W && Global::patternLength <= PENGK_MAX_W) {
    holdout_settings.fraction = Global::holdoutFraction;
    holdout_settings.threshold = Global::holdoutThreshold;
    holdout_settings.seed = Global::holdoutSeed;
    holdout_settings.pvalue = Global::holdoutPvalue;
    if (!scan) {
      scan.reset(new ScanInput);
      build_scan_input(*Global::inputSequenceSet, scan.get());
    }
    split_holdout(*Global::inputSequenceSet, *scan, lc_mask.attached ? lc_mask.input.d_valid.get() : nullptr,
                  Global::discriminative ? Global::backgroundSequenceSet : nullptr,
                  lc_mask.control_attached ? lc_mask.control.d_valid.get() : nullptr, Global::patternLength, holdout_settings,
                  &holdout);
    clock.lap("holdout split");
  }
  const ScanSubset training = holdout.input.share(0);
  // --dyads: spaced trinucleotide pairs over what round 1 counts -- the training share, behind the mask
  if (Global::dyadsFilename && Global::patternLength >= PENGK_MIN_W && Global::patternLength <= PENGK_MAX_W) {
    if (!scan) {
      scan.reset(new ScanInput);
      build_scan_input(*Global::inputSequenceSet, scan.get());
    }
    DyadSettings ds;
    ds.max_gap = Global::dyadsMaxGap;
    ds.evalue = Global::dyadsEvalue;
    ds.min_count = Global::dyadsMinCount;
    ds.top = Global::dyadsTop;
    ds.pvalue = Global::dyadsPvalue;
    RefineSettings rs;
    rs.flank = Global::refineFlank;
    rs.iterations = Global::refineIterations;
    rs.min_ic = Global::refineMinIC;
    write_dyads(*Global::inputSequenceSet, *scan, lc_mask.erase_valid(), holdout.attached ? &training : nullptr, *bgModel,
                Global::strand == Strand::BOTH_STRANDS, ds, rs, Global::dyadsFilename, Global::dyadsMotifsFilename);
    clock.lap("dyads");
  }
  // --positional: words with a position bias, over the same share behind the same mask
  if (Global::positionalFilename && Global::patternLength >= PENGK_MIN_W && Global::patternLength <= PENGK_MAX_W) {
    if (!scan) {
      scan.reset(new ScanInput);
      build_scan_input(*Global::inputSequenceSet, scan.get());
    }
    PositionalSettings ps;
    ps.width = Global::positionalWidth;
    ps.anchor = Global::positionalAnchor;
    ps.bin_size = Global::positionalBinSize;
    ps.bins = Global::positionalBins;
    ps.evalue = Global::positionalEvalue;
    ps.min_count = Global::positionalMinCount;
    ps.composition_null = Global::positionalCompositionNull;
    write_positional(*scan, lc_mask.erase_valid(), holdout.attached ? &training : nullptr, Global::strand == Strand::BOTH_STRANDS, ps,
                     Global::positionalFilename);
    clock.lap("positional");
  }
  // --stratified-background: the sweep's null becomes the mixture of the GC strata's models, weighted by the windows of
  // what round 1 counts -- the training share, behind the mask; the rounds of --erase keep it
  StratifiedNull stratified;
  if (Global::stratifiedBackground && Global::patternLength >= PENGK_MIN_W && Global::patternLength <= PENGK_MAX_W &&
      Global::patternLength % 2 == 0) {
    if (!scan) {
      scan.reset(new ScanInput);
      build_scan_input(*Global::inputSequenceSet, scan.get());
    }
    StratifiedSettings ss;
    ss.gc_bins = Global::stratifiedGcBins;
    ss.min_bases = Global::stratifiedMinBases;
    ss.report_path = Global::stratifiedReportFilename;
    build_stratified_null(*scan, lc_mask.erase_valid(), holdout.attached ? &training : nullptr,
                          Global::backgroundSequenceSet != Global::inputSequenceSet ? Global::backgroundSequenceSet : nullptr,
                          Global::patternLength, *bgModel, ss, &stratified);
    pengk_host::set_stratified_null(&stratified);
    clock.lap("stratified background");
  }
  // --high-order-background: the sweep's null becomes a Markov model of order 3 .. 5 of the background set as it was read
  // -- no mask, no hold-out, like the one model above; the rounds of --erase keep it
  HighOrderNull high_order;
  if (Global::highOrderBackground && Global::patternLength >= PENGK_MIN_W && Global::patternLength <= PENGK_MAX_W &&
      Global::patternLength % 2 == 0) {
    if (!scan) {
      scan.reset(new ScanInput);
      build_scan_input(*Global::inputSequenceSet, scan.get());
    }
    HighOrderSettings hs;
    hs.order = Global::highOrderBackground;
    hs.alpha = Global::highOrderAlpha;
    hs.report_path = Global::highOrderReportFilename;
    build_high_order_null(*scan, Global::backgroundSequenceSet != Global::inputSequenceSet ? Global::backgroundSequenceSet : nullptr, hs,
                          &high_order);
    pengk_host::set_high_order_null(&high_order);
    clock.lap("high-order background");
  }
  Peng peng(Global::strand, Global::bgModelOrder, Global::maxOptBgModelOrder, Global::inputSequenceSet, bgModel);

  PengParameters params;
  params.max_pattern_length = Global::patternLength;
  params.zscore_threshold = Global::zscoreThreshold;
  params.count_threshold = Global::countThreshold;
  params.pseudo_counts = Global::pseudoCounts;
  params.opt_score_type = Global::optScoreType;
  params.use_em = Global::useEm;
  params.em_saturation_factor = Global::emSaturationFactor;
  params.em_min_threshold = Global::emMinThreshold;
  params.em_max_iterations = Global::emMaxIterations;
  params.use_merging = Global::useMerging;
  params.bit_factor_merge_threshold = Global::mergeBitfactorThreshold;
  params.max_merged_length = Global::max_merged_length;
  params.adv_pwm = Global::useAdvPWM;
  params.enrich_pseudocount_factor = Global::enrich_pseudocount_factor;
  params.minimum_processed_motifs = Global::minimum_processed_motifs;
  params.filter_neighbors = Global::filter_neighbors;
  params.max_optimized_patterns = Global::maximum_optimized_patterns;

  std::vector<IUPACPattern*> result;
  if (Global::eraseFilename)
    std::cout << "erase mode: up to " << Global::eraseRounds << " further round" << (Global::eraseRounds == 1 ? "" : "s")
              << " on the input with the found motifs' sites (p-value <= " << Global::erasePvalue << ") masked" << std::endl
              << (lc_mask.attached ? "erase round 1: the input behind the low-complexity mask" : "erase round 1: the input as it is")
              << std::endl;
  peng.process(params, result);
  if (lc_mask.attached || holdout.attached) pengk_host::override_packed_input(nullptr, nullptr);
  clock.lap("process (count, sweep, hill-climb, PWMs, EM, merging)");
  peng.filter_redundancy(Global::mergeBitfactorThreshold, result);
  std::vector<MotifScore> scores;
  if (!scan && (Global::scoreMotifs || Global::sitesFilename || Global::centralityFilename || Global::refineFilename ||
      Global::spacingFilename || Global::dinucFilename || Global::enrichFilename || Global::eraseFilename)) {
    scan.reset(new ScanInput);
    build_scan_input(*Global::inputSequenceSet, scan.get());
  }
  // --erase: further rounds on the masked input; their motifs join the list, and every report below sees the union over
  // the unmasked scan input
  if (Global::eraseFilename) {
    run_erase_rounds(peng, params, result, *Global::inputSequenceSet, *scan, *bgModel, Global::strand == Strand::BOTH_STRANDS,
                     Global::erasePvalue, Global::eraseRounds, Global::mergeBitfactorThreshold, Global::eraseFilename,
                     lc_mask.erase_valid(), holdout.attached ? &training : nullptr);
    clock.lap("erase rounds");
  }
  if (lc_mask.control_attached || holdout.control_attached) pengk_host::override_control_input(nullptr, nullptr);
  pengk_host::set_stratified_null(nullptr);
  pengk_host::set_high_order_null(nullptr);
  if (holdout.attached) pengk_host::override_sequence_count(nullptr, 0);
  // (--enrich scores against the negatives of --score-motifs and --dinuc: with it they are built once, for all three)
  // (--score-negatives control: the control set, matched to the input, serves whichever of the three is asked for)
  std::unique_ptr<Negatives> negatives;
  if (Global::scoreNegativesControl && (Global::scoreMotifs || Global::dinucFilename || Global::enrichFilename || holdout.attached)) {
    negatives.reset(new Negatives);
    MatchSettings ms;
    ms.gc = Global::controlMatchGc;
    ms.length = Global::controlMatchLength;
    ms.gc_bins = Global::controlMatchGcBins;
    ms.ratio = Global::controlRatio;
    if (Global::controlMatchReportFilename) ms.report_path = Global::controlMatchReportFilename;
    build_control_negatives(*Global::backgroundSequenceSet, *scan, ms, negatives.get());
    clock.lap("control negatives");
  } else if (Global::enrichFilename || holdout.attached) {
    negatives.reset(new Negatives);
    build_negatives(*Global::inputSequenceSet, *scan, *bgModel, Global::bgModelOrder, Global::scoreSeed,
                    Global::scoreNegativesShuffled, negatives.get());
  }
  if (Global::scoreMotifs) {
    // the writers' order first, then stable by zoops_score descending (scripts/shoot_peng.py re-ranks the motifs so)
    std::sort(result.begin(), result.end(), sort_IUPAC_patterns);
    scores = score_motifs(result, *Global::inputSequenceSet, *scan, *bgModel, Global::bgModelOrder,
                          Global::strand == Strand::BOTH_STRANDS, Global::scoreSeed, Global::scoreNegativesShuffled,
                          negatives.get());
    std::vector<size_t> order(result.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return scores[a].zoops_score > scores[b].zoops_score; });
    std::vector<IUPACPattern*> r2;
    std::vector<MotifScore> s2;
    for (size_t i : order) {
      r2.push_back(result[i]);
      s2.push_back(scores[i]);
    }
    result.swap(r2);
    scores.swap(s2);
    clock.lap("score");
  }
  const std::vector<MotifScore>* sc = Global::scoreMotifs ? &scores : nullptr;
  // the MEME file's order: as it is, or as the writers sort it (the same sort of the same vector: the same order)
  std::vector<IUPACPattern*> meme_order(result);
  if (!sc && (Global::sitesFilename || Global::centralityFilename || Global::refineFilename || Global::spacingFilename ||
              Global::dinucFilename || holdout.attached))
    std::sort(meme_order.begin(), meme_order.end(), sort_IUPAC_patterns);
  if (holdout.attached) {
    write_motif_holdout(meme_order, *scan, holdout, *negatives, Global::backgroundSequenceSet, *bgModel,
                        Global::strand == Strand::BOTH_STRANDS, holdout_settings, Global::holdoutFilename);
    clock.lap("holdout");
  }
  if (Global::sitesFilename) {
    write_motif_sites(meme_order, *Global::inputSequenceSet, *scan, *bgModel, Global::strand == Strand::BOTH_STRANDS,
                      Global::sitesPvalue, Global::sitesQvalue, Global::sitesQvalueMax, Global::sitesFilename);
    clock.lap("sites");
  }
  if (Global::centralityFilename) {
    write_motif_centrality(meme_order, *Global::inputSequenceSet, *scan, *bgModel, Global::strand == Strand::BOTH_STRANDS,
                           Global::centralityPvalue, Global::centralityFilename);
    clock.lap("centrality");
  }
  if (Global::refineFilename) {
    RefineSettings rs;
    rs.pvalue = Global::refinePvalue;
    rs.flank = Global::refineFlank;
    rs.iterations = Global::refineIterations;
    rs.min_ic = Global::refineMinIC;
    write_refined_motifs(meme_order, *Global::inputSequenceSet, *scan, *bgModel, Global::strand == Strand::BOTH_STRANDS, rs,
                         Global::refineFilename);
    clock.lap("refine");
  }
  if (Global::spacingFilename) {
    write_motif_spacing(meme_order, *Global::inputSequenceSet, *scan, *bgModel, Global::strand == Strand::BOTH_STRANDS,
                        Global::spacingPvalue, Global::spacingMaxGap, Global::spacingMotifs, Global::spacingFilename);
    clock.lap("spacing");
  }
  if (Global::dinucFilename) {
    DinucSettings ds;
    ds.pvalue = Global::dinucPvalue;
    ds.flank = Global::dinucFlank;
    ds.alpha = Global::dinucAlpha;
    ds.bg_order = Global::bgModelOrder;
    ds.seed = Global::scoreSeed;
    ds.shuffled = Global::scoreNegativesShuffled;
    write_motif_dinuc(meme_order, *Global::inputSequenceSet, *scan, *bgModel, Global::strand == Strand::BOTH_STRANDS, ds,
                      Global::dinucFilename, Global::dinucModelsFilename ? Global::dinucModelsFilename : "", negatives.get());
    clock.lap("dinuc");
  }
  if (Global::enrichFilename) {
    EnrichSettings es;
    es.pvalue = Global::enrichPvalue;
    es.evalue = Global::enrichEvalue;
    write_motif_enrich(Global::enrichDb, *scan, *negatives, *bgModel,
                       Global::strand == Strand::BOTH_STRANDS, es, Global::enrichFilename);
    clock.lap("enrich");
  }
  negatives.reset();
  scan.reset();
  // (the comparison reads neither the sequences nor their scan layout: rank 0 alone runs it)
  if (Global::compareFilename && pengk_host::rank() == 0) {
    std::vector<IUPACPattern*> q(result);
    if (!sc) std::sort(q.begin(), q.end(), sort_IUPAC_patterns);
    CompareSettings cs;
    cs.evalue = Global::compareEvalue;
    cs.min_overlap = Global::compareMinOverlap;
    write_motif_compare(q, Global::compareDb, Global::strand == Strand::BOTH_STRANDS, cs, Global::compareFilename);
    clock.lap("compare");
  }
  if (pengk_host::rank() == 0) {
    if (Global::outputFilename) peng.printShortMeme(result, Global::outputFilename, bgModel, sc);
    if (Global::jsonFilename) peng.printJson(result, Global::jsonFilename, VERSION_NUMBER, bgModel, sc);
  }

  for (IUPACPattern* p : result) delete p;
  delete bgModel;
  clock.lap("output");
  // Everything this process owns -- gigabytes of sequence codes, the pinned table mirrors, the device buffers and the
  // HIP context -- dies with it; walking it all to hand it back piece by piece cost a quarter of the whole run on a
  // 2 GB input (0.25 of 1.1 s).  The outputs are closed and flushed, the device is idle: leave.
  // (PENGK_FULL_TEARDOWN=1 keeps the orderly release, e.g. under a leak checker.)
  pengk_host::check(pengk_synchronize(pengk_host::context()), "pengk_synchronize");
  pengk_host::finish_ranks();
  const char* full_teardown = std::getenv("PENGK_FULL_TEARDOWN");
  if (full_teardown && std::atoi(full_teardown)) {
    Global::destruct();
    pengk_host::shutdown();
    clock.lap("cleanup");
    clock.total();
    return 0;
  }
  clock.total();
  std::cout.flush();
  std::cerr.flush();
  fflush(nullptr);
  _exit(0);
}
