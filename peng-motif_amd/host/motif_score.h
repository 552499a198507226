// motif_score -- the second user-facing step of the reference's wrapper scripts/shoot_peng.py (which runs BaMMmotif2's
// FDR tool and an R script over peng_motif's output): every motif scored by how well it separates the input sequences
// from as many sequences sampled from the background model, on the device (include/pengk.h, "motif scoring").
// zoops_score / occur keep the wrapper's field names; the metric is this project's own.
#ifndef PENGK_HOST_MOTIF_SCORE_H_
#define PENGK_HOST_MOTIF_SCORE_H_

#include <cstdint>
#include <memory>
#include <vector>

#include "iupac_pattern.h"
#include "shared/BackgroundModel.h"
#include "shared/SequenceSet.h"

#include "device.h"

// The scan layout (include/pengk.h) of this rank's records of a set, on the device: built once for the scoring and the
// sites (--score-motifs, --sites).  The set must still hold its byte codes (pengk_host::keep_host_codes).
struct ScanInput {
  size_t n_local = 0;
  uint64_t n_words = 0;
  uint64_t valid_bases = 0;  // set validity bits of this rank's records (counted while the layout is built)
  pengk_host::DeviceBuffer<uint64_t> d_words;
  pengk_host::DeviceBuffer<uint32_t> d_valid;
  pengk_host::DeviceBuffer<int64_t> d_offs;
  pengk_host::DeviceBuffer<uint32_t> d_lens;
};
void build_scan_input(SequenceSet& set, ScanInput* in);
// A subset of a scan layout: a shorter pair of offs / lens arrays into the same words (include/pengk.h), which every
// scan entry accepts as it stands.  What the rounds of --erase take in place of the input's own arrays under --holdout.
struct ScanSubset {
  const int64_t* d_offs = nullptr;
  const uint32_t* d_lens = nullptr;
  size_t n = 0;
};

// one entry of the integer log-odds: clamp(lround(100 log2(p / b)), -2000, 2000)
int32_t log_odds(float p, float b);
// S[(m * PENGK_MAX_MOTIF_LEN + j) * 4 + a] = clamp(lround(100 log2(pwm / bg0)), -2000, 2000) and len[m] of every motif
// (a motif wider than PENGK_MAX_MOTIF_LEN ends the program; `who` names the step in the message)
void motif_log_odds(const std::vector<IUPACPattern*>& pats, const float* bg0, std::vector<int32_t>& S, std::vector<int32_t>& len,
                    const char* who);

// The negatives of this rank's records, in the words layout of `in` (--score-motifs and --dinuc score against the same
// ones): sampled from the background model of order K (V from bg) at the records' global indices, or, shuffled, every
// sequence's own dinucleotide-preserving shuffle with validity words of its own (valid_or_null(): NULL for a sample,
// whose bases are all valid).
// Or, --score-negatives control (motif_match.h), real sequences: the control set's own scan layout, and -- unless the
// whole control is used -- the compacted offsets / lengths of the sequences kept of it.  The consumers scan
// words() / valid_or_null() over offs(in) / lens(in) / n(in) and size what they keep per sequence by the larger count.
struct Negatives {
  pengk_host::DeviceBuffer<uint64_t> d_words;
  pengk_host::DeviceBuffer<uint32_t> d_valid;
  bool shuffled = false;
  std::unique_ptr<ScanInput> control;             // the control set (this rank's records)
  bool selected = false;                          // d_sel_offs / d_sel_lens / n_sel hold the kept ones
  pengk_host::DeviceBuffer<int64_t> d_sel_offs;
  pengk_host::DeviceBuffer<uint32_t> d_sel_lens;
  pengk_host::DeviceBuffer<uint32_t> d_sel_index;  // ... and their places among this rank's control records (--holdout splits by them)
  size_t n_sel = 0;
  const uint64_t* words() const { return control ? control->d_words.get() : d_words.get(); }
  const uint32_t* valid_or_null() const { return control ? control->d_valid.get() : shuffled ? d_valid.get() : nullptr; }
  const int64_t* offs(const ScanInput& in) const {
    return !control ? in.d_offs.get() : selected ? d_sel_offs.get() : control->d_offs.get();
  }
  const uint32_t* lens(const ScanInput& in) const {
    return !control ? in.d_lens.get() : selected ? d_sel_lens.get() : control->d_lens.get();
  }
  size_t n(const ScanInput& in) const { return !control ? in.n_local : selected ? n_sel : control->n_local; }
};
void build_negatives(SequenceSet& set, const ScanInput& in, BackgroundModel& bg, int K, uint64_t seed, bool shuffled,
                     Negatives* out);

struct MotifScore {
  double zoops_score = 0.0;  // AUC of the best window scores, input against its negatives (sampled or shuffled)
  double occur = 0.0;        // share of input sequences with a site, estimated at 1 % false positives
};

// Scores pats (in their order) over this rank's records of `set` and the negatives of their global indices; the
// histograms are summed over the ranks, so every rank gets the scores of the whole input.  K: the order of the
// sampling model (--bg-model-order), V from bg.  shuffled (--score-negatives shuffled): the negative of a sequence is
// its own dinucleotide-preserving shuffle (pengk_shuffle_sequences: same seed, same global indices) with validity bits
// of its own, not a sample of the model.  shared: negatives already built with these settings (--enrich builds them once
// for every step that scores against them), else NULL: built here.  Collective in a multi-rank run.
std::vector<MotifScore> score_motifs(const std::vector<IUPACPattern*>& pats, SequenceSet& set, const ScanInput& in,
                                     BackgroundModel& bg, int K, bool both_strands, uint64_t seed, bool shuffled = false,
                                     Negatives* shared = nullptr);

#endif
