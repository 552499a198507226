#include "motif_holdout.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>

#include "Global.h"
#include "device.h"

namespace {
using pengk_host::check;
using pengk_host::DeviceBuffer;

void write_or_die(const std::string& path, const void* p, size_t bytes, const char* what) {
  FILE* f = fopen(path.c_str(), "wb");
  const bool ok = f && fwrite(p, 1, bytes, f) == bytes;
  if (!f || (fclose(f) != 0) || !ok) {
    std::cerr << "Error: " << what << ": cannot write " << path << std::endl;
    exit(1);
  }
}

// s / 100 with exactly two decimals, from the integer (as --sites writes its scores)
std::string score_str(int32_t s) {
  char b[24];
  const long long a = s < 0 ? -(long long)s : s;
  snprintf(b, sizeof b, "%s%lld.%02lld", s < 0 ? "-" : "", a / 100, a % 100);
  return b;
}

// the two shares of n sequences given by offs / lens (global indices seq0 + (index ? index[i] : i))
void split_set(uint64_t seq0, size_t n, const uint32_t* d_index, const int64_t* d_offs, const uint32_t* d_lens,
               const HoldoutSettings& hs, SplitSet* out) {
  for (int c = 0; c < 2; ++c) {
    out->d_offs[c].resize(std::max<size_t>(n, 1));
    out->d_lens[c].resize(std::max<size_t>(n, 1));
    out->d_index[c].resize(std::max<size_t>(n, 1));
  }
  uint64_t n0 = 0, n1 = 0;
  check(pengk_split_sequences(pengk_host::context(), hs.seed, seq0, n, hs.threshold, d_index, d_offs, d_lens, nullptr,
                              out->d_offs[0].get(), out->d_lens[0].get(), out->d_index[0].get(), &n0, out->d_offs[1].get(),
                              out->d_lens[1].get(), out->d_index[1].get(), &n1),
        "pengk_split_sequences");
  out->n[0] = (size_t)n0;
  out->n[1] = (size_t)n1;
}

// one share of a scan layout in the count layout
void pack_share(const ScanInput& in, const uint32_t* valid, const ScanSubset& s, int W, DeviceBuffer<uint64_t>* d_words,
                DeviceBuffer<uint64_t>* d_items, pengk_host::PackedInput* packed) {
  pengk_ctx* ctx = pengk_host::context();
  DeviceBuffer<uint64_t> d_seq_base(s.n), d_seq_item(s.n);
  pengk_packed pk;
  check(pengk_pack_scan_sizes(ctx, valid, s.d_offs, s.d_lens, s.n, W, 0, d_seq_base.get(), d_seq_item.get(), &pk),
        "pengk_pack_scan_sizes");
  d_words->resize(pk.n_words);
  d_items->resize(pk.n_items + 1);
  check(pengk_pack_scan(ctx, in.d_words.get(), valid, s.d_offs, s.d_lens, s.n, W, 0, d_seq_base.get(), d_seq_item.get(),
                        d_words->get(), pk.n_words, d_items->get(), pk.n_items),
        "pengk_pack_scan");
  check(pengk_synchronize(ctx), "pengk_synchronize");  // (the offset arrays leave scope here)
  packed->W = W;
  packed->item_windows = pk.item_windows;
  packed->d_words = d_words->get();
  packed->d_items = d_items->get();
  packed->n_words = pk.n_words;
  packed->n_items = pk.n_items;
  packed->n_windows = pk.n_windows;
  packed->max_bin_bound = pk.max_bin_bound;
  packed->all_whole = pk.all_whole;
}

void sum_over_ranks(uint64_t* v, size_t n) {
  if (pengk_host::world() > 1) check(pengk_comm_host_allreduce_u64(v, n), "pengk_comm_host_allreduce_u64");
}
}  // namespace

void split_holdout(SequenceSet& input, const ScanInput& scan, const uint32_t* valid, SequenceSet* control,
                   const uint32_t* control_valid, int W, const HoldoutSettings& hs, Holdout* out) {
  pengk_host::Lap lap("  holdout: ");
  split_set(input.getLocalBase(), scan.n_local, nullptr, scan.d_offs.get(), scan.d_lens.get(), hs, &out->input);
  pack_share(scan, valid ? valid : scan.d_valid.get(), out->input.share(0), W, &out->d_words, &out->d_items, &out->packed);
  lap("input: split + pack of the training share");
  uint64_t tot[4] = {out->input.n[0], out->input.n[1], 0, 0};
  if (control) {
    out->control_scan.reset(new ScanInput);
    build_scan_input(*control, out->control_scan.get());
    const ScanInput& cs = *out->control_scan;
    split_set(control->getLocalBase(), cs.n_local, nullptr, cs.d_offs.get(), cs.d_lens.get(), hs, &out->control);
    pack_share(cs, control_valid ? control_valid : cs.d_valid.get(), out->control.share(0), W, &out->d_cwords, &out->d_citems,
               &out->control_packed);
    tot[2] = out->control.n[0];
    tot[3] = out->control.n[1];
    out->control_scan.reset();  // (the count layout stays; the scan layout of the control has done its duty)
    lap("control: scan layout + split + pack of the training share");
  }
  sum_over_ranks(tot, 4);
  out->n_train = tot[0];
  out->n_hold = tot[1];
  char f[32];
  snprintf(f, sizeof f, "%.6g", hs.fraction);
  std::cout << "holdout (fraction " << f << ", seed " << hs.seed << "): " << tot[1] << " of " << tot[0] + tot[1]
            << " input sequences set aside, motifs are searched on the other " << tot[0];
  if (control) std::cout << "; control set: " << tot[3] << " of " << tot[2] + tot[3] << " set aside";
  std::cout << std::endl;
  if (out->n_train == 0) Global::exitWithError("--holdout: no input sequence is left to search");
  pengk_host::override_packed_input(&input, &out->packed);
  pengk_host::override_sequence_count(&input, (size_t)out->n_train);
  out->attached = true;
  if (control) {
    pengk_host::override_control_input(control, &out->control_packed);
    out->control_attached = true;
  }
}

void write_motif_holdout(const std::vector<IUPACPattern*>& pats, const ScanInput& in, const Holdout& ho, Negatives& neg,
                         SequenceSet* control, BackgroundModel& bg, bool both_strands, const HoldoutSettings& hs,
                         const std::string& path) {
  pengk_host::Lap lap("  holdout: ");
  pengk_ctx* ctx = pengk_host::context();
  const int n_motifs = (int)pats.size();
  const size_t ML = PENGK_MAX_MOTIF_LEN;
  const float* bg0 = bg.getV()[0];
  const char* dump_dir = pengk_host::rank() == 0 ? std::getenv("PENGK_DUMP_TABLES") : nullptr;

  // the negatives' two shares: sampled and shuffled ones have the input's offs / lens and indices; a control set is split
  // by its sequences' indices in the control file, whether it was matched or not
  SplitSet neg_split;
  ScanSubset sets[4] = {ho.input.share(0), ho.input.share(0), ho.input.share(1), ho.input.share(1)};  // train +, train -, hold +, hold -
  if (neg.control) {
    split_set(control->getLocalBase(), neg.n(in), neg.selected ? neg.d_sel_index.get() : nullptr, neg.offs(in), neg.lens(in), hs,
              &neg_split);
    sets[1] = neg_split.share(0);
    sets[3] = neg_split.share(1);
  }
  lap("negatives' shares");

  // log-odds, thresholds (the smallest score with a tail at or below hs.pvalue; hi + 1: no bin)
  std::vector<int32_t> S, len, thr(std::max(n_motifs, 1), 0), hi(std::max(n_motifs, 1), 0), lo(std::max(n_motifs, 1), 0);
  motif_log_odds(pats, bg0, S, len, "holdout");
  std::vector<uint64_t> hoffs(n_motifs + 1, 0);
  for (int m = 0; m < n_motifs; ++m) {
    const int32_t* Sm = &S[(size_t)m * ML * 4];
    check(pengk_score_tail_pvalues(Sm, len[m], bg0, &lo[m], &hi[m], nullptr), "pengk_score_tail_pvalues");
    std::vector<double> tail((size_t)(hi[m] - lo[m]) + 1);
    check(pengk_score_tail_pvalues(Sm, len[m], bg0, &lo[m], &hi[m], tail.data()), "pengk_score_tail_pvalues");
    check(pengk_score_threshold(tail.data(), lo[m], hi[m], hs.pvalue, &thr[m]), "pengk_score_threshold");
    hoffs[m + 1] = hoffs[m] + (uint64_t)(hi[m] - thr[m] + 1);
  }
  if (dump_dir) {  // test hook: what the four scans are made with
    const std::string d(dump_dir);
    write_or_die(d + "/holdout_S.i32", S.data(), (size_t)n_motifs * ML * 4 * sizeof(int32_t), "PENGK_DUMP_TABLES");
    write_or_die(d + "/holdout_len.i32", len.data(), (size_t)n_motifs * sizeof(int32_t), "PENGK_DUMP_TABLES");
    write_or_die(d + "/holdout_thr.i32", thr.data(), (size_t)n_motifs * sizeof(int32_t), "PENGK_DUMP_TABLES");
  }

  // per set: the motifs' bins, then their scored counters, then the set's sequences
  const uint64_t nh = hoffs[n_motifs], per_set = nh + (uint64_t)n_motifs + 1;
  std::vector<uint64_t> hist(4 * per_set, 0);
  if (n_motifs) {
    DeviceBuffer<uint64_t> d_hist(4 * per_set);
    check(pengk_memset(ctx, d_hist.get(), 0, 4 * per_set * sizeof(uint64_t)), "pengk_memset");
    const int both = both_strands ? 1 : 0;
    for (int s = 0; s < 4; ++s) {
      const bool negative = s & 1;
      check(pengk_motif_enrich(ctx, negative ? neg.words() : in.d_words.get(), negative ? neg.valid_or_null() : in.d_valid.get(),
                               sets[s].d_offs, sets[s].d_lens, sets[s].n, n_motifs, S.data(), len.data(), both, thr.data(), hi.data(),
                               hoffs.data(), d_hist.get() + s * per_set, d_hist.get() + s * per_set + nh),
            "pengk_motif_enrich");
    }
    d_hist.download(hist.data(), 4 * per_set);
  }
  for (int s = 0; s < 4; ++s) hist[s * per_set + nh + n_motifs] = sets[s].n;
  lap("scans + histograms");
  sum_over_ranks(hist.data(), hist.size());
  if (pengk_host::rank() != 0) return;

  char line[512];
  snprintf(line, sizeof line, "# holdout fraction %.6g seed %llu train_pos %llu train_neg %llu hold_pos %llu hold_neg %llu\n", hs.fraction,
           hs.seed, (unsigned long long)hist[0 * per_set + nh + n_motifs], (unsigned long long)hist[1 * per_set + nh + n_motifs],
           (unsigned long long)hist[2 * per_set + nh + n_motifs], (unsigned long long)hist[3 * per_set + nh + n_motifs]);
  std::string o = line;
  o += "motif\tconsensus\tthreshold_bits\ttrain_pos_hits\ttrain_neg_hits\ttrain_log10_adj_p\thold_pos_hits\thold_pos_scored\t"
       "hold_neg_hits\thold_neg_scored\thold_log10_p\thold_log10_E\thold_enrichment\n";
  const double ln = n_motifs ? std::log10((double)n_motifs) : 0.0;
  for (int m = 0; m < n_motifs; ++m) {
    pengk_holdout h;
    const uint64_t* b = hist.data() + hoffs[m];
    check(pengk_holdout_summary(b, b + per_set, b + 2 * per_set, b + 3 * per_set, hoffs[m + 1] - hoffs[m], thr[m], hist[nh + m],
                                hist[per_set + nh + m], hist[2 * per_set + nh + m], hist[3 * per_set + nh + m], &h),
          "pengk_holdout_summary");
    std::string cons;
    for (int j = 0; j < len[m]; ++j) {  // the best letter of every column, the first of equals
      const int32_t* c = &S[((size_t)m * ML + j) * 4];
      int best = 0;
      for (int a = 1; a < 4; ++a)
        if (c[a] > c[best]) best = a;
      cons += "ACGT"[best];
    }
    const std::string id = pats[m]->get_pattern_string();
    std::vector<char> buf(id.size() + cons.size() + 384);
    snprintf(buf.data(), buf.size(), "%s\t%s\t%s\t%llu\t%llu\t%.3f\t%llu\t%llu\t%llu\t%llu\t%.3f\t%.3f\t%.3f\n", id.c_str(), cons.c_str(),
             score_str(h.threshold).c_str(), (unsigned long long)h.train_pos_hits, (unsigned long long)h.train_neg_hits,
             h.train_log10_adj_pvalue, (unsigned long long)h.hold_pos_hits, (unsigned long long)hist[2 * per_set + nh + m],
             (unsigned long long)h.hold_neg_hits, (unsigned long long)hist[3 * per_set + nh + m], h.hold_log10_pvalue,
             std::min(0.0, h.hold_log10_pvalue + ln), h.hold_enrichment);
    o += buf.data();
  }
  write_or_die(path, o.data(), o.size(), "--holdout");
  lap("written");
}
