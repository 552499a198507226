#include "motif_score.h"

#include <algorithm>
#include <cmath>
#include <iostream>
#include <thread>

#include "device.h"

int32_t log_odds(float p, float b) {
  const double v = 100.0 * std::log2((double)p / (double)b);  // (p = 0: -inf)
  return (int32_t)std::lround(std::max(-2000.0, std::min(2000.0, v)));
}

void motif_log_odds(const std::vector<IUPACPattern*>& pats, const float* bg0, std::vector<int32_t>& S, std::vector<int32_t>& len,
                    const char* who) {
  const int n_motifs = (int)pats.size();
  S.assign((size_t)std::max(n_motifs, 1) * PENGK_MAX_MOTIF_LEN * 4, 0);
  len.assign(std::max(n_motifs, 1), 0);
  for (int m = 0; m < n_motifs; ++m) {
    const int w = (int)pats[m]->get_pattern_length();
    if (w > PENGK_MAX_MOTIF_LEN) {
      std::cerr << "Error: " << who << ": motif width " << w << " above " << PENGK_MAX_MOTIF_LEN << std::endl;
      exit(1);
    }
    len[m] = w;
    float** pwm = pats[m]->get_pwm();
    for (int j = 0; j < w; ++j)
      for (int a = 0; a < 4; ++a) S[((size_t)m * PENGK_MAX_MOTIF_LEN + j) * 4 + a] = log_odds(pwm[j][a], bg0[a]);
  }
}

void build_scan_input(SequenceSet& set, ScanInput* in) {
  using pengk_host::check;
  pengk_host::Lap lap("  scan layout: ");
  if (set.codesReleased()) {
    std::cerr << "Error: motif scan: the sequences are no longer held on the host" << std::endl;
    exit(1);
  }
  // scan layout of this rank's records, chunk by chunk (the chunks' words are disjoint: built by several threads)
  const size_t NC = set.nChunks(), n_local = set.getLocalN();
  std::vector<uint64_t> word0(NC + 1, 0);
  for (size_t c = 0; c < NC; ++c) {
    uint64_t nw = 0;
    if (set.chunk(c).n == 0) {
      word0[c + 1] = word0[c];
      continue;
    }
    check(pengk_scan_layout_words(set.chunk(c).offs.data(), (int64_t)set.chunk(c).n, &nw), "pengk_scan_layout_words");
    word0[c + 1] = word0[c] + nw;
  }
  const uint64_t n_words = std::max<uint64_t>(word0[NC], 1);
  raw_vector<uint64_t> words(n_words);
  raw_vector<uint32_t> valid(n_words);
  raw_vector<int64_t> offs(std::max<size_t>(n_local, 1));
  raw_vector<uint32_t> lens(std::max<size_t>(n_local, 1));
  {
    unsigned nt = std::min<unsigned>(16, std::max(1u, std::thread::hardware_concurrency()));
    nt = (unsigned)std::max<size_t>(1, std::min<size_t>(nt, NC));
    std::vector<std::thread> th;
    std::vector<int> rc(nt, PENGK_OK);
    std::vector<uint64_t> ones(nt, 0);  // the valid bases of each thread's chunks (--mask-low-complexity reports them)
    for (unsigned t = 0; t < nt; ++t)
      th.emplace_back([&, t] {
        for (size_t c = t; c < NC && rc[t] == PENGK_OK; c += nt) {
          const SequenceChunk& ch = set.chunk(c);
          if (ch.n == 0) continue;
          rc[t] = pengk_scan_layout_build(ch.codes, ch.offs.data(), (int64_t)ch.n, word0[c], words.data(), valid.data(),
                                          offs.data() + ch.first, lens.data() + ch.first);
          uint64_t n1 = 0;
          for (uint64_t w = word0[c]; w < word0[c + 1]; ++w) n1 += (unsigned)__builtin_popcount(valid[w]);
          ones[t] += n1;
        }
      });
    for (auto& x : th) x.join();
    for (int r : rc) check(r, "pengk_scan_layout_build");
    in->valid_bases = 0;
    for (uint64_t n1 : ones) in->valid_bases += n1;
  }
  lap("built");
  in->n_local = n_local;
  in->n_words = n_words;
  in->d_words.resize(n_words);
  in->d_valid.resize(n_words);
  in->d_offs.resize(offs.size());
  in->d_lens.resize(lens.size());
  in->d_words.upload(words.data(), n_words);
  in->d_valid.upload(valid.data(), n_words);
  in->d_offs.upload(offs.data(), offs.size());
  in->d_lens.upload(lens.data(), lens.size());
  lap("uploaded");
}

void build_negatives(SequenceSet& set, const ScanInput& in, BackgroundModel& bg, int K, uint64_t seed, bool shuffled,
                     Negatives* out) {
  using pengk_host::check;
  pengk_ctx* ctx = pengk_host::context();
  const size_t n_local = in.n_local;
  out->shuffled = shuffled;
  out->d_words.resize(in.n_words);
  if (shuffled) {
    out->d_valid.resize(in.n_words);  // (a shuffle carries the sequence's other letters along)
    check(pengk_shuffle_sequences(ctx, seed, set.getLocalBase(), n_local, in.d_words.get(), in.d_valid.get(), in.d_offs.get(),
                                  in.d_lens.get(), out->d_words.get(), out->d_valid.get()),
          "pengk_shuffle_sequences");
    return;
  }
  // sampling thresholds of the contexts of orders 0..K
  std::vector<uint32_t> thr;
  for (int k = 0; k <= K; ++k)
    for (int ctx = 0; ctx < (1 << (2 * k)); ++ctx) {
      double c = 0.0;
      for (int b = 0; b < 3; ++b) {
        c += (double)bg.getV()[k][ctx * 4 + b];
        const double t = std::floor(c * 4294967296.0);
        thr.push_back(t >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)t);
      }
    }
  check(pengk_sample_background(ctx, seed, set.getLocalBase(), n_local, in.d_offs.get(), in.d_lens.get(), K, thr.data(),
                                out->d_words.get()),
        "pengk_sample_background");
}

std::vector<MotifScore> score_motifs(const std::vector<IUPACPattern*>& pats, SequenceSet& set, const ScanInput& in,
                                     BackgroundModel& bg, int K, bool both_strands, uint64_t seed, bool shuffled,
                                     Negatives* shared) {
  using pengk_host::check;
  using pengk_host::DeviceBuffer;
  pengk_host::Lap lap("  score: ");
  const int n_motifs = (int)pats.size();
  std::vector<MotifScore> out(n_motifs);
  const size_t n_local = in.n_local;
  // (the sampled path stays silent, as it was)
  if (shuffled && pengk_host::rank() == 0)
    std::cerr << "score: negatives are dinucleotide-preserving shuffles of the input sequences (seed " << seed << ")" << std::endl;

  // log-odds against the background letter frequencies, score ranges, histogram offsets
  const float* bg0 = bg.getV()[0];
  std::vector<int32_t> S, len, lo(std::max(n_motifs, 1), 0), hi(std::max(n_motifs, 1), 0);
  motif_log_odds(pats, bg0, S, len, "motif scoring");
  std::vector<uint64_t> hoffs(n_motifs + 1, 0);
  for (int m = 0; m < n_motifs; ++m) {
    for (int j = 0; j < len[m]; ++j) {
      const int32_t* r = &S[((size_t)m * PENGK_MAX_MOTIF_LEN + j) * 4];
      lo[m] += std::min(std::min(r[0], r[1]), std::min(r[2], r[3]));
      hi[m] += std::max(std::max(r[0], r[1]), std::max(r[2], r[3]));
    }
    hoffs[m + 1] = hoffs[m] + (uint64_t)(hi[m] - lo[m] + 2);
  }
  const uint64_t nh = std::max<uint64_t>(hoffs[n_motifs], 1);
  DeviceBuffer<uint64_t> d_hist(2 * nh);
  const size_t n_neg = shared ? shared->n(in) : n_local;  // (a control set brings its own number of sequences)
  DeviceBuffer<int32_t> d_best((size_t)std::max(n_motifs, 1) * std::max<size_t>(std::max(n_local, n_neg), 1));
  pengk_ctx* ctx = pengk_host::context();
  check(pengk_memset(ctx, d_hist.get(), 0, 2 * nh * sizeof(uint64_t)), "pengk_memset");
  const int both = both_strands ? 1 : 0;
  check(pengk_motif_scan(ctx, in.d_words.get(), in.d_valid.get(), in.d_offs.get(), in.d_lens.get(), n_local, n_motifs, S.data(),
                         len.data(), both, d_best.get()),
        "pengk_motif_scan");
  check(pengk_score_histograms(ctx, n_motifs, d_best.get(), n_local, lo.data(), hi.data(), hoffs.data(), d_hist.get()),
        "pengk_score_histograms");
  Negatives own;
  if (!shared) build_negatives(set, in, bg, K, seed, shuffled, &own);
  Negatives& neg = shared ? *shared : own;
  check(pengk_motif_scan(ctx, neg.words(), neg.valid_or_null(), neg.offs(in), neg.lens(in), n_neg, n_motifs, S.data(), len.data(),
                         both, d_best.get()),
        "pengk_motif_scan");
  check(pengk_score_histograms(ctx, n_motifs, d_best.get(), n_neg, lo.data(), hi.data(), hoffs.data(), d_hist.get() + nh),
        "pengk_score_histograms");
  std::vector<long long> hist(2 * nh);
  d_hist.download((uint64_t*)hist.data(), 2 * nh);
  lap(neg.control ? "scan + histograms" : shuffled ? "shuffle + scan + histograms" : "sample + scan + histograms");
  SequenceSet::allreduceSum(hist.data(), hist.size());  // (integers: the ranks' sum is exact)
  for (int m = 0; m < n_motifs; ++m)
    check(pengk_score_summary((const uint64_t*)hist.data() + hoffs[m], (const uint64_t*)hist.data() + nh + hoffs[m],
                              hoffs[m + 1] - hoffs[m], &out[m].zoops_score, &out[m].occur),
          "pengk_score_summary");
  lap("summed over the ranks");
  return out;
}
