#include "motif_sites.h"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <thread>

#include "device.h"

namespace {
// s / 100 with exactly two decimals, from the integer
void put_score(std::string& o, int32_t s) {
  char b[24];
  const long long a = s < 0 ? -(long long)s : s;
  snprintf(b, sizeof b, "%s%lld.%02lld", s < 0 ? "-" : "", a / 100, a % 100);
  o += b;
}

struct MotifInfo {
  std::string id;
  int w = 0;
  int32_t lo = 0, hi = 0, t = 0;
  std::vector<double> tail;  // P(score >= s) at tail[s - lo]
  std::vector<double> q;     // (--sites-qvalue) the q-value of a site with score s at q[s - t]
};
}  // namespace

void write_motif_sites(const std::vector<IUPACPattern*>& pats, SequenceSet& set, const ScanInput& in, BackgroundModel& bg,
                       bool both_strands, double pvalue, bool qvalues, double qvalue_max, const std::string& path) {
  using pengk_host::check;
  using pengk_host::DeviceBuffer;
  pengk_host::Lap lap("  sites: ");
  const int n_motifs = (int)pats.size();
  const size_t n_local = in.n_local;
  const float* bg0 = bg.getV()[0];
  std::vector<int32_t> S, len;
  motif_log_odds(pats, bg0, S, len, "motif sites");
  // thresholds: the smallest integer score whose tail p-value is at most `pvalue` (hi + 1: no site)
  std::vector<MotifInfo> mi(n_motifs);
  std::vector<int32_t> thr(std::max(n_motifs, 1), 0);
  for (int m = 0; m < n_motifs; ++m) {
    MotifInfo& x = mi[m];
    x.id = pats[m]->get_pattern_string();
    x.w = len[m];
    const int32_t* Sm = &S[(size_t)m * PENGK_MAX_MOTIF_LEN * 4];
    check(pengk_score_tail_pvalues(Sm, x.w, bg0, &x.lo, &x.hi, nullptr), "pengk_score_tail_pvalues");
    x.tail.resize((size_t)(x.hi - x.lo) + 1);
    check(pengk_score_tail_pvalues(Sm, x.w, bg0, &x.lo, &x.hi, x.tail.data()), "pengk_score_tail_pvalues");
    check(pengk_score_threshold(x.tail.data(), x.lo, x.hi, pvalue, &x.t), "pengk_score_threshold");
    thr[m] = x.t;
  }
  // PENGK_SITES_SCORES=FILE (diagnostic): the integer log-odds matrices as scanned -- per motif a line "index width lo hi
  // threshold", then its rows.  The PWMs of the MEME / JSON files are rounded, and written after the writers' pseudo
  // count: they do not give these integers back.
  if (const char* dump = std::getenv("PENGK_SITES_SCORES")) {
    if (pengk_host::rank() == 0) {
      FILE* f = fopen(dump, "wb");
      if (f) {
        for (int m = 0; m < n_motifs; ++m) {
          fprintf(f, "%d %d %d %d %d\n", m + 1, mi[m].w, mi[m].lo, mi[m].hi, mi[m].t);
          for (int j = 0; j < mi[m].w; ++j) {
            const int32_t* r = &S[((size_t)m * PENGK_MAX_MOTIF_LEN + j) * 4];
            fprintf(f, "%d %d %d %d\n", r[0], r[1], r[2], r[3]);
          }
        }
        fclose(f);
      }
    }
  }
  lap("thresholds");

  // where local record k lives: the chunk that holds it
  std::vector<size_t> chunk_first(set.nChunks());
  for (size_t c = 0; c < chunk_first.size(); ++c) chunk_first[c] = set.chunk(c).first;
  auto codes_of = [&](uint64_t k) -> const uint8_t* {
    const size_t c = (size_t)(std::upper_bound(chunk_first.begin(), chunk_first.end(), (size_t)k) - chunk_first.begin()) - 1;
    const SequenceChunk& ch = set.chunk(c);
    return ch.codes + ch.offs[k - ch.first];
  };

  // count, cut into slices whose records fit the budget, emit slice by slice; each motif's lines collect in out[m]
  std::vector<std::string> out(n_motifs);
  pengk_ctx* ctx = pengk_host::context();
  const int both = both_strands ? 1 : 0;
  const bool scan = n_motifs && n_local;
  DeviceBuffer<uint64_t> d_counts;
  if (scan) d_counts.resize((size_t)n_motifs * n_local);
  if (!qvalues) {
    if (scan)
      check(pengk_sites_count(ctx, in.d_words.get(), in.d_valid.get(), in.d_offs.get(), in.d_lens.get(), n_local, n_motifs,
                              S.data(), len.data(), both, thr.data(), d_counts.get()),
            "pengk_sites_count");
  } else if (n_motifs) {
    // the count pass with the histograms of the site scores and the scored window strands; their sums over the ranks
    // (integers) give every rank the same q-values
    std::vector<int32_t> hi(n_motifs);
    std::vector<uint64_t> hoffs(n_motifs);
    size_t nh = 0;
    for (int m = 0; m < n_motifs; ++m) {
      hi[m] = mi[m].hi;
      hoffs[m] = nh;
      nh += (size_t)std::max<int64_t>(0, (int64_t)mi[m].hi - mi[m].t + 1);
    }
    std::vector<long long> hist(nh + n_motifs, 0);  // the bins, then N_m
    if (scan) {
      DeviceBuffer<uint64_t> d_hist(nh + n_motifs);
      check(pengk_memset(ctx, d_hist.get(), 0, (nh + n_motifs) * sizeof(uint64_t)), "pengk_memset");
      check(pengk_sites_histograms(ctx, in.d_words.get(), in.d_valid.get(), in.d_offs.get(), in.d_lens.get(), n_local, n_motifs,
                                   S.data(), len.data(), both, thr.data(), hi.data(), hoffs.data(), d_hist.get(),
                                   d_hist.get() + nh, d_counts.get()),
            "pengk_sites_histograms");
      d_hist.download((uint64_t*)hist.data(), nh + n_motifs);
    }
    lap("count + histograms");
    SequenceSet::allreduceSum(hist.data(), hist.size());  // (integers: the ranks' sum is exact)
    bool raised = false;
    for (int m = 0; m < n_motifs; ++m) {
      MotifInfo& x = mi[m];
      const uint64_t nb = (uint64_t)std::max<int64_t>(0, (int64_t)x.hi - x.t + 1);
      x.q.resize(nb);
      check(pengk_sites_qvalues((const uint64_t*)hist.data() + hoffs[m], nb, (uint64_t)hist[nh + m],
                                nb ? x.tail.data() + (x.t - x.lo) : nullptr, x.q.data()),
            "pengk_sites_qvalues");
      if (qvalue_max > 0.0) {
        check(pengk_qvalue_threshold(x.q.data(), nb, x.t, qvalue_max, &thr[m]), "pengk_qvalue_threshold");
        raised = true;
      }
    }
    // --sites-qvalue-max: the sites at the raised thresholds (the q-values stay those of the set at `pvalue`)
    if (raised && scan)
      check(pengk_sites_count(ctx, in.d_words.get(), in.d_valid.get(), in.d_offs.get(), in.d_lens.get(), n_local, n_motifs,
                              S.data(), len.data(), both, thr.data(), d_counts.get()),
            "pengk_sites_count");
    lap("q-values");
  }
  if (scan) {
    std::vector<uint64_t> mtot(n_motifs), bounds(65), recs(64);
    uint64_t ns = 0;
    for (;;) {
      check(pengk_sites_slices(ctx, d_counts.get(), n_local, n_motifs, mtot.data(), recs.size(), bounds.data(), recs.data(), &ns),
            "pengk_sites_slices");
      if (ns <= recs.size()) break;
      recs.resize(ns);
      bounds.resize(ns + 1);
    }
    lap("count + slices");
    const uint64_t cap = std::max<uint64_t>(1, *std::max_element(recs.begin(), recs.begin() + ns));
    DeviceBuffer<pengk_site> d_sites(cap);
    std::vector<pengk_site> h(cap);
    const unsigned nt = std::min<unsigned>(16, std::max(1u, std::thread::hardware_concurrency()));
    for (uint64_t k = 0; k < ns; ++k) {
      const uint64_t i0 = bounds[k], i1 = bounds[k + 1], nr = recs[k];
      if (nr == 0) continue;
      check(pengk_sites_emit(ctx, in.d_words.get(), in.d_valid.get(), in.d_offs.get(), in.d_lens.get(), n_local, n_motifs, S.data(),
                             len.data(), both, thr.data(), d_counts.get(), i0, i1, d_sites.get(), cap),
            "pengk_sites_emit");
      d_sites.download(h.data(), nr);
      // the records are motif-major: pieces of one motif's run, formatted on up to 16 threads, appended in order
      struct Piece {
        int m;
        uint64_t b, e;
        std::string s;
      };
      std::vector<Piece> pieces;
      for (uint64_t b = 0; b < nr;) {
        const int m = (int)(h[b].motif_strand >> 1);
        uint64_t e = b;
        while (e < nr && (int)(h[e].motif_strand >> 1) == m && e - b < (1u << 16)) ++e;
        pieces.push_back(Piece{m, b, e, std::string()});
        b = e;
      }
      std::atomic<size_t> next(0);
      std::vector<std::thread> th;
      for (unsigned t = 0; t < std::min<size_t>(nt, pieces.size()); ++t)
        th.emplace_back([&] {
          char b[64];
          for (size_t p; (p = next++) < pieces.size();) {
            Piece& pc = pieces[p];
            const MotifInfo& x = mi[pc.m];
            for (uint64_t r = pc.b; r < pc.e; ++r) {
              const pengk_site& st = h[r];
              const uint64_t k = i0 + st.seq;
              const bool minus = st.motif_strand & 1;
              std::string name = set.header(k);
              const size_t cut = name.find_first_of(" \t\v\f\r");
              if (cut != std::string::npos) name.resize(cut);
              std::string& o = pc.s;
              o += std::to_string(pc.m + 1);
              o += '\t';
              o += x.id;
              o += '\t';
              o += name;
              snprintf(b, sizeof b, "\t%llu\t%llu\t%c\t", (unsigned long long)st.pos + 1, (unsigned long long)st.pos + x.w,
                       minus ? '-' : '+');
              o += b;
              put_score(o, st.score);
              snprintf(b, sizeof b, "\t%.3g\t", x.tail[(size_t)(st.score - x.lo)]);
              o += b;
              if (qvalues) {
                snprintf(b, sizeof b, "%.3g\t", x.q[(size_t)(st.score - x.t)]);
                o += b;
              }
              const uint8_t* c = codes_of(k) + st.pos;
              for (int j = 0; j < x.w; ++j) o += minus ? "TGCA"[c[x.w - 1 - j] - 1] : "ACGT"[c[j] - 1];
              o += '\n';
            }
          }
        });
      for (auto& x : th) x.join();
      for (Piece& pc : pieces) out[pc.m] += pc.s;
    }
    d_counts.release();
    lap("emit + format");
  }

  // rank 0 collects the other ranks' lines (motif by motif, in rank order) through the host channel, in bounded rounds
  const int R = pengk_host::world(), me = pengk_host::rank();
  std::vector<std::vector<uint64_t>> sizes(R, std::vector<uint64_t>(n_motifs, 0));
  std::vector<std::string> streams(R);
  if (R > 1) {
    std::vector<uint64_t> mine(std::max(n_motifs, 1), 0), all((size_t)R * std::max(n_motifs, 1));
    for (int m = 0; m < n_motifs; ++m) mine[m] = out[m].size();
    check(pengk_comm_host_allgather(mine.data(), all.data(), mine.size() * sizeof(uint64_t)), "pengk_comm_host_allgather");
    uint64_t longest = 0;
    std::vector<uint64_t> total(R, 0);
    for (int r = 0; r < R; ++r) {
      for (int m = 0; m < n_motifs; ++m) total[r] += (sizes[r][m] = all[(size_t)r * mine.size() + m]);
      longest = std::max(longest, total[r]);
    }
    std::string own;
    own.reserve(total[me]);
    for (int m = 0; m < n_motifs; ++m) own += out[m];
    const uint64_t C = std::min<uint64_t>(longest, 64ull << 20);
    if (C) {
      std::vector<char> send(C), recv((size_t)R * C);
      for (uint64_t off = 0; off < longest; off += C) {
        const uint64_t n = own.size() > off ? std::min<uint64_t>(C, own.size() - off) : 0;
        if (n) memcpy(send.data(), own.data() + off, n);
        check(pengk_comm_host_allgather(send.data(), recv.data(), C), "pengk_comm_host_allgather");
        if (me == 0)
          for (int r = 1; r < R; ++r)
            if (total[r] > off) streams[r].append(recv.data() + (size_t)r * C, std::min<uint64_t>(C, total[r] - off));
      }
    }
    lap("collected from the ranks");
  }
  if (me != 0) return;
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) {
    std::cerr << "Unable to open output file (" << path << ")!" << std::endl;
    exit(1);
  }
  const char* head = qvalues ? "#motif_index\tmotif_id\tsequence_name\tstart\tstop\tstrand\tscore\tp_value\tq_value\tmatched_sequence\n"
                             : "#motif_index\tmotif_id\tsequence_name\tstart\tstop\tstrand\tscore\tp_value\tmatched_sequence\n";
  bool ok = fwrite(head, 1, strlen(head), f) == strlen(head);
  std::vector<uint64_t> pos(R, 0);
  for (int m = 0; m < n_motifs; ++m) {
    ok = ok && fwrite(out[m].data(), 1, out[m].size(), f) == out[m].size();
    for (int r = 1; r < R; ++r) {
      ok = ok && fwrite(streams[r].data() + pos[r], 1, sizes[r][m], f) == sizes[r][m];
      pos[r] += sizes[r][m];
    }
  }
  ok = (fclose(f) == 0) && ok;
  if (!ok) {
    std::cerr << "Error: writing " << path << " failed" << std::endl;
    exit(1);
  }
  lap("written");
}
