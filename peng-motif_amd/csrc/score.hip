// score.hip -- motif scoring against sampled background sequences (the step scripts/shoot_peng.py adds after peng_motif:
// every found motif scored by how well it separates the input sequences from random ones).  DESIGN.md 10.
//
//   scan layout    host builder: byte codes -> 2-bit words + validity words, every sequence from a 32-base boundary
//   sampler        one thread per sequence, order-K Markov chain, counter-based draws: shards reproduce one process
//   shuffle         one thread per sequence, its 25 doublet counters in LDS: a negative with the
//                  sequence's own dinucleotide counts (shuffle_core.h)
//   scan           motif groups whose 4-mer chunk tables fit in LDS; one thread per sequence slides a 64-base look-ahead
//                  buffer over its words, so chunk c of the window is byte c of the buffer (scan_walk.h)
//   histograms     per-motif integer histograms of the best scores (LDS bins for the top of the range, global beyond)
//   staging        the chunk tables, records and groups of a launch's motifs, for every file that walks the scan layout
// The other walks of the scan layout: sites.hip (--sites, --sites-qvalue, --enrich), site_stats.hip (--centrality,
// --spacing, --refine, --dinuc), erase.hip (--erase); the summaries on the host: score_stats.cpp.
#include <string.h>

#include <algorithm>
#include <vector>

#include "pengk_internal.h"
#include "scan_walk.h"
#include "shuffle_core.h"

namespace pengk {
using namespace scan;  // the shared walk and its records (scan_walk.h)
namespace {

constexpr int HIST_LDS_BINS = 16384;   // the top of a motif's score range is counted in LDS (64 KiB), the rest globally

// pengk_motif_scan: the best window score of every motif on every sequence
template <bool BOTH>
__global__ __launch_bounds__(SCAN_THREADS) void motif_scan_kernel(const uint64_t* __restrict__ words,
                                                                  const uint32_t* __restrict__ valid,
                                                                  const int64_t* __restrict__ offs,
                                                                  const uint32_t* __restrict__ lens, uint64_t n_seq,
                                                                  const int32_t* __restrict__ tables,
                                                                  const MotifRec* __restrict__ recs,
                                                                  const GroupRec* __restrict__ groups,
                                                                  int32_t* __restrict__ best_out) {
  __shared__ int32_t tab[SCAN_TABLES * 256];
  __shared__ MotifRec mrec[SCAN_MAX_MOTIFS];
  const GroupRec g = groups[blockIdx.y];
  load_group(g, tables, recs, tab, mrec);
  __syncthreads();
  for (uint64_t i = blockIdx.x * (uint64_t)SCAN_THREADS + threadIdx.x; i < n_seq; i += (uint64_t)gridDim.x * SCAN_THREADS) {
    const uint32_t L = lens[i];
    const uint64_t w0 = (uint64_t)offs[i] >> 5;
    BestVisit<BOTH> v{mrec, best_out, n_seq, i, {}};
    walk_sequence<BOTH>(words + w0, valid ? valid + w0 : nullptr, L, tab, mrec, g.m1 - g.m0, v);
  }
}

struct Thresholds {
  uint32_t t[21 * 3];
};

__global__ __launch_bounds__(256) void sample_background_kernel(uint64_t seed, uint64_t seq0, uint64_t n_seq,
                                                                const int64_t* __restrict__ offs,
                                                                const uint32_t* __restrict__ lens, int K, Thresholds th,
                                                                uint64_t* __restrict__ words) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n_seq; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t L = lens[i];
    uint64_t* wp = words + ((uint64_t)offs[i] >> 5);
    const uint64_t ctr0 = (seq0 + i) << 32;
    uint32_t hist = 0;  // the last two sampled bases, big-endian (the older one more significant)
    for (uint32_t j = 0; 32u * j < L; ++j) {
      uint64_t v = 0;
      const uint32_t n = L - 32u * j < 32u ? L - 32u * j : 32u;
      for (uint32_t k = 0; k < n; ++k) {
        const uint32_t p = 32u * j + k;
        const uint32_t r = (uint32_t)(mix64(seed + 0x9E3779B97F4A7C15ull * (ctr0 + p + 1)) >> 32);
        const int kk = p < (uint32_t)K ? (int)p : K;
        const uint32_t* T = th.t + 3 * (kk == 0 ? 0u : kk == 1 ? 1u + (hist & 3u) : 5u + (hist & 15u));
        const uint32_t b = (uint32_t)(r >= T[0]) + (uint32_t)(r >= T[1]) + (uint32_t)(r >= T[2]);
        hist = ((hist << 2) | b) & 15u;
        v |= (uint64_t)b << (2 * k);
      }
      wp[j] = v;
    }
  }
}

// pengk_shuffle_sequences: one thread per sequence, grid-stride like the sampler.  The 25 counters of a thread are
// indexed at run time, so they live in LDS (25 KiB per workgroup; a private array would go to scratch): counter k of
// thread t at dword k * SHUFFLE_THREADS + t, bank t % 32 whatever k is.  No barrier: a thread touches its own only.
constexpr int SHUFFLE_THREADS = 256;
constexpr int SHUFFLE_BLOCKS_PER_CU = 6;  // the workgroups whose counters fit in a CU's 160 KiB of LDS

__global__ __launch_bounds__(SHUFFLE_THREADS) void shuffle_sequences_kernel(uint64_t seed, uint64_t seq0, uint64_t n_seq,
                                                                            const uint64_t* __restrict__ words,
                                                                            const uint32_t* __restrict__ valid,
                                                                            const int64_t* __restrict__ offs,
                                                                            const uint32_t* __restrict__ lens,
                                                                            uint64_t* __restrict__ out_words,
                                                                            uint32_t* __restrict__ out_valid) {
  __shared__ uint32_t cnt[25 * SHUFFLE_THREADS];
  for (uint64_t i = blockIdx.x * (uint64_t)SHUFFLE_THREADS + threadIdx.x; i < n_seq; i += (uint64_t)gridDim.x * SHUFFLE_THREADS) {
    const uint32_t L = lens[i];
    if (L == 0) continue;
    const uint64_t w0 = (uint64_t)offs[i] >> 5;
    shuffle_sequence<SHUFFLE_THREADS>(seed, seq0 + i, words + w0, valid ? valid + w0 : nullptr, L, cnt + threadIdx.x,
                                      out_words + w0, out_valid ? out_valid + w0 : nullptr);
  }
}

// pengk_synth_sequences' bases (count.hip, synth_words_kernel), one word of the scan layout per thread
__global__ __launch_bounds__(256) void synth_scan_kernel(uint64_t seed, uint64_t seq0, uint64_t n_seq, uint32_t L,
                                                         uint64_t* __restrict__ words, uint32_t* __restrict__ valid,
                                                         int64_t* __restrict__ offs, uint32_t* __restrict__ lens) {
  const uint64_t motif = 2ull | (1ull << 2) | (3ull << 4) | (2ull << 6) | (0ull << 8) | (2ull << 10) | (3ull << 12) |
                         (1ull << 14) | (0ull << 16) | (3ull << 18);  // GCTGAGTCAT
  const uint32_t wps = (L + 31u) >> 5;
  const uint64_t n_words = n_seq * wps;
  for (uint64_t w = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; w < n_words; w += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t si = w / wps;
    const uint32_t wj = (uint32_t)(w % wps);
    const uint64_t n = seq0 + si;
    const bool planted = L >= 10 && mix64(seed ^ 0xA5A5A5A5ull ^ (n + 1)) % 10 == 0;
    const uint64_t q = planted ? mix64(seed ^ 0x5A5A5A5Aull ^ (n + 1)) % (L - 9) : 0;
    uint64_t v = 0;
    uint32_t vm = 0;
    for (uint32_t k = 0; k < 32u; ++k) {
      const uint32_t j = 32u * wj + k;
      if (j >= L) break;
      uint64_t d = mix64(seed + 0x9E3779B97F4A7C15ull * (n * (uint64_t)L + j + 1)) >> 62;
      if (planted && j >= q && j < q + 10) d = (motif >> (2 * (j - q))) & 3ull;
      v |= d << (2 * k);
      vm |= 1u << k;
    }
    words[w] = v;
    valid[w] = vm;
    if (wj == 0) {
      offs[si] = (int64_t)(si * wps * 32u);
      lens[si] = L;
    }
  }
}

template <bool LDS>
__global__ __launch_bounds__(HIST_THREADS) void score_hist_kernel(const int32_t* __restrict__ best, uint64_t n_seq,
                                                                  const int32_t* __restrict__ lo_hi,
                                                                  const uint64_t* __restrict__ hoffs,
                                                                  unsigned long long* __restrict__ hist) {
  __shared__ uint32_t h[LDS ? HIST_LDS_BINS : 1];
  const int m = blockIdx.y;
  const int32_t lo = lo_hi[2 * m], hi = lo_hi[2 * m + 1];
  const int64_t nb = (int64_t)hi - lo + 2;
  // LDS bins: [b_lds, nb) -- the top of the range, where the best window score of a sequence lands
  const int64_t b_lds = nb > HIST_LDS_BINS ? nb - HIST_LDS_BINS : 0;
  unsigned long long* H = hist + hoffs[m];
  if (LDS) {
    for (int t = threadIdx.x; t < HIST_LDS_BINS; t += HIST_THREADS) h[t] = 0;
    __syncthreads();
  }
  const int32_t* B = best + (uint64_t)m * n_seq;
  for (uint64_t i = blockIdx.x * (uint64_t)HIST_THREADS + threadIdx.x; i < n_seq; i += (uint64_t)gridDim.x * HIST_THREADS) {
    const int32_t s = B[i];
    int64_t b = s == PENGK_SCORE_SENTINEL ? 0 : 1 + (int64_t)(s < lo ? lo : s > hi ? hi : s) - lo;
    if (LDS && b >= b_lds) atomicAdd(&h[b - b_lds], 1u);
    else atomicAdd(&H[b], 1ull);
  }
  if (LDS) {
    __syncthreads();
    for (int64_t t = threadIdx.x; t < nb - b_lds; t += HIST_THREADS)
      if (h[t]) atomicAdd(&H[b_lds + t], (unsigned long long)h[t]);
  }
}

// The staging both table models share: motif records and groups by the grouping rule (scan::fit_motif), the tables by
// fill(m, w, strand, chunk, tables), which appends the Model::STRIDE ints of one chunk table; then all of it -- and h_thr
// when given -- into ctx->d_score.
template <class Model, class Fill>
int stage_groups(pengk_ctx* ctx, int n_motifs, const int32_t* h_len, int strands, const int32_t* h_thr, StagedMotifs* out,
                 Fill fill) {
  std::vector<int32_t> tables;
  std::vector<MotifRec> recs;
  std::vector<GroupRec> groups;
  for (int m = 0; m < n_motifs; ++m) {
    const int w = h_len[m], nch = (w + 3) / 4;
    const MotifFit fit = fit_motif(groups.empty() ? 0 : groups.back().n_ints, w, strands, Model::STRIDE);
    if (groups.empty() || fit.opens) groups.push_back(GroupRec{(int32_t)recs.size(), (int32_t)recs.size(), (int32_t)tables.size(), 0});
    GroupRec& g = groups.back();
    recs.push_back(MotifRec{g.n_ints, w, nch, m});
    g.m1 = (int32_t)recs.size();
    g.n_ints += fit.need;
    for (int st = 0; st < strands; ++st)
      for (int c = 0; c < nch; ++c) fill(m, w, st, c, tables);
  }
  const size_t tb = tables.size() * sizeof(int32_t), rb = recs.size() * sizeof(MotifRec), gb = groups.size() * sizeof(GroupRec);
  const size_t hb = h_thr ? (size_t)n_motifs * sizeof(int32_t) : 0;
  int rc = ensure_scratch(ctx, &ctx->d_score, &ctx->score_bytes, tb + rb + gb + hb);
  if (rc) return rc;
  char* base = (char*)ctx->d_score;
  std::vector<char> staged(tb + rb + gb + hb);
  memcpy(staged.data(), tables.data(), tb);
  memcpy(staged.data() + tb, recs.data(), rb);
  memcpy(staged.data() + tb + rb, groups.data(), gb);
  if (hb) memcpy(staged.data() + tb + rb + gb, h_thr, hb);
  // (synchronous: the staging vector dies with this call, and the scratch may still be read by an earlier scan)
  PENGK_HIP(hipStreamSynchronize(ctx->stream));
  PENGK_HIP(hipMemcpy(base, staged.data(), staged.size(), hipMemcpyHostToDevice));
  out->tables = (const int32_t*)base;
  out->recs = (const MotifRec*)(base + tb);
  out->groups = (const GroupRec*)(base + tb + rb);
  out->thr = hb ? (const int32_t*)(base + tb + rb + gb) : nullptr;
  out->n_groups = (int)groups.size();
  return PENGK_OK;
}

}  // namespace

// (declared in scan_walk.h: every file that walks the scan layout stages its motifs and sizes its grids the same way)
int grid_for(pengk_ctx* ctx, uint64_t work, uint32_t per_block, uint32_t per_cu) {
  const uint64_t need = (work + per_block - 1) / per_block;
  const uint64_t cap = (uint64_t)ctx->num_cu * per_cu;
  return (int)std::max<uint64_t>(1, std::min(need, cap));
}

int check_motifs(const char* who, int n_motifs, const int32_t* h_S, const int32_t* h_len) {
  for (int m = 0; m < n_motifs; ++m) {
    if (h_len[m] < 1 || h_len[m] > PENGK_MAX_MOTIF_LEN)
      return fail(PENGK_ERR_ARG, "%s: motif %d has width %d (1..%d)", who, m, h_len[m], PENGK_MAX_MOTIF_LEN);
    for (int j = 0; j < h_len[m] * 4; ++j) {
      const int32_t v = h_S[(size_t)m * PENGK_MAX_MOTIF_LEN * 4 + j];
      if (v < -2000 || v > 2000) return fail(PENGK_ERR_ARG, "%s: motif %d: log-odds %d outside [-2000, 2000]", who, m, v);
    }
  }
  return PENGK_OK;
}

int stage_motifs(pengk_ctx* ctx, int n_motifs, const int32_t* h_S, const int32_t* h_len, int strands, const int32_t* h_thr,
                 StagedMotifs* out) {
  return stage_groups<Order0>(ctx, n_motifs, h_len, strands, h_thr, out, [&](int m, int w, int st, int c, std::vector<int32_t>& tables) {
    const int32_t* S = h_S + (size_t)m * PENGK_MAX_MOTIF_LEN * 4;
    for (int idx = 0; idx < 256; ++idx) {
      int32_t v = 0;
      for (int k = 0; k < 4 && 4 * c + k < w; ++k) {
        const int j = 4 * c + k, a = (idx >> (2 * k)) & 3;
        v += st == 0 ? S[j * 4 + a] : S[(w - 1 - j) * 4 + (3 - a)];  // reverse complement: S_rc[j][a] = S[w-1-j][3-a]
      }
      tables.push_back(v);
    }
  });
}

// In window positions j the + strand has the single term S0[x_0] at j = 0 and the pair terms D[j][4 x_{j-1} + x_j],
// j = 1 .. w - 1; the - strand, y_j = 3 - x_{w-1-j}, has S0[3 - x_{w-1}] at j = w - 1 and the pair terms
// D[w - j][4 (3 - x_j) + (3 - x_{j-1})].  A chunk's table sums the terms whose positions lie inside it (positions at or
// beyond w add nothing: the entries repeat over them).
int stage_motifs_dinuc(pengk_ctx* ctx, int n_motifs, const int32_t* h_S0, const int32_t* h_D, const int32_t* h_len, int strands,
                       StagedMotifs* out) {
  return stage_groups<Order1>(ctx, n_motifs, h_len, strands, nullptr, out, [&](int m, int w, int st, int c, std::vector<int32_t>& tables) {
    const int32_t* S0 = h_S0 + (size_t)m * 4;
    const int32_t* D = h_D + (size_t)m * PENGK_MAX_MOTIF_LEN * 16;
    // the pair term of positions (j - 1, j) holding the bases (a, b), j = 1 .. w - 1
    auto pair = [&](int j, int a, int b) -> int32_t {
      return st == 0 ? D[j * 16 + 4 * a + b] : D[(w - j) * 16 + 4 * (3 - b) + (3 - a)];
    };
    for (int idx = 0; idx < 256; ++idx) {
      int32_t v = 0;
      for (int k = 0; k < 4 && 4 * c + k < w; ++k) {
        const int j = 4 * c + k, b = (idx >> (2 * k)) & 3;
        if (st == 0 && j == 0) v += S0[b];
        if (st == 1 && j == w - 1) v += S0[3 - b];
        if (k > 0) v += pair(j, (idx >> (2 * k - 2)) & 3, b);
      }
      tables.push_back(v);
    }
    for (int px = 0; px < 16; ++px) tables.push_back(c > 0 ? pair(4 * c, px & 3, px >> 2) : 0);
  });
}

}  // namespace pengk

using namespace pengk;

extern "C" {

int pengk_scan_layout_words(const int64_t* h_code_offs, int64_t n_seq, uint64_t* n_words) {
  if (!h_code_offs || !n_words || n_seq < 0) return fail(PENGK_ERR_ARG, "pengk_scan_layout_words: bad argument");
  uint64_t nw = 0;
  for (int64_t i = 0; i < n_seq; ++i) {
    const int64_t L = h_code_offs[i + 1] - h_code_offs[i];
    if (L < 0 || L > 0xFFFFFFFFll) return fail(PENGK_ERR_ARG, "pengk_scan_layout_words: sequence %lld has length %lld", (long long)i, (long long)L);
    nw += ((uint64_t)L + 31) / 32;
  }
  *n_words = nw;
  return PENGK_OK;
}

int pengk_scan_layout_build(const uint8_t* h_codes, const int64_t* h_code_offs, int64_t n_seq, uint64_t word0,
                            uint64_t* h_words, uint32_t* h_valid, int64_t* h_offs, uint32_t* h_lens) {
  if (!h_code_offs || n_seq < 0 || (n_seq && (!h_codes || !h_words || !h_valid || !h_offs || !h_lens)))
    return fail(PENGK_ERR_ARG, "pengk_scan_layout_build: bad argument");
  uint64_t w = word0;
  for (int64_t i = 0; i < n_seq; ++i) {
    const int64_t L = h_code_offs[i + 1] - h_code_offs[i];
    if (L < 0 || L > 0xFFFFFFFFll) return fail(PENGK_ERR_ARG, "pengk_scan_layout_build: sequence %lld has length %lld", (long long)i, (long long)L);
    const uint8_t* c = h_codes + h_code_offs[i];
    h_offs[i] = (int64_t)(w * 32);
    h_lens[i] = (uint32_t)L;
    for (int64_t p = 0; p < L; p += 32, ++w) {
      uint64_t v = 0;
      uint32_t vm = 0;
      const int n = L - p < 32 ? (int)(L - p) : 32;
      for (int k = 0; k < n; ++k) {
        const uint32_t x = c[p + k];
        const bool ok = x >= 1 && x <= 4;
        v |= (uint64_t)(ok ? x - 1 : 0) << (2 * k);
        vm |= (uint32_t)ok << k;
      }
      h_words[w] = v;
      h_valid[w] = vm;
    }
  }
  return PENGK_OK;
}

int pengk_synth_scan_sequences(pengk_ctx* ctx, uint64_t seed, uint64_t seq0, uint64_t n_seq, uint32_t L, uint64_t* d_words,
                               uint32_t* d_valid, int64_t* d_offs, uint32_t* d_lens) {
  if (!ctx || !d_words || !d_valid || !d_offs || !d_lens || L == 0)
    return fail(PENGK_ERR_ARG, "pengk_synth_scan_sequences: bad argument");
  SCORE_ENTER(ctx);
  if (n_seq == 0) return PENGK_OK;
  const uint64_t n_words = n_seq * ((L + 31u) / 32u);
  hipLaunchKernelGGL(synth_scan_kernel, dim3(grid_for(ctx, n_words, 256, 16)), dim3(256), 0, ctx->stream, seed, seq0, n_seq, L,
                     d_words, d_valid, d_offs, d_lens);
  PENGK_HIP(hipGetLastError());
  return PENGK_OK;
}

int pengk_sample_background(pengk_ctx* ctx, uint64_t seed, uint64_t seq0, uint64_t n_seq, const int64_t* d_offs,
                            const uint32_t* d_lens, int K, const uint32_t* h_thresholds, uint64_t* d_words) {
  if (!ctx || K < 0 || K > 2 || !h_thresholds || (n_seq && (!d_offs || !d_lens || !d_words)))
    return fail(PENGK_ERR_ARG, "pengk_sample_background: bad argument");
  if (seq0 + n_seq > (1ull << 32)) return fail(PENGK_ERR_ARG, "pengk_sample_background: sequence index beyond 2^32");
  SCORE_ENTER(ctx);
  if (n_seq == 0) return PENGK_OK;
  Thresholds th;
  memset(&th, 0, sizeof th);
  const int n_ctx = K == 0 ? 1 : K == 1 ? 5 : 21;
  memcpy(th.t, h_thresholds, (size_t)n_ctx * 3 * sizeof(uint32_t));
  hipLaunchKernelGGL(sample_background_kernel, dim3(grid_for(ctx, n_seq, 256, 16)), dim3(256), 0, ctx->stream, seed, seq0, n_seq,
                     d_offs, d_lens, K, th, d_words);
  PENGK_HIP(hipGetLastError());
  return PENGK_OK;
}

int pengk_shuffle_sequences(pengk_ctx* ctx, uint64_t seed, uint64_t seq0, uint64_t n_seq, const uint64_t* d_words,
                            const uint32_t* d_valid, const int64_t* d_offs, const uint32_t* d_lens, uint64_t* d_out_words,
                            uint32_t* d_out_valid) {
  if (!ctx || (n_seq && (!d_words || !d_offs || !d_lens || !d_out_words || (d_valid && !d_out_valid))))
    return fail(PENGK_ERR_ARG, "pengk_shuffle_sequences: bad argument");
  if (n_seq && (d_out_words == d_words || (d_out_valid && d_out_valid == d_valid)))
    return fail(PENGK_ERR_ARG, "pengk_shuffle_sequences: the output buffers must differ from the input");
  if (seq0 + n_seq > (1ull << 32)) return fail(PENGK_ERR_ARG, "pengk_shuffle_sequences: sequence index beyond 2^32");
  SCORE_ENTER(ctx);
  if (n_seq == 0) return PENGK_OK;
  hipLaunchKernelGGL(shuffle_sequences_kernel, dim3(grid_for(ctx, n_seq, SHUFFLE_THREADS, SHUFFLE_BLOCKS_PER_CU)),
                     dim3(SHUFFLE_THREADS), 0, ctx->stream, seed, seq0, n_seq, d_words, d_valid, d_offs, d_lens, d_out_words,
                     d_out_valid);
  PENGK_HIP(hipGetLastError());
  return PENGK_OK;
}

int pengk_motif_scan(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                     const uint32_t* d_lens, uint64_t n_seq, int n_motifs, const int32_t* h_S, const int32_t* h_len,
                     int both_strands, int32_t* d_best) {
  if (!ctx || n_motifs < 0 || (n_motifs && (!h_S || !h_len)) || (n_seq && n_motifs && (!d_words || !d_offs || !d_lens || !d_best)))
    return fail(PENGK_ERR_ARG, "pengk_motif_scan: bad argument");
  int rc = check_motifs("pengk_motif_scan", n_motifs, h_S, h_len);
  if (rc) return rc;
  SCORE_ENTER(ctx);
  if (n_seq == 0 || n_motifs == 0) return PENGK_OK;
  StagedMotifs st;
  rc = stage_motifs(ctx, n_motifs, h_S, h_len, both_strands ? 2 : 1, nullptr, &st);
  if (rc) return rc;
  const dim3 grid(grid_for(ctx, n_seq, SCAN_THREADS, 8), (unsigned)st.n_groups);
  by_strands(both_strands, [&](auto B) {
    hipLaunchKernelGGL(motif_scan_kernel<decltype(B)::value>, grid, dim3(SCAN_THREADS), 0, ctx->stream, d_words, d_valid, d_offs,
                       d_lens, n_seq, st.tables, st.recs, st.groups, d_best);
  });
  PENGK_HIP(hipGetLastError());
  return PENGK_OK;
}

int pengk_score_histograms(pengk_ctx* ctx, int n_motifs, const int32_t* d_best, uint64_t n_seq, const int32_t* h_lo,
                           const int32_t* h_hi, const uint64_t* h_hist_offs, uint64_t* d_hist) {
  if (!ctx || n_motifs < 0 || (n_motifs && (!h_lo || !h_hi || !h_hist_offs || !d_hist)) || (n_seq && n_motifs && !d_best))
    return fail(PENGK_ERR_ARG, "pengk_score_histograms: bad argument");
  for (int m = 0; m < n_motifs; ++m)
    if (h_hi[m] < h_lo[m]) return fail(PENGK_ERR_ARG, "pengk_score_histograms: motif %d: hi < lo", m);
  SCORE_ENTER(ctx);
  if (n_seq == 0 || n_motifs == 0) return PENGK_OK;
  std::vector<char> staged((size_t)n_motifs * (2 * sizeof(int32_t) + sizeof(uint64_t)));
  int32_t* lh = (int32_t*)staged.data();
  for (int m = 0; m < n_motifs; ++m) {
    lh[2 * m] = h_lo[m];
    lh[2 * m + 1] = h_hi[m];
  }
  memcpy(staged.data() + (size_t)n_motifs * 2 * sizeof(int32_t), h_hist_offs, (size_t)n_motifs * sizeof(uint64_t));
  int rc = ensure_scratch(ctx, &ctx->d_misc, &ctx->misc_bytes, staged.size());
  if (rc) return rc;
  PENGK_HIP(hipStreamSynchronize(ctx->stream));
  PENGK_HIP(hipMemcpy(ctx->d_misc, staged.data(), staged.size(), hipMemcpyHostToDevice));
  const int32_t* d_lh = (const int32_t*)ctx->d_misc;
  const uint64_t* d_ho = (const uint64_t*)((char*)ctx->d_misc + (size_t)n_motifs * 2 * sizeof(int32_t));
  // blocks per motif: enough to fill the device once over all motifs, each block flushing its LDS bins once
  const uint64_t per_motif = std::max<uint64_t>(1, std::min<uint64_t>((n_seq + HIST_THREADS - 1) / HIST_THREADS,
                                                                      (uint64_t)ctx->num_cu * 2 / (uint64_t)n_motifs + 1));
  const dim3 grid((unsigned)per_motif, (unsigned)n_motifs);
  const bool lds = n_seq >= (uint64_t)HIST_THREADS * 16;  // (a small set: the global atomics alone, no LDS bins to flush)
  if (lds)
    hipLaunchKernelGGL(score_hist_kernel<true>, grid, dim3(HIST_THREADS), 0, ctx->stream, d_best, n_seq, d_lh, d_ho,
                       (unsigned long long*)d_hist);
  else
    hipLaunchKernelGGL(score_hist_kernel<false>, grid, dim3(HIST_THREADS), 0, ctx->stream, d_best, n_seq, d_lh, d_ho,
                       (unsigned long long*)d_hist);
  PENGK_HIP(hipGetLastError());
  return PENGK_OK;
}

}  // extern "C"
