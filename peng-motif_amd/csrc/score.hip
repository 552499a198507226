// score.hip -- motif scoring against sampled background sequences (the step scripts/shoot_peng.py adds after peng_motif:
// every found motif scored by how well it separates the input sequences from random ones).  DESIGN.md 10.
//
//   scan layout    host builder: byte codes -> 2-bit words + validity words, every sequence from a 32-base boundary
//   sampler        one thread per sequence, order-K Markov chain, counter-based draws: shards reproduce one process
//   scan           motif groups whose 4-mer chunk tables fit in LDS; one thread per sequence slides a 64-base look-ahead
//                  buffer over its words, so chunk c of the window is byte c of the buffer
//   histograms     per-motif integer histograms of the best scores (LDS bins for the top of the range, global beyond)
#include <string.h>

#include <algorithm>
#include <vector>

#include "pengk_internal.h"

namespace pengk {
namespace {

constexpr int SCAN_THREADS = 256;
constexpr int SCAN_TABLES = 40;        // 4-mer chunk tables (256 int each) of one motif group in LDS: 40 KiB, 4 groups per CU
constexpr int SCAN_MAX_MOTIFS = SCAN_TABLES;  // (a motif needs at least one table)
constexpr int MAX_CHUNKS = PENGK_MAX_MOTIF_LEN / 4;
constexpr int SCAN_PASS = 1;           // motifs scored side by side in one pass over a sequence (4 measured 1.4x slower: DESIGN.md 10)
constexpr int HIST_THREADS = 256;
constexpr int HIST_LDS_BINS = 16384;   // the top of a motif's score range is counted in LDS (64 KiB), the rest globally

// the splitmix64 finalizer of count.hip's synthetic input (mix64 there), restated for the sampler
__device__ __forceinline__ uint64_t mix64(uint64_t x) {
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

struct MotifRec {
  int32_t off;    // first table of the motif within its group's tables (ints)
  int32_t w;      // width
  int32_t nch;    // chunk tables per strand: ceil(w / 4)
  int32_t m;      // motif index (row of d_best)
};
struct GroupRec {
  int32_t m0, m1;       // records [m0, m1)
  int32_t table0;       // first int of the group's tables in the table array
  int32_t n_ints;       // their number
};

__device__ __forceinline__ uint32_t byte_of(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3, int c) {
  const uint32_t v = c < 4 ? b0 : c < 8 ? b1 : c < 12 ? b2 : b3;  // (c is a compile-time constant after unrolling)
  return (v >> (8 * (c & 3))) & 0xFFu;
}

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
  for (int t = threadIdx.x; t < g.n_ints; t += SCAN_THREADS) tab[t] = tables[g.table0 + t];
  for (int t = threadIdx.x; t < g.m1 - g.m0; t += SCAN_THREADS) mrec[t] = recs[g.m0 + t];
  __syncthreads();
  for (uint64_t i = blockIdx.x * (uint64_t)SCAN_THREADS + threadIdx.x; i < n_seq; i += (uint64_t)gridDim.x * SCAN_THREADS) {
    const uint32_t L = lens[i];
    const uint64_t w0 = (uint64_t)offs[i] >> 5;
    const uint64_t* wp = words + w0;
    const uint32_t* vp = valid ? valid + w0 : nullptr;
    const uint32_t nw = (L + 31u) >> 5;
    auto ldw = [&](uint32_t j) -> uint64_t { return j < nw ? wp[j] : 0ull; };
    auto ldv = [&](uint32_t j) -> uint32_t {
      if (j >= nw) return 0u;
      if (vp) return vp[j];
      const uint32_t rem = L - 32u * j;
      return rem >= 32u ? 0xFFFFFFFFu : ((1u << rem) - 1u);
    };
    // SCAN_PASS motifs per pass over the sequence: the buffer's upkeep per base is shared by them
    for (int r0 = 0; r0 < g.m1 - g.m0; r0 += SCAN_PASS) {
      const int np = g.m1 - g.m0 - r0 < SCAN_PASS ? g.m1 - g.m0 - r0 : SCAN_PASS;
      uint64_t wmask[SCAN_PASS];
      int nch[SCAN_PASS], best[SCAN_PASS];
      const int32_t* tf[SCAN_PASS];
      int wmin = PENGK_MAX_MOTIF_LEN;
#pragma unroll
      for (int q = 0; q < SCAN_PASS; ++q) {
        const MotifRec mr = mrec[r0 + (q < np ? q : 0)];
        wmask[q] = mr.w >= 64 ? ~0ull : ((1ull << mr.w) - 1ull);
        nch[q] = mr.nch;
        tf[q] = tab + mr.off;
        best[q] = PENGK_SCORE_SENTINEL;
        wmin = q < np && mr.w < wmin ? mr.w : wmin;
      }
      // (a window past the sequence's end has invalid bits: the passes' wider motifs need no bound of their own)
      const uint32_t nwin = L >= (uint32_t)wmin ? L - (uint32_t)wmin + 1u : 0u;
      // look-ahead buffer: bases s .. s+63 of the sequence (b0 low), their validity bits in vb
      const uint64_t x0 = ldw(0), x1 = ldw(1);
      uint32_t b0 = (uint32_t)x0, b1 = (uint32_t)(x0 >> 32), b2 = (uint32_t)x1, b3 = (uint32_t)(x1 >> 32);
      uint64_t vb = (uint64_t)ldv(0) | ((uint64_t)ldv(1) << 32);
      for (uint32_t s = 0, j = 2; s < nwin; ++j) {
        uint64_t fw = ldw(j);
        uint32_t fv = ldv(j);
        const uint32_t cnt = nwin - s < 32u ? nwin - s : 32u;
        for (uint32_t k = 0; k < cnt; ++k) {
#pragma unroll
          for (int q = 0; q < SCAN_PASS; ++q) {
            if (q < np && (vb & wmask[q]) == wmask[q]) {
              int32_t sf = 0, sr = 0;
#pragma unroll
              for (int c = 0; c < MAX_CHUNKS; ++c) {
                if (c < nch[q]) {
                  const uint32_t idx = byte_of(b0, b1, b2, b3, c);
                  sf += tf[q][c * 256 + idx];
                  if (BOTH) sr += tf[q][(nch[q] + c) * 256 + idx];
                }
              }
              best[q] = max(best[q], BOTH ? max(sf, sr) : sf);
            }
          }
          b0 = __builtin_amdgcn_alignbit(b1, b0, 2);
          b1 = __builtin_amdgcn_alignbit(b2, b1, 2);
          b2 = __builtin_amdgcn_alignbit(b3, b2, 2);
          b3 = __builtin_amdgcn_alignbit((uint32_t)fw, b3, 2);
          fw >>= 2;
          vb = (vb >> 1) | ((uint64_t)(fv & 1u) << 63);
          fv >>= 1;
        }
        s += cnt;
      }
#pragma unroll
      for (int q = 0; q < SCAN_PASS; ++q)
        if (q < np) best_out[(uint64_t)mrec[r0 + q].m * n_seq + i] = best[q];
    }
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

int grid_for(pengk_ctx* ctx, uint64_t work, uint32_t per_block, uint32_t per_cu) {
  const uint64_t need = (work + per_block - 1) / per_block;
  const uint64_t cap = (uint64_t)ctx->num_cu * per_cu;
  return (int)std::max<uint64_t>(1, std::min(need, cap));
}

}  // namespace
}  // namespace pengk

using namespace pengk;

#define SCORE_ENTER(ctx)                   \
  do {                                     \
    int rc_enter_ = ::pengk::enter(ctx);   \
    if (rc_enter_) return rc_enter_;       \
  } while (0)

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

int pengk_motif_scan(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                     const uint32_t* d_lens, uint64_t n_seq, int n_motifs, const int32_t* h_S, const int32_t* h_len,
                     int both_strands, int32_t* d_best) {
  if (!ctx || n_motifs < 0 || (n_motifs && (!h_S || !h_len)) || (n_seq && n_motifs && (!d_words || !d_offs || !d_lens || !d_best)))
    return fail(PENGK_ERR_ARG, "pengk_motif_scan: bad argument");
  for (int m = 0; m < n_motifs; ++m) {
    if (h_len[m] < 1 || h_len[m] > PENGK_MAX_MOTIF_LEN)
      return fail(PENGK_ERR_ARG, "pengk_motif_scan: motif %d has width %d (1..%d)", m, h_len[m], PENGK_MAX_MOTIF_LEN);
    for (int j = 0; j < h_len[m] * 4; ++j) {
      const int32_t v = h_S[(size_t)m * PENGK_MAX_MOTIF_LEN * 4 + j];
      if (v < -2000 || v > 2000) return fail(PENGK_ERR_ARG, "pengk_motif_scan: motif %d: log-odds %d outside [-2000, 2000]", m, v);
    }
  }
  SCORE_ENTER(ctx);
  if (n_seq == 0 || n_motifs == 0) return PENGK_OK;
  const int strands = both_strands ? 2 : 1;
  // chunk tables, motif records and groups (greedy, in motif order)
  std::vector<int32_t> tables;
  std::vector<MotifRec> recs;
  std::vector<GroupRec> groups;
  for (int m = 0; m < n_motifs; ++m) {
    const int w = h_len[m], nch = (w + 3) / 4;
    const int need = nch * strands * 256;
    if (groups.empty() || groups.back().n_ints + need > SCAN_TABLES * 256) {
      GroupRec g;
      g.m0 = g.m1 = (int32_t)recs.size();
      g.table0 = (int32_t)tables.size();
      g.n_ints = 0;
      groups.push_back(g);
    }
    GroupRec& g = groups.back();
    MotifRec r;
    r.off = g.n_ints;
    r.w = w;
    r.nch = nch;
    r.m = m;
    recs.push_back(r);
    g.m1 = (int32_t)recs.size();
    g.n_ints += need;
    const int32_t* S = h_S + (size_t)m * PENGK_MAX_MOTIF_LEN * 4;
    for (int st = 0; st < strands; ++st)
      for (int c = 0; c < nch; ++c)
        for (int idx = 0; idx < 256; ++idx) {
          int32_t v = 0;
          for (int k = 0; k < 4 && 4 * c + k < w; ++k) {
            const int j = 4 * c + k, a = (idx >> (2 * k)) & 3;
            v += st == 0 ? S[j * 4 + a] : S[(w - 1 - j) * 4 + (3 - a)];  // reverse complement: S_rc[j][a] = S[w-1-j][3-a]
          }
          tables.push_back(v);
        }
  }
  const size_t tb = tables.size() * sizeof(int32_t), rb = recs.size() * sizeof(MotifRec), gb = groups.size() * sizeof(GroupRec);
  int rc = ensure_scratch(ctx, &ctx->d_score, &ctx->score_bytes, tb + rb + gb);
  if (rc) return rc;
  char* base = (char*)ctx->d_score;
  std::vector<char> staged(tb + rb + gb);
  memcpy(staged.data(), tables.data(), tb);
  memcpy(staged.data() + tb, recs.data(), rb);
  memcpy(staged.data() + tb + rb, groups.data(), gb);
  // (synchronous: the staging vector dies with this call, and the scratch may still be read by an earlier scan)
  PENGK_HIP(hipStreamSynchronize(ctx->stream));
  PENGK_HIP(hipMemcpy(base, staged.data(), staged.size(), hipMemcpyHostToDevice));
  const dim3 grid(grid_for(ctx, n_seq, SCAN_THREADS, 8), (unsigned)groups.size());
  const int32_t* dt = (const int32_t*)base;
  const MotifRec* dr = (const MotifRec*)(base + tb);
  const GroupRec* dg = (const GroupRec*)(base + tb + rb);
  if (both_strands)
    hipLaunchKernelGGL(motif_scan_kernel<true>, grid, dim3(SCAN_THREADS), 0, ctx->stream, d_words, d_valid, d_offs, d_lens, n_seq,
                       dt, dr, dg, d_best);
  else
    hipLaunchKernelGGL(motif_scan_kernel<false>, grid, dim3(SCAN_THREADS), 0, ctx->stream, d_words, d_valid, d_offs, d_lens, n_seq,
                       dt, dr, dg, d_best);
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

int pengk_score_summary(const uint64_t* h_pos, const uint64_t* h_neg, uint64_t nbins, double* zoops_out, double* occur_out) {
  if (!h_pos || !h_neg || !zoops_out || !occur_out || nbins == 0) return fail(PENGK_ERR_ARG, "pengk_score_summary: bad argument");
  const uint64_t LIMIT = 1ull << 62;
  uint64_t npos = 0, nneg = 0;
  for (uint64_t s = 0; s < nbins; ++s) {
    npos += h_pos[s];
    nneg += h_neg[s];
    if (npos > LIMIT || nneg > LIMIT) return fail(PENGK_ERR_RANGE, "pengk_score_summary: counts above 2^62");
  }
  if (npos == 0 || nneg == 0) {  // nothing to separate
    *zoops_out = 0.5;
    *occur_out = 0.0;
    return PENGK_OK;
  }
  // AUC numerator: sum_s P[s] * (2 * Nneg_below(s) + N[s]), every product and sum checked against 2^62
  unsigned __int128 num = 0;
  uint64_t below = 0;
  for (uint64_t s = 0; s < nbins; ++s) {
    num += (unsigned __int128)h_pos[s] * (2 * (unsigned __int128)below + h_neg[s]);
    if (num > (unsigned __int128)LIMIT) return fail(PENGK_ERR_RANGE, "pengk_score_summary: AUC numerator above 2^62");
    below += h_neg[s];
  }
  *zoops_out = (double)(uint64_t)num / (2.0 * (double)npos * (double)nneg);
  // occur: the smallest threshold t with 100 * Nneg_ge(t) <= Nneg (t = nbins: above every score)
  uint64_t neg_ge = nneg, pos_ge = npos, t = 0;
  for (; t < nbins; ++t) {
    if ((unsigned __int128)100 * neg_ge <= nneg) break;
    neg_ge -= h_neg[t];
    pos_ge -= h_pos[t];
  }
  const double fpr = (double)neg_ge / (double)nneg, tpr = (double)pos_ge / (double)npos;
  double occ = fpr == 1.0 ? 0.0 : (tpr - fpr) / (1.0 - fpr);
  *occur_out = occ < 0.0 ? 0.0 : occ > 1.0 ? 1.0 : occ;
  return PENGK_OK;
}

}  // extern "C"
