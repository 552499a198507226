// score.hip -- motif scoring against sampled background sequences (the step scripts/shoot_peng.py adds after peng_motif:
// every found motif scored by how well it separates the input sequences from random ones).  DESIGN.md 10.
//
//   scan layout    host builder: byte codes -> 2-bit words + validity words, every sequence from a 32-base boundary
//   sampler        one thread per sequence, order-K Markov chain, counter-based draws: shards reproduce one process
//   shuffle         one thread per sequence, its 25 doublet counters in LDS: a negative with the
//                  sequence's own dinucleotide counts (shuffle_core.h)
//   scan           motif groups whose 4-mer chunk tables fit in LDS; one thread per sequence slides a 64-base look-ahead
//                  buffer over its words, so chunk c of the window is byte c of the buffer
//   histograms     per-motif integer histograms of the best scores (LDS bins for the top of the range, global beyond)
//   sites          (--sites) the scan's walk again with per-motif thresholds: a count pass, block totals
//                  that cut the sequences into slices of bounded records, an exclusive scan of a slice's counts and an
//                  emit pass that writes every site at its place
//   first order    (--dinuc) the adjacent-pair counts of the best sites, the interpolated model on the
//                  host, and the scan again with a 16-entry boundary table behind every chunk table
//   enrichment     (--enrich) the scan with a sequence's best score kept in a register and binned where it
//                  stands, for a whole motif database: nothing of size motifs x sequences; Fisher's exact tail on the host
#include <string.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "pengk_internal.h"
#include "scan_walk.h"
#include "shuffle_core.h"

namespace pengk {
using namespace scan;  // the shared walk and its records (scan_walk.h)
namespace {

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

// pengk_motif_scan: the best window score of every motif on every sequence
template <bool BOTH>
struct BestVisit {
  const MotifRec* mrec;
  int32_t* best_out;
  uint64_t n_seq, i;
  int best[SCAN_PASS];
  __device__ __forceinline__ void begin(int q, int) { best[q] = PENGK_SCORE_SENTINEL; }
  __device__ __forceinline__ void window(int q, uint32_t, int32_t sf, int32_t sr) { best[q] = max(best[q], BOTH ? max(sf, sr) : sf); }
  __device__ __forceinline__ void end(int q, int r) { best_out[(uint64_t)mrec[r].m * n_seq + i] = best[q]; }
};

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

// ---- motif sites (pengk_sites_*): every window strand at or above a motif's threshold, in a fixed order --------------
constexpr int SITES_THREADS = 256;
constexpr uint32_t SITES_BLOCK = PENGK_SITES_BLOCK;  // sequences per block total of pengk_sites_slices
constexpr int XS_PER = 8;                            // offsets scan: elements per thread ...
constexpr int XS_TILE = SITES_THREADS * XS_PER;      // ... and per workgroup

// sites of every motif on every sequence: counts[m * n_seq + i] (uint64: 2 per window of a 2^32-base sequence)
template <bool BOTH>
struct CountVisit {
  const MotifRec* mrec;
  const int32_t* thr;  // by group record
  unsigned long long* counts;
  uint64_t n_seq, i;
  int32_t t[SCAN_PASS];
  unsigned long long c[SCAN_PASS];
  __device__ __forceinline__ void begin(int q, int r) {
    t[q] = thr[r];
    c[q] = 0;
  }
  __device__ __forceinline__ void window(int q, uint32_t, int32_t sf, int32_t sr) {
    c[q] += (unsigned)(sf >= t[q]) + (unsigned)(BOTH && sr >= t[q]);
  }
  __device__ __forceinline__ void end(int q, int r) { counts[(uint64_t)mrec[r].m * n_seq + i] = c[q]; }
};

// the records of sequences [i0, i1): sequence i's sites of motif m from d_so[m * (i1 - i0) + i - i0] on, in window order,
// + before -; a record at or beyond cap is not written (the caller sized cap from the counts: none is)
template <bool BOTH>
struct EmitVisit {
  const MotifRec* mrec;
  const int32_t* thr;
  const unsigned long long* so;
  pengk_site* out;
  uint64_t cap, ns, i, il;
  int32_t t[SCAN_PASS];
  uint64_t o[SCAN_PASS];
  uint32_t ms[SCAN_PASS];
  __device__ __forceinline__ void begin(int q, int r) {
    t[q] = thr[r];
    o[q] = so[(uint64_t)mrec[r].m * ns + il];
    ms[q] = (uint32_t)mrec[r].m << 1;
  }
  __device__ __forceinline__ void put(int q, uint32_t pos, int32_t sc, uint32_t strand) {
    if (o[q] < cap) {
      pengk_site rec;
      rec.seq = (uint32_t)il;
      rec.pos = pos;
      rec.score = sc;
      rec.motif_strand = ms[q] | strand;
      out[o[q]] = rec;
    }
    ++o[q];
  }
  __device__ __forceinline__ void window(int q, uint32_t pos, int32_t sf, int32_t sr) {
    if (sf >= t[q]) put(q, pos, sf, 0u);
    if (BOTH && sr >= t[q]) put(q, pos, sr, 1u);
  }
  __device__ __forceinline__ void end(int, int) {}
};

// one kernel for both passes: the shared walk, the visitor's state per sequence
template <bool BOTH, bool EMIT>
__global__ __launch_bounds__(SCAN_THREADS) void motif_sites_kernel(const uint64_t* __restrict__ words,
                                                                   const uint32_t* __restrict__ valid,
                                                                   const int64_t* __restrict__ offs,
                                                                   const uint32_t* __restrict__ lens, uint64_t i0, uint64_t i1,
                                                                   uint64_t n_seq, const int32_t* __restrict__ tables,
                                                                   const MotifRec* __restrict__ recs,
                                                                   const GroupRec* __restrict__ groups,
                                                                   const int32_t* __restrict__ thr,
                                                                   unsigned long long* __restrict__ counts,
                                                                   const unsigned long long* __restrict__ so,
                                                                   pengk_site* __restrict__ out, uint64_t cap) {
  __shared__ int32_t tab[SCAN_TABLES * 256];
  __shared__ MotifRec mrec[SCAN_MAX_MOTIFS];
  __shared__ int32_t mthr[SCAN_MAX_MOTIFS];
  const GroupRec g = groups[blockIdx.y];
  for (int t = threadIdx.x; t < g.n_ints; t += SCAN_THREADS) tab[t] = tables[g.table0 + t];
  for (int t = threadIdx.x; t < g.m1 - g.m0; t += SCAN_THREADS) {
    mrec[t] = recs[g.m0 + t];
    mthr[t] = thr[recs[g.m0 + t].m];
  }
  __syncthreads();
  for (uint64_t i = i0 + blockIdx.x * (uint64_t)SCAN_THREADS + threadIdx.x; i < i1; i += (uint64_t)gridDim.x * SCAN_THREADS) {
    const uint32_t L = lens[i];
    const uint64_t w0 = (uint64_t)offs[i] >> 5;
    if (EMIT) {
      EmitVisit<BOTH> v{mrec, mthr, so, out, cap, i1 - i0, i, i - i0, {}, {}, {}};
      walk_sequence<BOTH>(words + w0, valid ? valid + w0 : nullptr, L, tab, mrec, g.m1 - g.m0, v);
    } else {
      CountVisit<BOTH> v{mrec, mthr, counts, n_seq, i, {}, {}};
      walk_sequence<BOTH>(words + w0, valid ? valid + w0 : nullptr, L, tab, mrec, g.m1 - g.m0, v);
    }
  }
}

// inclusive sum over the workgroup (sh: SITES_THREADS entries; every thread calls it)
__device__ __forceinline__ unsigned long long block_inclusive_sum(unsigned long long v, unsigned long long* sh,
                                                                  unsigned long long* total = nullptr) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int d = 1; d < SITES_THREADS; d <<= 1) {
    const unsigned long long x = t >= d ? sh[t - d] : 0ull;
    __syncthreads();
    sh[t] += x;
    __syncthreads();
  }
  const unsigned long long r = sh[t];
  if (total) *total = sh[SITES_THREADS - 1];
  __syncthreads();
  return r;
}

// per-sequence totals over the motifs, per-block totals (SITES_BLOCK sequences) and per-motif totals (added to mtot)
__global__ __launch_bounds__(SITES_THREADS) void site_totals_kernel(const unsigned long long* __restrict__ counts, uint64_t n_seq,
                                                                   int n_motifs, unsigned long long* __restrict__ seq_tot,
                                                                   unsigned long long* __restrict__ block_tot,
                                                                   unsigned long long* __restrict__ mtot) {
  __shared__ unsigned long long sh[SITES_THREADS];
  constexpr int PER = SITES_BLOCK / SITES_THREADS;
  const uint64_t base = (uint64_t)blockIdx.x * SITES_BLOCK;
  unsigned long long st[PER];
#pragma unroll
  for (int r = 0; r < PER; ++r) st[r] = 0;
  for (int m = 0; m < n_motifs; ++m) {
    unsigned long long ms = 0;
#pragma unroll
    for (int r = 0; r < PER; ++r) {
      const uint64_t i = base + (uint64_t)r * SITES_THREADS + threadIdx.x;
      if (i < n_seq) {
        const unsigned long long c = counts[(uint64_t)m * n_seq + i];
        st[r] += c;
        ms += c;
      }
    }
    ms = block_inclusive_sum(ms, sh);
    if (threadIdx.x == SITES_THREADS - 1 && ms) atomicAdd(&mtot[m], ms);
  }
  unsigned long long bs = 0;
#pragma unroll
  for (int r = 0; r < PER; ++r) {
    const uint64_t i = base + (uint64_t)r * SITES_THREADS + threadIdx.x;
    if (i < n_seq) seq_tot[i] = st[r];
    bs += st[r];
  }
  bs = block_inclusive_sum(bs, sh);
  if (threadIdx.x == SITES_THREADS - 1) block_tot[blockIdx.x] = bs;
}

// exclusive scan of the counts of sequences [i0, i0 + ns), motif-major: element k = counts[(k / ns) * n_seq + i0 + k % ns]
__device__ __forceinline__ unsigned long long xs_elem(const unsigned long long* counts, uint64_t n_seq, uint64_t i0, uint64_t ns,
                                                      uint64_t k) {
  return counts[(k / ns) * n_seq + i0 + k % ns];
}

__global__ __launch_bounds__(SITES_THREADS) void xscan_tiles_kernel(const unsigned long long* __restrict__ counts, uint64_t n_seq,
                                                                    uint64_t i0, uint64_t ns, uint64_t n,
                                                                    unsigned long long* __restrict__ part) {
  __shared__ unsigned long long sh[SITES_THREADS];
  const uint64_t k0 = (uint64_t)blockIdx.x * XS_TILE + (uint64_t)threadIdx.x * XS_PER;
  unsigned long long s = 0;
  for (int r = 0; r < XS_PER; ++r)
    if (k0 + r < n) s += xs_elem(counts, n_seq, i0, ns, k0 + r);
  s = block_inclusive_sum(s, sh);
  if (threadIdx.x == SITES_THREADS - 1) part[blockIdx.x] = s;
}

// (one workgroup) the tiles' sums -> their exclusive prefix sums, in place
__global__ __launch_bounds__(SITES_THREADS) void xscan_parts_kernel(unsigned long long* __restrict__ part, uint64_t n_tiles) {
  __shared__ unsigned long long sh[SITES_THREADS];
  unsigned long long carry = 0;
  for (uint64_t b = 0; b < n_tiles; b += XS_TILE) {
    unsigned long long v[XS_PER], s = 0;
    const uint64_t k0 = b + (uint64_t)threadIdx.x * XS_PER;
    for (int r = 0; r < XS_PER; ++r) {
      v[r] = k0 + r < n_tiles ? part[k0 + r] : 0ull;
      s += v[r];
    }
    unsigned long long tot = 0;
    unsigned long long e = carry + block_inclusive_sum(s, sh, &tot) - s;
    for (int r = 0; r < XS_PER; ++r) {
      if (k0 + r < n_tiles) part[k0 + r] = e;
      e += v[r];
    }
    carry += tot;
  }
}

__global__ __launch_bounds__(SITES_THREADS) void xscan_apply_kernel(const unsigned long long* __restrict__ counts, uint64_t n_seq,
                                                                    uint64_t i0, uint64_t ns, uint64_t n,
                                                                    const unsigned long long* __restrict__ part,
                                                                    unsigned long long* __restrict__ out) {
  __shared__ unsigned long long sh[SITES_THREADS];
  const uint64_t k0 = (uint64_t)blockIdx.x * XS_TILE + (uint64_t)threadIdx.x * XS_PER;
  unsigned long long v[XS_PER], s = 0;
  for (int r = 0; r < XS_PER; ++r) {
    v[r] = k0 + r < n ? xs_elem(counts, n_seq, i0, ns, k0 + r) : 0ull;
    s += v[r];
  }
  unsigned long long e = part[blockIdx.x] + block_inclusive_sum(s, sh) - s;
  for (int r = 0; r < XS_PER; ++r) {
    if (k0 + r < n) out[k0 + r] = e;
    e += v[r];
  }
}

// ---- central enrichment (pengk_motif_best_sites, pengk_centrality_histograms) --------------------------
constexpr uint64_t GOLDEN = 0x9E3779B97F4A7C15ull;
constexpr int CENT_LDS_BINS = 16384;  // offset and length bins of one motif in LDS (64 KiB) when they all fit, else global

// the best window strand of every motif on every sequence: the largest (score, key), key = mix64(h ^ (2p + s)),
// h = mix64(GOLDEN * (g + 1) ^ m); an equal key keeps the earlier window strand, which the scan order (p, then + before
// -) makes the smaller (p, s).  Keys are computed on ties only: the best's own key once, then the challenger's.
template <bool BOTH>
struct BestSiteVisit {
  const MotifRec* mrec;
  int32_t* best_out;
  unsigned long long* site_out;
  uint64_t n_seq, i, g;
  int32_t b[SCAN_PASS];
  uint64_t c[SCAN_PASS];   // 2p + s of the best
  uint64_t h[SCAN_PASS];
  uint64_t kb[SCAN_PASS];  // its key, once kv
  bool kv[SCAN_PASS];
  __device__ __forceinline__ void begin(int q, int r) {
    b[q] = PENGK_SCORE_SENTINEL;
    c[q] = 0;
    kv[q] = false;
    h[q] = mix64((GOLDEN * (g + 1)) ^ (uint64_t)mrec[r].m);
  }
  __device__ __forceinline__ void offer(int q, uint64_t cand, int32_t sc) {
    if (sc > b[q]) {
      b[q] = sc;
      c[q] = cand;
      kv[q] = false;
      return;
    }
    if (!kv[q]) {
      kb[q] = mix64(h[q] ^ c[q]);
      kv[q] = true;
    }
    const uint64_t k = mix64(h[q] ^ cand);
    if (k > kb[q]) {
      c[q] = cand;
      kb[q] = k;
    }
  }
  __device__ __forceinline__ void window(int q, uint32_t pos, int32_t sf, int32_t sr) {
    if (sf >= b[q]) offer(q, 2ull * pos, sf);
    if (BOTH && sr >= b[q]) offer(q, 2ull * pos + 1ull, sr);
  }
  __device__ __forceinline__ void end(int q, int r) {
    const uint64_t o = (uint64_t)mrec[r].m * n_seq + i;
    best_out[o] = b[q];
    site_out[o] = c[q];
  }
};

// a kernel of its own: the visitor's state (key, site) stays out of the scoring and sites kernels
template <bool BOTH>
__global__ __launch_bounds__(SCAN_THREADS) void motif_best_site_kernel(const uint64_t* __restrict__ words,
                                                                       const uint32_t* __restrict__ valid,
                                                                       const int64_t* __restrict__ offs,
                                                                       const uint32_t* __restrict__ lens, uint64_t n_seq,
                                                                       uint64_t seq0, const int32_t* __restrict__ tables,
                                                                       const MotifRec* __restrict__ recs,
                                                                       const GroupRec* __restrict__ groups,
                                                                       int32_t* __restrict__ best_out,
                                                                       unsigned long long* __restrict__ site_out) {
  __shared__ int32_t tab[SCAN_TABLES * 256];
  __shared__ MotifRec mrec[SCAN_MAX_MOTIFS];
  const GroupRec g = groups[blockIdx.y];
  for (int t = threadIdx.x; t < g.n_ints; t += SCAN_THREADS) tab[t] = tables[g.table0 + t];
  for (int t = threadIdx.x; t < g.m1 - g.m0; t += SCAN_THREADS) mrec[t] = recs[g.m0 + t];
  __syncthreads();
  for (uint64_t i = blockIdx.x * (uint64_t)SCAN_THREADS + threadIdx.x; i < n_seq; i += (uint64_t)gridDim.x * SCAN_THREADS) {
    const uint32_t L = lens[i];
    const uint64_t w0 = (uint64_t)offs[i] >> 5;
    BestSiteVisit<BOTH> v{mrec, best_out, site_out, n_seq, i, seq0 + i, {}, {}, {}, {}, {}};
    walk_sequence<BOTH>(words + w0, valid ? valid + w0 : nullptr, L, tab, mrec, g.m1 - g.m0, v);
  }
}

// per motif (blockIdx.y): the best sites at or above its threshold of the sequences with w <= L <= max_len, ADDED to
// the offset bins hd[m * (2 max_len + 1) + max_len + d], d = 2p + w - L, and the length bins hl[m * (max_len + 1) + L].
// LDS: every bin of the motif in LDS (equal lengths send all counts to a few bins), flushed once per block.
template <bool LDS>
__global__ __launch_bounds__(HIST_THREADS) void centrality_hist_kernel(const int32_t* __restrict__ best,
                                                                       const unsigned long long* __restrict__ site,
                                                                       const uint32_t* __restrict__ lens, uint64_t n_seq,
                                                                       const int32_t* __restrict__ wt, uint32_t max_len,
                                                                       unsigned long long* __restrict__ hd,
                                                                       unsigned long long* __restrict__ hl) {
  __shared__ uint32_t h[LDS ? CENT_LDS_BINS : 1];
  const int m = blockIdx.y;
  const uint32_t w = (uint32_t)wt[2 * m];
  const int32_t t = wt[2 * m + 1];
  const uint32_t nd = 2 * max_len + 1, nl = max_len + 1;
  unsigned long long* HD = hd + (uint64_t)m * nd;
  unsigned long long* HL = hl + (uint64_t)m * nl;
  if (LDS) {
    for (uint32_t k = threadIdx.x; k < nd + nl; k += HIST_THREADS) h[k] = 0;
    __syncthreads();
  }
  const int32_t* B = best + (uint64_t)m * n_seq;
  const unsigned long long* C = site + (uint64_t)m * n_seq;
  for (uint64_t i = blockIdx.x * (uint64_t)HIST_THREADS + threadIdx.x; i < n_seq; i += (uint64_t)gridDim.x * HIST_THREADS) {
    const uint32_t L = lens[i];
    if (B[i] < t || L > max_len || L < w) continue;
    const uint64_t p = C[i] >> 1;
    if (p > L - w) continue;  // (not a window of this sequence: no bin)
    const uint32_t bd = 2 * (uint32_t)p + w + max_len - L;  // max_len + d, in [max_len - (L - w), max_len + (L - w)]
    if (LDS) {
      atomicAdd(&h[bd], 1u);
      atomicAdd(&h[nd + L], 1u);
    } else {
      atomicAdd(&HD[bd], 1ull);
      atomicAdd(&HL[L], 1ull);
    }
  }
  if (LDS) {
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < nd + nl; k += HIST_THREADS)
      if (h[k]) atomicAdd(k < nd ? &HD[k] : &HL[k - nd], (unsigned long long)h[k]);
  }
}

// ---- motif pair spacing (pengk_spacing_histograms) ---------------------------------------------------
constexpr int SPACE_THREADS = 1024;
constexpr int SPACE_LDS_BINS = 16000;  // the bins of one row's pairs in LDS (62.5 KiB, two workgroups per CU)

// a grid row: motif b against the motifs [a0, a1) before it; the row with a0 = 0 also counts b's own sites
struct SpaceRow {
  int32_t b, a0, a1, pad;
};

// One more in bin `bin` of h for every lane with `on`; every lane of the wave calls.  The lanes that share the first
// counting lane's bin add once, together: a composite element sends nearly every lane to one gap bin and equal-length
// input sends every lane to one length bin, where 64 adds to one LDS address would queue.  The others add on their own.
__device__ __forceinline__ void wave_count(uint32_t* h, bool on, uint32_t bin) {
  const unsigned long long act = __ballot(on);
  if (!act) return;
  const int lead = __ffsll(act) - 1;
  const uint32_t first = (uint32_t)__shfl((int)bin, lead);
  const unsigned long long same = __ballot(on && bin == first);
  if (!on) return;
  if (bin != first) atomicAdd(&h[bin], 1u);
  else if ((int)(threadIdx.x & 63u) == lead) atomicAdd(&h[first], (uint32_t)__popcll(same));
}

// per row (blockIdx.y): motif b's site read once per sequence and, only where b has one, the motifs a of the row: best[a]
// first, site[a] on a hit.  wt: (width, threshold) per motif.  Considered: min_len <= L <= max_len.  Pair q = b (b - 1) / 2
// + a owns nb = 4 (G + 1) + 2 gap bins in hg and max_len + 1 length bins in hl (include/pengk.h, "motif pair spacing").
// LDS: the row's (a1 - a0) (nb + max_len + 1) bins in LDS as uint32, flushed once per block, one add per non-zero bin.
template <bool LDS>
__global__ __launch_bounds__(SPACE_THREADS) void spacing_hist_kernel(const int32_t* __restrict__ best,
                                                                     const unsigned long long* __restrict__ site,
                                                                     const uint32_t* __restrict__ lens, uint64_t n_seq,
                                                                     const int32_t* __restrict__ wt,
                                                                     const SpaceRow* __restrict__ rows, uint32_t G,
                                                                     uint32_t min_len, uint32_t max_len,
                                                                     unsigned long long* __restrict__ hg,
                                                                     unsigned long long* __restrict__ hl,
                                                                     unsigned long long* __restrict__ hm) {
  __shared__ uint32_t h[LDS ? SPACE_LDS_BINS : 1];
  __shared__ int32_t sw[PENGK_SPACING_MAX_MOTIFS], st[PENGK_SPACING_MAX_MOTIFS];
  __shared__ unsigned long long s_sites;
  const SpaceRow row = rows[blockIdx.y];
  const uint32_t nb = 4 * (G + 1) + 2, nl = max_len + 1, per = nb + nl;
  const uint32_t n_lds = (uint32_t)(row.a1 - row.a0) * per;  // (LDS only: the host made it fit)
  if (threadIdx.x < (unsigned)row.a1 || (int)threadIdx.x == row.b) {
    sw[threadIdx.x] = wt[2 * threadIdx.x];
    st[threadIdx.x] = wt[2 * threadIdx.x + 1];
  }
  if (threadIdx.x == 0) s_sites = 0;
  if (LDS)
    for (uint32_t k = threadIdx.x; k < n_lds; k += SPACE_THREADS) h[k] = 0;
  __syncthreads();
  const uint32_t wb = (uint32_t)sw[row.b];
  const int32_t tb = st[row.b];
  const int32_t* Bb = best + (uint64_t)row.b * n_seq;
  const unsigned long long* Cb = site + (uint64_t)row.b * n_seq;
  const uint64_t q0 = (uint64_t)row.b * (uint64_t)(row.b - 1) / 2;  // (b = 0: no pair, never used)
  uint32_t mine = 0;  // b's sites seen by this thread (a block walks fewer than 2^32 sequences: the host sees to it)
  // (the loop's trip count is the same for every lane of a wave: wave_count needs them all)
  for (uint64_t i0 = blockIdx.x * (uint64_t)SPACE_THREADS; i0 < n_seq; i0 += (uint64_t)gridDim.x * SPACE_THREADS) {
    const uint64_t i = i0 + threadIdx.x;
    bool has = false;
    uint32_t L = 0, pb = 0, sb = 0;
    if (i < n_seq) {
      L = lens[i];
      if (L >= min_len && L <= max_len) {
        const int32_t s = Bb[i];
        if (s != PENGK_SCORE_SENTINEL && s >= tb) {
          const unsigned long long c = Cb[i];
          has = (c >> 1) <= (unsigned long long)(L - wb);
          pb = (uint32_t)(c >> 1);
          sb = (uint32_t)(c & 1u);
        }
      }
    }
    mine += has;
    if (!__any(has)) continue;
    for (int a = row.a0; a < row.a1; ++a) {
      bool apart = false, hit = false;
      uint32_t bin = 0;
      if (has) {
        const int32_t s = best[(uint64_t)a * n_seq + i];
        if (s != PENGK_SCORE_SENTINEL && s >= st[a]) {
          const unsigned long long c = site[(uint64_t)a * n_seq + i];
          const uint32_t wa = (uint32_t)sw[a], sa = (uint32_t)(c & 1u);
          if ((c >> 1) <= (unsigned long long)(L - wa)) {
            const uint32_t pa = (uint32_t)(c >> 1);
            hit = true;
            if (pb >= pa + wa || pa >= pb + wb) {
              apart = true;
              const uint32_t side = pb >= pa + wa ? 0u : 1u;
              const uint32_t g = side ? pa - pb - wb : pb - pa - wa;
              bin = g <= G ? (2 * (sa ^ sb) + (side ^ sa)) * (G + 1) + g : nb - 1;
            } else {
              bin = nb - 2;
            }
          }
        }
      }
      if (LDS) {
        uint32_t* hp = h + (uint32_t)(a - row.a0) * per;
        wave_count(hp, hit, bin);
        wave_count(hp + nb, apart, L);
      } else if (hit) {
        const uint64_t q = q0 + (uint64_t)a;
        atomicAdd(&hg[q * nb + bin], 1ull);
        if (apart) atomicAdd(&hl[q * nl + L], 1ull);
      }
    }
  }
  if (row.a0 == 0 && mine) atomicAdd(&s_sites, (unsigned long long)mine);
  __syncthreads();
  if (row.a0 == 0 && threadIdx.x == 0 && s_sites) atomicAdd(&hm[row.b], s_sites);
  if (LDS)
    for (uint32_t k = threadIdx.x; k < n_lds; k += SPACE_THREADS)
      if (h[k]) {
        const uint32_t slot = k / per, r = k - slot * per;
        const uint64_t q = q0 + (uint64_t)row.a0 + slot;
        atomicAdd(r < nb ? &hg[q * nb + r] : &hl[q * nl + (r - nb)], (unsigned long long)h[k]);
      }
}

// ---- site profiles (pengk_site_profiles) -------------------------------------------------------------
constexpr int PROF_THREADS = 256;
constexpr int PROF_BINS = PENGK_MAX_MOTIF_LEN * 5;

// per motif (blockIdx.y): the base of every column c in [-F, w + F) of the best sites at or above the motif's threshold,
// read on the site's strand, ADDED to counts[(m * PENGK_MAX_MOTIF_LEN + c + F) * 5 + b] (b = 4: outside the sequence or
// not A/C/G/T).  A wave takes 64 consecutive sequences.  For a strong motif nearly every lane of it adds to the same
// (column, base) bin, so the lanes do not add at all: per column the wave ballots the two bits of the base, "is a base"
// and "has a site", counts the five bins from the masks, and lanes 0..4 add them once to the block's LDS bins, which
// are flushed once per block.  A site with its flanks spans at most 64 bases: three words per lane, loaded once.
// A wave without a site (the usual wave of a weak motif) reads best, site and length and goes on.
__global__ __launch_bounds__(PROF_THREADS) void site_profile_kernel(const uint64_t* __restrict__ words,
                                                                    const uint32_t* __restrict__ valid,
                                                                    const int64_t* __restrict__ offs,
                                                                    const uint32_t* __restrict__ lens, uint64_t n_seq,
                                                                    const int32_t* __restrict__ best,
                                                                    const unsigned long long* __restrict__ site,
                                                                    const int32_t* __restrict__ wtf,
                                                                    unsigned long long* __restrict__ counts) {
  __shared__ uint32_t bins[PROF_BINS];
  const int m = blockIdx.y;
  const int32_t w = wtf[3 * m], t = wtf[3 * m + 1], F = wtf[3 * m + 2];
  const int32_t C = w + 2 * F;  // <= PENGK_MAX_MOTIF_LEN (the host clamps F)
  for (int k = threadIdx.x; k < PROF_BINS; k += PROF_THREADS) bins[k] = 0;
  __syncthreads();
  const int32_t* B = best + (uint64_t)m * n_seq;
  const unsigned long long* S = site + (uint64_t)m * n_seq;
  const int lane = threadIdx.x & 63;
  // (every lane of a wave makes the same trips: the ballots below see the whole wave)
  for (uint64_t i0 = blockIdx.x * (uint64_t)PROF_THREADS + (threadIdx.x & ~63); i0 < n_seq;
       i0 += (uint64_t)gridDim.x * PROF_THREADS) {
    const uint64_t i = i0 + lane;
    bool sel = false;
    int64_t L = 0, p = 0;
    int32_t strand = 0;
    if (i < n_seq) {
      const int32_t b = B[i];
      L = lens[i];
      if (b != PENGK_SCORE_SENTINEL && b >= t && L >= w) {
        const uint64_t c = S[i];
        p = (int64_t)(c >> 1);
        strand = (int32_t)(c & 1);
        sel = p <= L - w;  // (not a window of this sequence: no site)
      }
    }
    const unsigned long long has = __ballot(sel);
    if (has == 0) continue;
    // the bases [g0, g0 + C) of the sequence that lie inside it: [a, e), in the words j0 .. j0 + 2 of the sequence
    const int64_t g0 = p - F;
    int64_t a = 0, e = 0, j0 = 0;
    uint64_t W0 = 0, W1 = 0, W2 = 0;
    uint32_t V0 = 0, V1 = 0, V2 = 0;
    if (sel) {
      a = g0 > 0 ? g0 : 0;
      e = g0 + C < L ? g0 + C : L;  // a <= p < p + w <= e
      j0 = a >> 5;
      const int64_t j1 = (e - 1) >> 5;  // <= j0 + 2: e - a <= 64
      const uint64_t w0 = ((uint64_t)offs[i] >> 5) + (uint64_t)j0;
      W0 = words[w0];
      V0 = valid ? valid[w0] : 0xFFFFFFFFu;
      if (j0 + 1 <= j1) {
        W1 = words[w0 + 1];
        V1 = valid ? valid[w0 + 1] : 0xFFFFFFFFu;
      }
      if (j0 + 2 <= j1) {
        W2 = words[w0 + 2];
        V2 = valid ? valid[w0 + 2] : 0xFFFFFFFFu;
      }
    }
    for (int32_t c = 0; c < C; ++c) {
      // column c of the site: base g0 + c on +, g0 + C - 1 - c complemented on -
      const int64_t q = g0 + (strand ? C - 1 - c : c);
      bool ok = false;
      uint32_t b = 0;
      if (sel && q >= a && q < e) {
        const int64_t j = (q >> 5) - j0;
        const uint64_t W = j == 0 ? W0 : (j == 1 ? W1 : W2);
        const uint32_t V = j == 0 ? V0 : (j == 1 ? V1 : V2);
        const uint32_t r = (uint32_t)q & 31u;
        ok = (V >> r) & 1u;
        b = ((uint32_t)(W >> (2 * r)) & 3u) ^ (strand ? 3u : 0u);
      }
      const unsigned long long mo = __ballot(ok), m0 = __ballot(b & 1u), m1 = __ballot(b & 2u);
      if (lane < 5) {
        const unsigned long long mask =
            lane == 4 ? has & ~mo : mo & (lane & 1 ? m0 : ~m0) & (lane & 2 ? m1 : ~m1);
        const uint32_t n = (uint32_t)__popcll(mask);
        if (n) atomicAdd(&bins[c * 5 + lane], n);
      }
    }
  }
  __syncthreads();
  unsigned long long* out = counts + (uint64_t)m * PROF_BINS;
  for (int k = threadIdx.x; k < C * 5; k += PROF_THREADS)
    if (bins[k]) atomicAdd(&out[k], (unsigned long long)bins[k]);
}

// ---- site histograms (pengk_sites_histograms: the ranks behind --sites-qvalue) -------------------------
constexpr int QH_PRIV_BINS = 2560;          // workgroup-private 32-bit bins (10 KiB), shared evenly by the group's motifs
constexpr uint32_t QH_LONG_SEQ = 1u << 16;  // a longer sequence adds to the global bins only
constexpr int QH_FLUSH_TRIPS = 64;          // trips of the workgroup's sequence loop between two flushes of the private bins

// Per motif of the group: the global bins (bin 0 = the threshold), the lowest score with a private bin, the scored
// window strands of the workgroup.
struct HistRec {
  unsigned long long* H;
  unsigned long long tests;
  int32_t thr, top;
};

// A fourth visitor: every site adds 1 to its motif's bin score - t, every valid window counts as one or two scored
// strands, and the per-(motif, sequence) site count is CountVisit's.  The top `per` scores of each motif of the group
// (where a motif that sits in every sequence sends its sites) have a workgroup-private 32-bit bin in LDS; a lower score
// adds to the global uint64 bin directly.
// No private bin can wrap: a thread adds to it only for a sequence of at most QH_LONG_SEQ = 2^16 bases, so at most 2^17
// times per trip of the workgroup's loop (one sequence per thread and trip, two strands per window); 256 threads and
// QH_FLUSH_TRIPS = 64 trips between two flushes bound a bin by 2^8 * 2^17 * 2^6 = 2^31 < 2^32.  A longer sequence (up to
// 2^33 window strands) gets top = INT32_MAX, which no score reaches: all its sites go to the global bins.
template <bool BOTH>
struct HistVisit {
  const MotifRec* mrec;
  HistRec* hrec;
  uint32_t* priv;
  unsigned long long* counts;  // NULL: not stored
  uint64_t n_seq, i;
  int per;
  bool short_seq;
  int32_t t[SCAN_PASS], top[SCAN_PASS], pb[SCAN_PASS], r[SCAN_PASS];
  uint32_t nw[SCAN_PASS];
  unsigned long long c[SCAN_PASS];
  __device__ __forceinline__ void begin(int q, int rr) {
    r[q] = rr;
    t[q] = hrec[rr].thr;
    top[q] = short_seq ? hrec[rr].top : INT32_MAX;
    pb[q] = rr * per - hrec[rr].top;  // private bin of score s: priv[pb + s], in [rr * per, (rr + 1) * per) for top <= s <= hi
    nw[q] = 0;
    c[q] = 0;
  }
  __device__ __forceinline__ void bump(int q, int32_t sc) {
    if (sc >= top[q]) atomicAdd(&priv[pb[q] + sc], 1u);
    else atomicAdd(&hrec[r[q]].H[(int64_t)sc - t[q]], 1ull);
    ++c[q];
  }
  __device__ __forceinline__ void window(int q, uint32_t, int32_t sf, int32_t sr) {
    ++nw[q];
    if (sf >= t[q]) bump(q, sf);
    if (BOTH && sr >= t[q]) bump(q, sr);
  }
  __device__ __forceinline__ void end(int q, int rr) {
    if (nw[q]) atomicAdd(&hrec[rr].tests, (unsigned long long)nw[q] * (BOTH ? 2u : 1u));
    if (counts) counts[(uint64_t)mrec[rr].m * n_seq + i] = c[q];
  }
};

// a kernel of its own: the count pass of --sites keeps its code when q-values are not asked for
template <bool BOTH>
__global__ __launch_bounds__(SCAN_THREADS) void motif_sites_hist_kernel(const uint64_t* __restrict__ words,
                                                                        const uint32_t* __restrict__ valid,
                                                                        const int64_t* __restrict__ offs,
                                                                        const uint32_t* __restrict__ lens, uint64_t n_seq,
                                                                        const int32_t* __restrict__ tables,
                                                                        const MotifRec* __restrict__ recs,
                                                                        const GroupRec* __restrict__ groups,
                                                                        const int32_t* __restrict__ thr,
                                                                        const int32_t* __restrict__ hi,
                                                                        const uint64_t* __restrict__ hoffs,
                                                                        unsigned long long* __restrict__ hist,
                                                                        unsigned long long* __restrict__ tests,
                                                                        unsigned long long* __restrict__ counts) {
  __shared__ int32_t tab[SCAN_TABLES * 256];
  __shared__ MotifRec mrec[SCAN_MAX_MOTIFS];
  __shared__ HistRec hrec[SCAN_MAX_MOTIFS];
  __shared__ uint32_t priv[QH_PRIV_BINS];
  const GroupRec g = groups[blockIdx.y];
  const int nrec = g.m1 - g.m0;
  const int per = QH_PRIV_BINS / nrec;  // (1 <= nrec <= SCAN_MAX_MOTIFS: at least 64 bins each)
  for (int t = threadIdx.x; t < g.n_ints; t += SCAN_THREADS) tab[t] = tables[g.table0 + t];
  for (int t = threadIdx.x; t < nrec; t += SCAN_THREADS) {
    const MotifRec mr = recs[g.m0 + t];
    mrec[t] = mr;
    // the private bins: scores (hi - per, hi], none below the threshold (hi >= every score: the host checked it)
    const int64_t tp = (int64_t)hi[mr.m] - per + 1;
    HistRec h;
    h.H = hist + hoffs[mr.m];
    h.tests = 0;
    h.thr = thr[mr.m];
    h.top = tp > (int64_t)h.thr ? (int32_t)tp : h.thr;
    hrec[t] = h;
  }
  for (int t = threadIdx.x; t < QH_PRIV_BINS; t += SCAN_THREADS) priv[t] = 0;
  __syncthreads();
  // private bin k of record k / per holds score top + k % per: bin top - thr + k % per of the motif (a bin above hi - thr
  // is never added to and stays 0)
  auto flush = [&]() {
    for (int k = threadIdx.x; k < nrec * per; k += SCAN_THREADS) {
      const uint32_t n = priv[k];
      if (n) {
        const int rr = k / per;
        atomicAdd(&hrec[rr].H[(int64_t)hrec[rr].top - hrec[rr].thr + (k - rr * per)], (unsigned long long)n);
        priv[k] = 0;
      }
    }
  };
  // (every thread of the workgroup makes the same trips: the flush inside the loop is reached by all of them)
  int trips = 0;
  for (uint64_t ib = blockIdx.x * (uint64_t)SCAN_THREADS; ib < n_seq; ib += (uint64_t)gridDim.x * SCAN_THREADS) {
    const uint64_t i = ib + threadIdx.x;
    if (i < n_seq) {
      const uint32_t L = lens[i];
      const uint64_t w0 = (uint64_t)offs[i] >> 5;
      HistVisit<BOTH> v{mrec, hrec, priv, counts, n_seq, i, per, L <= QH_LONG_SEQ, {}, {}, {}, {}, {}, {}};
      walk_sequence<BOTH>(words + w0, valid ? valid + w0 : nullptr, L, tab, mrec, nrec, v);
    }
    if (++trips == QH_FLUSH_TRIPS) {
      __syncthreads();
      flush();
      __syncthreads();
      trips = 0;
    }
  }
  __syncthreads();
  flush();
  // the scored window strands: one global atomic per motif and workgroup
  for (int t = threadIdx.x; t < nrec; t += SCAN_THREADS)
    if (hrec[t].tests) atomicAdd(&tests[mrec[t].m], hrec[t].tests);
}

// ---- database enrichment (pengk_motif_enrich: the histograms behind --enrich) ----------------------------
// Per motif of the group: the global bins (bin 0 = the threshold) and the lowest score with a private bin.
struct EnrichRec {
  unsigned long long* H;
  int32_t thr, top;
};

// A fifth visitor: BestVisit's register maximum, binned where it stands instead of stored.  The window loop is
// BestVisit's (a score is above PENGK_SCORE_SENTINEL, so the maximum itself says whether there was a window); per
// (motif, sequence) the end adds the sequence to the motif's scored counter -- one 32-bit LDS add per wave: the lanes
// that are here together are counted by a ballot, and a lane that is not counts itself the same way -- and, at or above
// the threshold, 1 to the bin of the best score: a private 32-bit LDS bin for the top `per` scores (HistVisit's
// arrangement), the global uint64 bin below them.
// No private bin or counter can wrap and none is flushed inside the loop: a sequence adds at most once per motif and
// the host refuses n_seq >= 2^32.
template <bool BOTH>
struct EnrichVisit {
  const EnrichRec* erec;
  uint32_t* priv;
  uint32_t* scored;
  int per;
  int best[SCAN_PASS];
  __device__ __forceinline__ void begin(int q, int) { best[q] = PENGK_SCORE_SENTINEL; }
  __device__ __forceinline__ void window(int q, uint32_t, int32_t sf, int32_t sr) { best[q] = max(best[q], BOTH ? max(sf, sr) : sf); }
  __device__ __forceinline__ void end(int q, int rr) {
    const int32_t b = best[q];
    const bool had = b != PENGK_SCORE_SENTINEL;
    const unsigned long long here = __ballot(1), hm = __ballot(had);
    if (hm && (int)__lane_id() == __ffsll((long long)here) - 1) atomicAdd(&scored[rr], (uint32_t)__popcll(hm));
    if (!had) return;
    const EnrichRec e = erec[rr];
    if (b < e.thr) return;
    if (b >= e.top) atomicAdd(&priv[rr * per + (b - e.top)], 1u);
    else atomicAdd(&e.H[(int64_t)b - e.thr], 1ull);
  }
};

template <bool BOTH>
__global__ __launch_bounds__(SCAN_THREADS) void motif_enrich_kernel(const uint64_t* __restrict__ words,
                                                                    const uint32_t* __restrict__ valid,
                                                                    const int64_t* __restrict__ offs,
                                                                    const uint32_t* __restrict__ lens, uint64_t n_seq,
                                                                    const int32_t* __restrict__ tables,
                                                                    const MotifRec* __restrict__ recs,
                                                                    const GroupRec* __restrict__ groups,
                                                                    const int32_t* __restrict__ thr,
                                                                    const int32_t* __restrict__ hi,
                                                                    const uint64_t* __restrict__ hoffs,
                                                                    unsigned long long* __restrict__ hist,
                                                                    unsigned long long* __restrict__ scored_out) {
  __shared__ int32_t tab[SCAN_TABLES * 256];
  __shared__ MotifRec mrec[SCAN_MAX_MOTIFS];
  __shared__ EnrichRec erec[SCAN_MAX_MOTIFS];
  __shared__ uint32_t scored[SCAN_MAX_MOTIFS];
  __shared__ uint32_t priv[QH_PRIV_BINS];
  const GroupRec g = groups[blockIdx.y];
  const int nrec = g.m1 - g.m0;
  const int per = QH_PRIV_BINS / nrec;  // (1 <= nrec <= SCAN_MAX_MOTIFS: at least 64 bins each)
  for (int t = threadIdx.x; t < g.n_ints; t += SCAN_THREADS) tab[t] = tables[g.table0 + t];
  for (int t = threadIdx.x; t < nrec; t += SCAN_THREADS) {
    const MotifRec mr = recs[g.m0 + t];
    mrec[t] = mr;
    // the private bins: scores (hi - per, hi], none below the threshold (hi >= every score: the host checked it)
    const int64_t tp = (int64_t)hi[mr.m] - per + 1;
    EnrichRec e;
    e.H = hist + hoffs[mr.m];
    e.thr = thr[mr.m];
    e.top = tp > (int64_t)e.thr ? (int32_t)tp : e.thr;
    erec[t] = e;
    scored[t] = 0;
  }
  for (int t = threadIdx.x; t < QH_PRIV_BINS; t += SCAN_THREADS) priv[t] = 0;
  __syncthreads();
  for (uint64_t i = blockIdx.x * (uint64_t)SCAN_THREADS + threadIdx.x; i < n_seq; i += (uint64_t)gridDim.x * SCAN_THREADS) {
    const uint32_t L = lens[i];
    const uint64_t w0 = (uint64_t)offs[i] >> 5;
    EnrichVisit<BOTH> v{erec, priv, scored, per, {}};
    walk_sequence<BOTH>(words + w0, valid ? valid + w0 : nullptr, L, tab, mrec, nrec, v);
  }
  __syncthreads();
  // private bin k of record k / per holds score top + k % per: bin top - thr + k % per of the motif (a bin above hi - thr
  // is never added to and stays 0); then the scored sequences: one global atomic per motif and workgroup
  for (int k = threadIdx.x; k < nrec * per; k += SCAN_THREADS) {
    const uint32_t n = priv[k];
    if (n) {
      const int rr = k / per;
      atomicAdd(&erec[rr].H[(int64_t)erec[rr].top - erec[rr].thr + (k - rr * per)], (unsigned long long)n);
    }
  }
  for (int t = threadIdx.x; t < nrec; t += SCAN_THREADS)
    if (scored[t]) atomicAdd(&scored_out[mrec[t].m], (unsigned long long)scored[t]);
}

// ---- first-order models (--dinuc) --------------------------------------------------------------------
constexpr int PAIR_BINS = PENGK_MAX_MOTIF_LEN * 17;

// site_profile_kernel for adjacent pairs: per motif (blockIdx.y) and column c in (-F, w + F) of its best sites, the
// letters a at c - 1 and b at c, read on the site's strand, ADDED to counts[(m * PENGK_MAX_MOTIF_LEN + c + F) * 17 + 4a + b]
// (bin 16: either position outside the sequence or not A/C/G/T; row 0 stays untouched).  The same wave per 64
// sequences and the same three words per lane; the column's (is a base, base) is kept for the next column.  Per column
// the wave ballots the two bits of a, the two bits of b, "both are bases" and "has a site"; lane l < 16 builds the mask
// of its own bin from them, lane 16 takes the rest, and each of the 17 adds its count once to the block's LDS bins.
__global__ __launch_bounds__(PROF_THREADS) void site_pair_profile_kernel(const uint64_t* __restrict__ words,
                                                                         const uint32_t* __restrict__ valid,
                                                                         const int64_t* __restrict__ offs,
                                                                         const uint32_t* __restrict__ lens, uint64_t n_seq,
                                                                         const int32_t* __restrict__ best,
                                                                         const unsigned long long* __restrict__ site,
                                                                         const int32_t* __restrict__ wtf,
                                                                         unsigned long long* __restrict__ counts) {
  __shared__ uint32_t bins[PAIR_BINS];
  const int m = blockIdx.y;
  const int32_t w = wtf[3 * m], t = wtf[3 * m + 1], F = wtf[3 * m + 2];
  const int32_t C = w + 2 * F;  // <= PENGK_MAX_MOTIF_LEN (the host clamps F)
  for (int k = threadIdx.x; k < PAIR_BINS; k += PROF_THREADS) bins[k] = 0;
  __syncthreads();
  const int32_t* B = best + (uint64_t)m * n_seq;
  const unsigned long long* S = site + (uint64_t)m * n_seq;
  const int lane = threadIdx.x & 63;
  // (every lane of a wave makes the same trips: the ballots below see the whole wave)
  for (uint64_t i0 = blockIdx.x * (uint64_t)PROF_THREADS + (threadIdx.x & ~63); i0 < n_seq;
       i0 += (uint64_t)gridDim.x * PROF_THREADS) {
    const uint64_t i = i0 + lane;
    bool sel = false;
    int64_t L = 0, p = 0;
    int32_t strand = 0;
    if (i < n_seq) {
      const int32_t b = B[i];
      L = lens[i];
      if (b != PENGK_SCORE_SENTINEL && b >= t && L >= w) {
        const uint64_t c = S[i];
        p = (int64_t)(c >> 1);
        strand = (int32_t)(c & 1);
        sel = p <= L - w;  // (not a window of this sequence: no site)
      }
    }
    const unsigned long long has = __ballot(sel);
    if (has == 0) continue;
    // the bases [g0, g0 + C) of the sequence that lie inside it: [a, e), in the words j0 .. j0 + 2 of the sequence
    const int64_t g0 = p - F;
    int64_t a = 0, e = 0, j0 = 0;
    uint64_t W0 = 0, W1 = 0, W2 = 0;
    uint32_t V0 = 0, V1 = 0, V2 = 0;
    if (sel) {
      a = g0 > 0 ? g0 : 0;
      e = g0 + C < L ? g0 + C : L;  // a <= p < p + w <= e
      j0 = a >> 5;
      const int64_t j1 = (e - 1) >> 5;  // <= j0 + 2: e - a <= 64
      const uint64_t w0 = ((uint64_t)offs[i] >> 5) + (uint64_t)j0;
      W0 = words[w0];
      V0 = valid ? valid[w0] : 0xFFFFFFFFu;
      if (j0 + 1 <= j1) {
        W1 = words[w0 + 1];
        V1 = valid ? valid[w0 + 1] : 0xFFFFFFFFu;
      }
      if (j0 + 2 <= j1) {
        W2 = words[w0 + 2];
        V2 = valid ? valid[w0 + 2] : 0xFFFFFFFFu;
      }
    }
    bool pok = false;
    uint32_t pb = 0;
    for (int32_t c = 0; c < C; ++c) {
      // column c of the site: base g0 + c on +, g0 + C - 1 - c complemented on -
      const int64_t q = g0 + (strand ? C - 1 - c : c);
      bool ok = false;
      uint32_t b = 0;
      if (sel && q >= a && q < e) {
        const int64_t j = (q >> 5) - j0;
        const uint64_t W = j == 0 ? W0 : (j == 1 ? W1 : W2);
        const uint32_t V = j == 0 ? V0 : (j == 1 ? V1 : V2);
        const uint32_t r = (uint32_t)q & 31u;
        ok = (V >> r) & 1u;
        b = ((uint32_t)(W >> (2 * r)) & 3u) ^ (strand ? 3u : 0u);
      }
      if (c > 0) {
        const unsigned long long mo = __ballot(ok && pok), a0 = __ballot(pb & 1u), a1 = __ballot(pb & 2u),
                                 b0 = __ballot(b & 1u), b1 = __ballot(b & 2u);
        if (lane < 17) {
          const unsigned long long mask = lane == 16 ? has & ~mo
                                                     : mo & (lane & 4 ? a0 : ~a0) & (lane & 8 ? a1 : ~a1) &
                                                           (lane & 1 ? b0 : ~b0) & (lane & 2 ? b1 : ~b1);
          const uint32_t n = (uint32_t)__popcll(mask);
          if (n) atomicAdd(&bins[c * 17 + lane], n);
        }
      }
      pok = ok;
      pb = b;
    }
  }
  __syncthreads();
  unsigned long long* out = counts + (uint64_t)m * PAIR_BINS;
  for (int k = 17 + threadIdx.x; k < C * 17; k += PROF_THREADS)
    if (bins[k]) atomicAdd(&out[k], (unsigned long long)bins[k]);
}

// The first-order scan.  A motif's chunk c owns DN_STRIDE ints per strand: the 256-entry 4-mer table -- S0 (chunk 0)
// plus every pair term whose two columns lie inside the chunk -- and behind it the 16-entry boundary table of the one
// pair that straddles chunks c - 1 and c, indexed by bits [8c - 2, 8c + 2) of the look-ahead buffer: the last base of
// byte c - 1 (low) and the first of byte c (chunk 0 has no such pair; its 16 entries are not read).
constexpr int DN_STRIDE = 256 + 16;

__device__ __forceinline__ uint32_t pair_of(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3, int c) {
  // (c >= 1 is a compile-time constant after unrolling; c = 4, 8, 12: the pair crosses a register)
  const uint32_t hi = c < 4 ? b0 : c < 8 ? b1 : c < 12 ? b2 : b3;
  const uint32_t lo = c <= 4 ? b0 : c <= 8 ? b1 : b2;
  const uint32_t v = (c & 3) ? hi >> (8 * (c & 3) - 2) : __builtin_amdgcn_alignbit(hi, lo, 30);
  return v & 15u;
}

// walk_sequence for first-order tables, a sibling (the order-0 kernels keep their code: DESIGN.md 9.5); one motif per pass
template <bool BOTH, class Visit>
__device__ __forceinline__ void walk_sequence_dinuc(const uint64_t* wp, const uint32_t* vp, uint32_t L, const int32_t* tab,
                                                    const MotifRec* mrec, int nrec, Visit& v) {
  const uint32_t nw = (L + 31u) >> 5;
  auto ldw = [&](uint32_t j) -> uint64_t { return j < nw ? wp[j] : 0ull; };
  auto ldv = [&](uint32_t j) -> uint32_t {
    if (j >= nw) return 0u;
    if (vp) return vp[j];
    const uint32_t rem = L - 32u * j;
    return rem >= 32u ? 0xFFFFFFFFu : ((1u << rem) - 1u);
  };
  for (int r = 0; r < nrec; ++r) {
    const MotifRec mr = mrec[r];
    const uint64_t wmask = mr.w >= 64 ? ~0ull : ((1ull << mr.w) - 1ull);
    const int nch = mr.nch;
    const int32_t* tf = tab + mr.off;
    v.begin(0, r);
    const uint32_t nwin = L >= (uint32_t)mr.w ? L - (uint32_t)mr.w + 1u : 0u;
    const uint64_t x0 = ldw(0), x1 = ldw(1);
    uint32_t b0 = (uint32_t)x0, b1 = (uint32_t)(x0 >> 32), b2 = (uint32_t)x1, b3 = (uint32_t)(x1 >> 32);
    uint64_t vb = (uint64_t)ldv(0) | ((uint64_t)ldv(1) << 32);
    for (uint32_t s = 0, j = 2; s < nwin; ++j) {
      uint64_t fw = ldw(j);
      uint32_t fv = ldv(j);
      const uint32_t cnt = nwin - s < 32u ? nwin - s : 32u;
      for (uint32_t k = 0; k < cnt; ++k) {
        if ((vb & wmask) == wmask) {
          int32_t sf = 0, sr = 0;
#pragma unroll
          for (int c = 0; c < MAX_CHUNKS; ++c) {
            if (c < nch) {
              const uint32_t idx = byte_of(b0, b1, b2, b3, c);
              sf += tf[c * DN_STRIDE + idx];
              if (BOTH) sr += tf[(nch + c) * DN_STRIDE + idx];
              if (c > 0) {
                const uint32_t px = pair_of(b0, b1, b2, b3, c);
                sf += tf[c * DN_STRIDE + 256 + px];
                if (BOTH) sr += tf[(nch + c) * DN_STRIDE + 256 + px];
              }
            }
          }
          v.window(0, s + k, sf, sr);
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
    v.end(0, r);
  }
}

template <bool BOTH>
__global__ __launch_bounds__(SCAN_THREADS) void motif_scan_dinuc_kernel(const uint64_t* __restrict__ words,
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
    BestVisit<BOTH> v{mrec, best_out, n_seq, i, {}};
    walk_sequence_dinuc<BOTH>(words + w0, valid ? valid + w0 : nullptr, L, tab, mrec, g.m1 - g.m0, v);
  }
}

}  // namespace

// (declared in scan_walk.h: erase.hip stages its motifs and sizes its grids the same way)
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

namespace {
int upload_staged(pengk_ctx* ctx, const std::vector<int32_t>& tables, const std::vector<MotifRec>& recs,
                  const std::vector<GroupRec>& groups, int n_motifs, const int32_t* h_thr, StagedMotifs* out);
}  // namespace

// chunk tables, motif records and groups (greedy, in motif order) -- and h_thr when given -- staged in ctx->d_score
int stage_motifs(pengk_ctx* ctx, int n_motifs, const int32_t* h_S, const int32_t* h_len, int strands, const int32_t* h_thr,
                 StagedMotifs* out) {
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
  return upload_staged(ctx, tables, recs, groups, n_motifs, h_thr, out);
}

namespace {

// tables, motif records and groups -- and h_thr when given -- into ctx->d_score
int upload_staged(pengk_ctx* ctx, const std::vector<int32_t>& tables, const std::vector<MotifRec>& recs,
                  const std::vector<GroupRec>& groups, int n_motifs, const int32_t* h_thr, StagedMotifs* out) {
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

// stage_motifs for the first-order scan: DN_STRIDE ints per chunk and strand.  In window positions j the + strand has
// the single term S0[x_0] at j = 0 and the pair terms D[j][4 x_{j-1} + x_j], j = 1 .. w - 1; the - strand, y_j = 3 -
// x_{w-1-j}, has S0[3 - x_{w-1}] at j = w - 1 and the pair terms D[w - j][4 (3 - x_j) + (3 - x_{j-1})].  A chunk's table
// sums the terms whose positions lie inside it (positions at or beyond w add nothing: the entries repeat over them).
int stage_motifs_dinuc(pengk_ctx* ctx, int n_motifs, const int32_t* h_S0, const int32_t* h_D, const int32_t* h_len, int strands,
                       StagedMotifs* out) {
  std::vector<int32_t> tables;
  std::vector<MotifRec> recs;
  std::vector<GroupRec> groups;
  for (int m = 0; m < n_motifs; ++m) {
    const int w = h_len[m], nch = (w + 3) / 4;
    const int need = nch * strands * DN_STRIDE;
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
    const int32_t* S0 = h_S0 + (size_t)m * 4;
    const int32_t* D = h_D + (size_t)m * PENGK_MAX_MOTIF_LEN * 16;
    // the pair term of positions (j - 1, j) holding the bases (a, b), j = 1 .. w - 1
    auto pair = [&](int st, int j, int a, int b) -> int32_t {
      return st == 0 ? D[j * 16 + 4 * a + b] : D[(w - j) * 16 + 4 * (3 - b) + (3 - a)];
    };
    for (int st = 0; st < strands; ++st)
      for (int c = 0; c < nch; ++c) {
        for (int idx = 0; idx < 256; ++idx) {
          int32_t v = 0;
          for (int k = 0; k < 4 && 4 * c + k < w; ++k) {
            const int j = 4 * c + k, b = (idx >> (2 * k)) & 3;
            if (st == 0 && j == 0) v += S0[b];
            if (st == 1 && j == w - 1) v += S0[3 - b];
            if (k > 0) v += pair(st, j, (idx >> (2 * k - 2)) & 3, b);
          }
          tables.push_back(v);
        }
        for (int px = 0; px < 16; ++px) tables.push_back(c > 0 ? pair(st, 4 * c, px & 3, px >> 2) : 0);
      }
  }
  return upload_staged(ctx, tables, recs, groups, n_motifs, nullptr, out);
}

// clamp(lround(100 log2(p / g)), -2000, 2000) in double: log_odds of host/motif_score.cpp
int32_t dinuc_log_odds(double p, double g) {
  const double v = 100.0 * std::log2(p / g);
  return (int32_t)std::lround(std::max(-2000.0, std::min(2000.0, v)));
}

// Lentz's continued fraction of the regularised incomplete beta: I_x(a, b) = x^a (1-x)^b / (a B(a, b)) * betacf(a, b, x),
// fast to converge for x < (a + 1) / (a + b + 2) (Numerical Recipes 6.4)
double betacf(double a, double b, double x) {
  const double FPMIN = 1e-300, EPS = 1e-16;
  const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
  auto tiny = [&](double v) { return std::fabs(v) < FPMIN ? FPMIN : v; };
  double c = 1.0, d = 1.0 / tiny(1.0 - qab * x / qap), h = d;
  for (int64_t i = 1; i <= (1 << 22); ++i) {
    const double m = (double)i, m2 = 2.0 * m;
    double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
    d = 1.0 / tiny(1.0 + aa * d);
    c = tiny(1.0 + aa / c);
    h *= d * c;
    aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
    d = 1.0 / tiny(1.0 + aa * d);
    c = tiny(1.0 + aa / c);
    const double del = d * c;
    h *= del;
    if (std::fabs(del - 1.0) < EPS) break;
  }
  return h;
}

// log10 P(X >= k) for X ~ Binomial(n, p) = log10 I_p(k, n - k + 1), in log space throughout: no underflow however small
// the tail (CentriMo's binomial test, which reports the same tail)
double log10_binomial_sf(uint64_t n, uint64_t k, double p) {
  if (k == 0 || p >= 1.0) return 0.0;
  if (p <= 0.0) return -INFINITY;
  const double a = (double)k, b = (double)(n - k) + 1.0;
  const double lbeta = std::lgamma(a) + std::lgamma(b) - std::lgamma(a + b);
  const double lfront = a * std::log(p) + b * std::log1p(-p) - lbeta;
  double ln;
  if (p < (a + 1.0) / (a + b + 2.0)) {
    ln = lfront - std::log(a) + std::log(betacf(a, b, p));
  } else {  // the upper tail is the larger part: 1 - I_{1-p}(b, a)
    const double q = std::exp(lfront - std::log(b)) * betacf(b, a, 1.0 - p);
    ln = q < 1.0 ? std::log1p(-q) : lfront - std::log(a) + std::log(betacf(a, b, p));  // (rounding: the direct form)
  }
  return ln / std::log(10.0);
}

// ---- the hypergeometric tail of --enrich (Loader 2000, "Fast and accurate computation of binomial probabilities") -----
// stirlerr(n) = log(n!) - log(sqrt(2 pi n) (n / e)^n), n >= 1: the series in 1 / n above 15, lgamma below
double stirlerr(double n) {
  const double S0 = 1.0 / 12.0, S1 = 1.0 / 360.0, S2 = 1.0 / 1260.0, S3 = 1.0 / 1680.0, S4 = 1.0 / 1188.0;
  const double HALF_LN_2PI = 0.918938533204672741780329736406;
  if (n <= 15.0) return std::lgamma(n + 1.0) - (n + 0.5) * std::log(n) + n - HALF_LN_2PI;
  const double nn = n * n;
  if (n > 500.0) return (S0 - S1 / nn) / n;
  if (n > 80.0) return (S0 - (S1 - S2 / nn) / nn) / n;
  if (n > 35.0) return (S0 - (S1 - (S2 - S3 / nn) / nn) / nn) / n;
  return (S0 - (S1 - (S2 - (S3 - S4 / nn) / nn) / nn) / nn) / n;
}

// bd0(x, np) = x log(x / np) + np - x, x > 0, np > 0: by its series in (x - np) / (x + np) where the direct form cancels
double bd0(double x, double np) {
  if (std::fabs(x - np) < 0.1 * (x + np)) {
    double v = (x - np) / (x + np);
    double s = (x - np) * v, ej = 2.0 * x * v;
    v = v * v;
    for (int j = 1; j < 1000; ++j) {
      ej *= v;
      const double s1 = s + ej / (double)(2 * j + 1);
      if (s1 == s) return s1;
      s = s1;
    }
    return s;
  }
  return x * std::log(x / np) + np - x;
}

// log of the Binomial(n, p) point mass at x (q = 1 - p, given apart so that neither is formed by a cancelling difference)
double log_dbinom(double x, double n, double p, double q) {
  if (p == 0.0) return x == 0.0 ? 0.0 : -INFINITY;
  if (q == 0.0) return x == n ? 0.0 : -INFINITY;
  if (x == 0.0) return n == 0.0 ? 0.0 : n * (p < 0.5 ? std::log1p(-p) : std::log(q));
  if (x == n) return n * (q < 0.5 ? std::log1p(-q) : std::log(p));
  const double lc = stirlerr(n) - stirlerr(x) - stirlerr(n - x) - bd0(x, n * p) - bd0(n - x, n * q);
  const double lf = 1.837877066409345483560659472811 + std::log(x) + std::log1p(-x / n);  // log(2 pi x (n - x) / n)
  return lc - 0.5 * lf;
}

// log P(X = x), X ~ Hypergeometric(N, K marked, n drawn), x inside the support: three binomial point masses at p = n / N
double log_dhyper(uint64_t N, uint64_t K, uint64_t n, uint64_t x) {
  const double p = (double)n / (double)N, q = (double)(N - n) / (double)N;
  return log_dbinom((double)x, (double)K, p, q) + log_dbinom((double)(n - x), (double)(N - K), p, q) -
         log_dbinom((double)n, (double)N, p, q);
}

// log10 P(X >= k) for the same X.  The point mass at the end of the shorter tail, then the ratio recurrence away from the
// mode, its terms relative to that point mass (they fall from 1.0: nothing under- or overflows): upwards from k when the
// terms fall from k on, else downwards from k - 1 and the complement.
double log10_hypergeom_sf(uint64_t N, uint64_t K, uint64_t n, uint64_t k) {
  const uint64_t lo = n + K > N ? n + K - N : 0, hi = std::min(K, n);
  if (k <= lo) return 0.0;
  if (k > hi) return -INFINITY;
  const double dN = (double)N, dK = (double)K, dn = (double)n;
  // P(x + 1) / P(x) = (K - x)(n - x) / ((x + 1)(N - K - n + x + 1))
  auto up = [&](double x) { return (dK - x) * (dn - x) / ((x + 1.0) * (dN - dK - dn + x + 1.0)); };
  const double LN10 = std::log(10.0);
  if (up((double)k) <= 1.0) {
    double term = 1.0, sum = 1.0;
    for (uint64_t x = k; x < hi; ++x) {
      term *= up((double)x);
      sum += term;
      if (term < sum * 1e-18) break;
    }
    return (log_dhyper(N, K, n, k) + std::log(sum)) / LN10;
  }
  // (k is at or below the mode: k - 1 >= lo is below it)
  double term = 1.0, sum = 1.0;
  for (uint64_t x = k - 1; x > lo; --x) {
    term /= up((double)(x - 1));
    sum += term;
    if (term < sum * 1e-18) break;
  }
  const double lower = std::exp(log_dhyper(N, K, n, k - 1) + std::log(sum));
  return lower < 1.0 ? std::log1p(-lower) / LN10 : -INFINITY;
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
  if (both_strands)
    hipLaunchKernelGGL(motif_scan_kernel<true>, grid, dim3(SCAN_THREADS), 0, ctx->stream, d_words, d_valid, d_offs, d_lens, n_seq,
                       st.tables, st.recs, st.groups, d_best);
  else
    hipLaunchKernelGGL(motif_scan_kernel<false>, grid, dim3(SCAN_THREADS), 0, ctx->stream, d_words, d_valid, d_offs, d_lens, n_seq,
                       st.tables, st.recs, st.groups, d_best);
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

int pengk_score_tail_pvalues(const int32_t* h_S, int w, const float* h_bg, int32_t* lo_out, int32_t* hi_out, double* h_tail) {
  if (!h_S || !h_bg || !lo_out || !hi_out || w < 1 || w > PENGK_MAX_MOTIF_LEN)
    return fail(PENGK_ERR_ARG, "pengk_score_tail_pvalues: bad argument");
  int32_t lo = 0, hi = 0;
  for (int j = 0; j < w; ++j) {
    int32_t mn = 2000, mx = -2000;
    for (int a = 0; a < 4; ++a) {
      const int32_t v = h_S[j * 4 + a];
      if (v < -2000 || v > 2000) return fail(PENGK_ERR_ARG, "pengk_score_tail_pvalues: log-odds %d outside [-2000, 2000]", v);
      mn = std::min(mn, v);
      mx = std::max(mx, v);
    }
    lo += mn;
    hi += mx;
  }
  *lo_out = lo;
  *hi_out = hi;
  if (!h_tail) return PENGK_OK;
  double bg[4];
  for (int a = 0; a < 4; ++a) bg[a] = (double)h_bg[a];
  // q_j over the scores [clo, chi] of the first j columns; q_{j+1}[t] = sum over a = 0..3, in this order, of
  // q_j[t - S[j][a]] * bg[a], each from 0.0
  const size_t n = (size_t)(hi - lo) + 1;
  std::vector<double> q(n, 0.0), nq(n, 0.0);
  q[0] = 1.0;
  int32_t clo = 0, chi = 0;
  for (int j = 0; j < w; ++j) {
    int32_t mn = 2000, mx = -2000;
    for (int a = 0; a < 4; ++a) {
      mn = std::min(mn, h_S[j * 4 + a]);
      mx = std::max(mx, h_S[j * 4 + a]);
    }
    const int32_t nlo = clo + mn, nhi = chi + mx;
    for (int32_t t = nlo; t <= nhi; ++t) {
      double v = 0.0;
      for (int a = 0; a < 4; ++a) {
        const int32_t u = t - h_S[j * 4 + a];
        if (u >= clo && u <= chi) v += q[(size_t)(u - clo)] * bg[a];
      }
      nq[(size_t)(t - nlo)] = v;
    }
    q.swap(nq);
    clo = nlo;
    chi = nhi;
  }
  // the tail, summed from the highest score down
  double acc = 0.0;
  for (int64_t t = hi; t >= lo; --t) {
    acc += q[(size_t)(t - lo)];
    h_tail[t - lo] = acc;
  }
  return PENGK_OK;
}

int pengk_score_threshold(const double* h_tail, int32_t lo, int32_t hi, double p, int32_t* t_out) {
  if (!h_tail || !t_out || hi < lo || !(p > 0.0 && p <= 1.0)) return fail(PENGK_ERR_ARG, "pengk_score_threshold: bad argument");
  int32_t t = lo;
  while (t <= hi && !(h_tail[t - lo] <= p)) ++t;
  *t_out = t;
  return PENGK_OK;
}

int pengk_sites_count(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                      const uint32_t* d_lens, uint64_t n_seq, int n_motifs, const int32_t* h_S, const int32_t* h_len,
                      int both_strands, const int32_t* h_thr, uint64_t* d_counts) {
  if (!ctx || n_motifs < 0 || (n_motifs && (!h_S || !h_len || !h_thr)) ||
      (n_seq && n_motifs && (!d_words || !d_offs || !d_lens || !d_counts)))
    return fail(PENGK_ERR_ARG, "pengk_sites_count: bad argument");
  int rc = check_motifs("pengk_sites_count", n_motifs, h_S, h_len);
  if (rc) return rc;
  SCORE_ENTER(ctx);
  if (n_seq == 0 || n_motifs == 0) return PENGK_OK;
  StagedMotifs st;
  rc = stage_motifs(ctx, n_motifs, h_S, h_len, both_strands ? 2 : 1, h_thr, &st);
  if (rc) return rc;
  const dim3 grid(grid_for(ctx, n_seq, SCAN_THREADS, 8), (unsigned)st.n_groups);
  unsigned long long* c = (unsigned long long*)d_counts;
  if (both_strands)
    hipLaunchKernelGGL((motif_sites_kernel<true, false>), grid, dim3(SCAN_THREADS), 0, ctx->stream, d_words, d_valid, d_offs, d_lens,
                       (uint64_t)0, n_seq, n_seq, st.tables, st.recs, st.groups, st.thr, c, nullptr, nullptr, (uint64_t)0);
  else
    hipLaunchKernelGGL((motif_sites_kernel<false, false>), grid, dim3(SCAN_THREADS), 0, ctx->stream, d_words, d_valid, d_offs, d_lens,
                       (uint64_t)0, n_seq, n_seq, st.tables, st.recs, st.groups, st.thr, c, nullptr, nullptr, (uint64_t)0);
  PENGK_HIP(hipGetLastError());
  return PENGK_OK;
}

int pengk_sites_histograms(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                           const uint32_t* d_lens, uint64_t n_seq, int n_motifs, const int32_t* h_S, const int32_t* h_len,
                           int both_strands, const int32_t* h_thr, const int32_t* h_hi, const uint64_t* h_hist_offs,
                           uint64_t* d_hist, uint64_t* d_tests, uint64_t* d_counts) {
  if (!ctx || n_motifs < 0 || (n_motifs && (!h_S || !h_len || !h_thr || !h_hi || !h_hist_offs || !d_tests)) ||
      (n_seq && n_motifs && (!d_words || !d_offs || !d_lens)))
    return fail(PENGK_ERR_ARG, "pengk_sites_histograms: bad argument");
  int rc = check_motifs("pengk_sites_histograms", n_motifs, h_S, h_len);
  if (rc) return rc;
  // every score must have its bin: h_hi[m] at or above the sum of the column maxima, and bins to add to
  for (int m = 0; m < n_motifs; ++m) {
    int32_t mx = 0;
    for (int j = 0; j < h_len[m]; ++j) {
      const int32_t* c = h_S + ((size_t)m * PENGK_MAX_MOTIF_LEN + j) * 4;
      mx += std::max(std::max(c[0], c[1]), std::max(c[2], c[3]));
    }
    if (h_hi[m] < mx) return fail(PENGK_ERR_ARG, "pengk_sites_histograms: motif %d: hi %d below its best score %d", m, h_hi[m], mx);
    if (h_hi[m] >= h_thr[m] && !d_hist) return fail(PENGK_ERR_ARG, "pengk_sites_histograms: bad argument");
  }
  SCORE_ENTER(ctx);
  if (n_seq == 0 || n_motifs == 0) return PENGK_OK;
  const size_t hb = ((size_t)n_motifs * sizeof(int32_t) + 7) & ~(size_t)7;
  std::vector<char> staged(hb + (size_t)n_motifs * sizeof(uint64_t));
  memcpy(staged.data(), h_hi, (size_t)n_motifs * sizeof(int32_t));
  memcpy(staged.data() + hb, h_hist_offs, (size_t)n_motifs * sizeof(uint64_t));
  rc = ensure_scratch(ctx, &ctx->d_misc, &ctx->misc_bytes, staged.size());
  if (rc) return rc;
  StagedMotifs st;
  rc = stage_motifs(ctx, n_motifs, h_S, h_len, both_strands ? 2 : 1, h_thr, &st);  // (synchronises with the stream)
  if (rc) return rc;
  PENGK_HIP(hipMemcpy(ctx->d_misc, staged.data(), staged.size(), hipMemcpyHostToDevice));
  const int32_t* d_hi = (const int32_t*)ctx->d_misc;
  const uint64_t* d_ho = (const uint64_t*)((char*)ctx->d_misc + hb);
  const dim3 grid(grid_for(ctx, n_seq, SCAN_THREADS, 8), (unsigned)st.n_groups);
  unsigned long long* h = (unsigned long long*)d_hist;
  unsigned long long* t = (unsigned long long*)d_tests;
  unsigned long long* c = (unsigned long long*)d_counts;
  if (both_strands)
    hipLaunchKernelGGL(motif_sites_hist_kernel<true>, grid, dim3(SCAN_THREADS), 0, ctx->stream, d_words, d_valid, d_offs, d_lens,
                       n_seq, st.tables, st.recs, st.groups, st.thr, d_hi, d_ho, h, t, c);
  else
    hipLaunchKernelGGL(motif_sites_hist_kernel<false>, grid, dim3(SCAN_THREADS), 0, ctx->stream, d_words, d_valid, d_offs, d_lens,
                       n_seq, st.tables, st.recs, st.groups, st.thr, d_hi, d_ho, h, t, c);
  PENGK_HIP(hipGetLastError());
  return PENGK_OK;
}

int pengk_motif_enrich(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                       const uint32_t* d_lens, uint64_t n_seq, int n_motifs, const int32_t* h_S, const int32_t* h_len,
                       int both_strands, const int32_t* h_thr, const int32_t* h_hi, const uint64_t* h_hist_offs,
                       uint64_t* d_hist, uint64_t* d_scored) {
  if (!ctx || n_motifs < 0 || (n_motifs && (!h_S || !h_len || !h_thr || !h_hi || !h_hist_offs || !d_scored)) ||
      (n_seq && n_motifs && (!d_words || !d_offs || !d_lens)))
    return fail(PENGK_ERR_ARG, "pengk_motif_enrich: bad argument");
  // (what keeps a 32-bit private bin from wrapping without a flush inside the loop: a sequence adds once per motif)
  if (n_seq >= (1ull << 32)) return fail(PENGK_ERR_ARG, "pengk_motif_enrich: n_seq %llu (below 2^32)", (unsigned long long)n_seq);
  int rc = check_motifs("pengk_motif_enrich", n_motifs, h_S, h_len);
  if (rc) return rc;
  // every score must have its bin: h_hi[m] at or above the sum of the column maxima, and bins to add to
  for (int m = 0; m < n_motifs; ++m) {
    int32_t mx = 0;
    for (int j = 0; j < h_len[m]; ++j) {
      const int32_t* c = h_S + ((size_t)m * PENGK_MAX_MOTIF_LEN + j) * 4;
      mx += std::max(std::max(c[0], c[1]), std::max(c[2], c[3]));
    }
    if (h_hi[m] < mx) return fail(PENGK_ERR_ARG, "pengk_motif_enrich: motif %d: hi %d below its best score %d", m, h_hi[m], mx);
    if (h_hi[m] >= h_thr[m] && !d_hist) return fail(PENGK_ERR_ARG, "pengk_motif_enrich: bad argument");
  }
  SCORE_ENTER(ctx);
  if (n_seq == 0 || n_motifs == 0) return PENGK_OK;
  const int strands = both_strands ? 2 : 1;
  const int64_t per_launch = ctx->enrich_groups_per_launch;
  unsigned long long* h = (unsigned long long*)d_hist;
  unsigned long long* sc = (unsigned long long*)d_scored;
  // batches of whole motif groups: the groups are stage_motifs' (greedy, in motif order), so a batch that starts where a
  // group starts is cut into the groups the whole set would be cut into
  for (int m0 = 0; m0 < n_motifs;) {
    int m1 = m0, ints = 0;
    int64_t n_groups = 1;
    for (; m1 < n_motifs; ++m1) {
      const int need = (h_len[m1] + 3) / 4 * strands * 256;
      if (ints + need > SCAN_TABLES * 256) {
        if (n_groups == per_launch) break;
        ++n_groups;
        ints = 0;
      }
      ints += need;
    }
    const int nb = m1 - m0;
    const size_t hb = ((size_t)nb * sizeof(int32_t) + 7) & ~(size_t)7;
    std::vector<char> staged(hb + (size_t)nb * sizeof(uint64_t));
    memcpy(staged.data(), h_hi + m0, (size_t)nb * sizeof(int32_t));
    memcpy(staged.data() + hb, h_hist_offs + m0, (size_t)nb * sizeof(uint64_t));
    rc = ensure_scratch(ctx, &ctx->d_misc, &ctx->misc_bytes, staged.size());
    if (rc) return rc;
    StagedMotifs st;
    rc = stage_motifs(ctx, nb, h_S + (size_t)m0 * PENGK_MAX_MOTIF_LEN * 4, h_len + m0, strands, h_thr + m0, &st);  // (synchronises)
    if (rc) return rc;
    if (st.n_groups != (int)n_groups) return fail(PENGK_ERR_RANGE, "pengk_motif_enrich: %d groups staged, %d planned", st.n_groups, (int)n_groups);
    PENGK_HIP(hipMemcpy(ctx->d_misc, staged.data(), staged.size(), hipMemcpyHostToDevice));
    const int32_t* d_hi = (const int32_t*)ctx->d_misc;
    const uint64_t* d_ho = (const uint64_t*)((char*)ctx->d_misc + hb);
    const dim3 grid(grid_for(ctx, n_seq, SCAN_THREADS, 8), (unsigned)st.n_groups);
    // (the records carry motif indices within the batch: the scored counters are passed from the batch's first motif on;
    // the histogram offsets are the caller's, from d_hist)
    if (both_strands)
      hipLaunchKernelGGL(motif_enrich_kernel<true>, grid, dim3(SCAN_THREADS), 0, ctx->stream, d_words, d_valid, d_offs, d_lens, n_seq,
                         st.tables, st.recs, st.groups, st.thr, d_hi, d_ho, h, sc + m0);
    else
      hipLaunchKernelGGL(motif_enrich_kernel<false>, grid, dim3(SCAN_THREADS), 0, ctx->stream, d_words, d_valid, d_offs, d_lens, n_seq,
                         st.tables, st.recs, st.groups, st.thr, d_hi, d_ho, h, sc + m0);
    PENGK_HIP(hipGetLastError());
    m0 = m1;
  }
  return PENGK_OK;
}

int pengk_hypergeom_log10_sf(uint64_t N, uint64_t K, uint64_t n, uint64_t k, double* out) {
  if (!out || K > N || n > N) return fail(PENGK_ERR_ARG, "pengk_hypergeom_log10_sf: bad argument");
  *out = log10_hypergeom_sf(N, K, n, k);
  return PENGK_OK;
}

int pengk_enrich_summary(const uint64_t* h_pos, const uint64_t* h_neg, uint64_t nbins, int32_t thr, uint64_t n_pos,
                         uint64_t n_neg, pengk_enrichment* out) {
  if (!out || (nbins && (!h_pos || !h_neg)) || nbins > (1ull << 31) || (int64_t)thr + (int64_t)nbins > (int64_t)INT32_MAX ||
      n_pos + n_neg < n_pos)
    return fail(PENGK_ERR_ARG, "pengk_enrich_summary: bad argument");
  uint64_t a = 0, b = 0;
  for (uint64_t k = 0; k < nbins; ++k) {
    if (h_pos[k] > n_pos - a || h_neg[k] > n_neg - b)
      return fail(PENGK_ERR_ARG, "pengk_enrich_summary: more hits than scored sequences");
    a += h_pos[k];
    b += h_neg[k];
  }
  memset(out, 0, sizeof *out);
  out->threshold = (int32_t)((int64_t)thr + (int64_t)nbins);
  const uint64_t N = n_pos + n_neg;
  a = b = 0;
  for (uint64_t k = nbins; k-- > 0;) {
    a += h_pos[k];
    b += h_neg[k];
    if (h_pos[k] + h_neg[k] == 0) continue;  // (the tail of the threshold above: not a test of its own)
    const double lp = log10_hypergeom_sf(N, a + b, n_pos, a);
    if (out->n_thresholds == 0 || lp < out->log10_pvalue) {  // (from the top down: the higher threshold wins a tie)
      out->threshold = (int32_t)((int64_t)thr + (int64_t)k);
      out->pos_hits = a;
      out->neg_hits = b;
      out->log10_pvalue = lp;
    }
    ++out->n_thresholds;
  }
  out->enrichment = (((double)out->pos_hits + 1.0) / ((double)n_pos + 1.0)) / (((double)out->neg_hits + 1.0) / ((double)n_neg + 1.0));
  out->log10_adj_pvalue = out->n_thresholds ? std::min(0.0, out->log10_pvalue + std::log10((double)out->n_thresholds)) : 0.0;
  return PENGK_OK;
}

int pengk_sites_qvalues(const uint64_t* h_hist, uint64_t nbins, uint64_t n_tests, const double* h_tail_from_thr, double* h_q) {
  if (nbins && (!h_hist || !h_tail_from_thr || !h_q)) return fail(PENGK_ERR_ARG, "pengk_sites_qvalues: bad argument");
  // r(s) = N * tail / n(s), the ranks n(s) summed from the highest score down
  const double N = (double)n_tests;
  uint64_t n = 0;
  for (uint64_t k = nbins; k-- > 0;) {
    n += h_hist[k];
    if (n > 0) {
      const double x = N * h_tail_from_thr[k];
      h_q[k] = x / (double)n;
    } else {
      h_q[k] = INFINITY;
    }
  }
  // q(s) = min(1, min over s' <= s of r(s')), a running minimum from the threshold up
  double mn = INFINITY;
  for (uint64_t k = 0; k < nbins; ++k) {
    if (h_q[k] < mn) mn = h_q[k];
    h_q[k] = mn < 1.0 ? mn : 1.0;
  }
  return PENGK_OK;
}

int pengk_qvalue_threshold(const double* h_q, uint64_t nbins, int32_t t, double q_max, int32_t* t_out) {
  if (!t_out || (nbins && !h_q) || !(q_max >= 0.0) || (int64_t)t + (int64_t)nbins > (int64_t)INT32_MAX || nbins > (1ull << 32))
    return fail(PENGK_ERR_ARG, "pengk_qvalue_threshold: bad argument");
  uint64_t k = 0;
  while (k < nbins && !(h_q[k] <= q_max)) ++k;
  *t_out = (int32_t)((int64_t)t + (int64_t)k);
  return PENGK_OK;
}

int pengk_sites_slices(pengk_ctx* ctx, const uint64_t* d_counts, uint64_t n_seq, int n_motifs, uint64_t* h_motif_totals,
                       uint64_t max_slices, uint64_t* h_bounds, uint64_t* h_records, uint64_t* n_slices) {
  if (!ctx || n_motifs < 0 || !n_slices || (n_motifs && !h_motif_totals) || (max_slices && (!h_bounds || !h_records)) ||
      (n_seq && n_motifs && !d_counts))
    return fail(PENGK_ERR_ARG, "pengk_sites_slices: bad argument");
  SCORE_ENTER(ctx);
  *n_slices = 0;
  for (int m = 0; m < n_motifs; ++m) h_motif_totals[m] = 0;
  if (n_seq == 0) return PENGK_OK;
  const uint64_t nb = (n_seq + SITES_BLOCK - 1) / SITES_BLOCK;
  std::vector<uint64_t> bt(nb, 0);
  unsigned long long *seq_tot = nullptr, *block_tot = nullptr;
  if (n_motifs) {
    const size_t bytes = (n_seq + nb + (size_t)n_motifs) * sizeof(uint64_t);
    int rc = ensure_scratch(ctx, &ctx->d_sites, &ctx->sites_bytes, bytes);
    if (rc) return rc;
    seq_tot = (unsigned long long*)ctx->d_sites;
    block_tot = seq_tot + n_seq;
    unsigned long long* mtot = block_tot + nb;
    PENGK_HIP(hipMemsetAsync(mtot, 0, (size_t)n_motifs * sizeof(uint64_t), ctx->stream));
    hipLaunchKernelGGL(site_totals_kernel, dim3((unsigned)nb), dim3(SITES_THREADS), 0, ctx->stream,
                       (const unsigned long long*)d_counts, n_seq, n_motifs, seq_tot, block_tot, mtot);
    PENGK_HIP(hipGetLastError());
    PENGK_HIP(hipMemcpyAsync(bt.data(), block_tot, nb * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    PENGK_HIP(hipMemcpyAsync(h_motif_totals, mtot, (size_t)n_motifs * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    PENGK_HIP(hipStreamSynchronize(ctx->stream));
  }
  // slices of whole blocks while their records fit the budget; a block above it alone is cut between its sequences, and a
  // sequence above it is a slice of its own
  const uint64_t B = ctx->sites_record_budget;
  const uint64_t MAX_SEQ = 1ull << 31;  // (a record's sequence is an index into its slice: uint32)
  uint64_t ns = 0, i0 = 0, acc = 0;
  auto close = [&](uint64_t i1) {
    if (ns < max_slices) {
      h_bounds[ns] = i0;
      h_bounds[ns + 1] = i1;
      h_records[ns] = acc;
    }
    ++ns;
    i0 = i1;
    acc = 0;
  };
  std::vector<uint64_t> st;
  for (uint64_t b = 0; b < nb; ++b) {
    const uint64_t bb = b * SITES_BLOCK, be = std::min<uint64_t>(n_seq, bb + SITES_BLOCK);
    if (be - i0 > MAX_SEQ) close(bb);
    if (acc + bt[b] <= B) {
      acc += bt[b];
      continue;
    }
    if (bt[b] <= B) {
      close(bb);
      acc = bt[b];
      continue;
    }
    st.resize(be - bb);
    PENGK_HIP(hipMemcpy(st.data(), seq_tot + bb, (be - bb) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    for (uint64_t i = bb; i < be; ++i) {
      const uint64_t t = st[i - bb];
      if (acc + t > B && i > i0) close(i);
      acc += t;
    }
  }
  close(n_seq);
  *n_slices = ns;
  return PENGK_OK;
}

int pengk_sites_emit(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                     const uint32_t* d_lens, uint64_t n_seq, int n_motifs, const int32_t* h_S, const int32_t* h_len,
                     int both_strands, const int32_t* h_thr, const uint64_t* d_counts, uint64_t i0, uint64_t i1,
                     pengk_site* d_sites, uint64_t cap) {
  if (!ctx || n_motifs < 0 || i0 > i1 || i1 > n_seq || i1 - i0 > (1ull << 31) || (n_motifs && (!h_S || !h_len || !h_thr)) ||
      (i1 > i0 && n_motifs && (!d_words || !d_offs || !d_lens || !d_counts || (cap && !d_sites))))
    return fail(PENGK_ERR_ARG, "pengk_sites_emit: bad argument");
  int rc = check_motifs("pengk_sites_emit", n_motifs, h_S, h_len);
  if (rc) return rc;
  SCORE_ENTER(ctx);
  if (i1 == i0 || n_motifs == 0) return PENGK_OK;
  const uint64_t ns = i1 - i0, n = ns * (uint64_t)n_motifs, n_tiles = (n + XS_TILE - 1) / XS_TILE;
  StagedMotifs st;
  rc = stage_motifs(ctx, n_motifs, h_S, h_len, both_strands ? 2 : 1, h_thr, &st);
  if (rc) return rc;
  rc = ensure_scratch(ctx, &ctx->d_sites, &ctx->sites_bytes, (n + n_tiles) * sizeof(uint64_t));
  if (rc) return rc;
  unsigned long long* so = (unsigned long long*)ctx->d_sites;
  unsigned long long* part = so + n;
  const unsigned long long* c = (const unsigned long long*)d_counts;
  // where each (motif, sequence) writes: the exclusive scan of the counts, motif-major
  hipLaunchKernelGGL(xscan_tiles_kernel, dim3((unsigned)n_tiles), dim3(SITES_THREADS), 0, ctx->stream, c, n_seq, i0, ns, n, part);
  hipLaunchKernelGGL(xscan_parts_kernel, dim3(1), dim3(SITES_THREADS), 0, ctx->stream, part, n_tiles);
  hipLaunchKernelGGL(xscan_apply_kernel, dim3((unsigned)n_tiles), dim3(SITES_THREADS), 0, ctx->stream, c, n_seq, i0, ns, n, part, so);
  PENGK_HIP(hipGetLastError());
  const dim3 grid(grid_for(ctx, ns, SCAN_THREADS, 8), (unsigned)st.n_groups);
  if (both_strands)
    hipLaunchKernelGGL((motif_sites_kernel<true, true>), grid, dim3(SCAN_THREADS), 0, ctx->stream, d_words, d_valid, d_offs, d_lens, i0,
                       i1, n_seq, st.tables, st.recs, st.groups, st.thr, nullptr, so, d_sites, cap);
  else
    hipLaunchKernelGGL((motif_sites_kernel<false, true>), grid, dim3(SCAN_THREADS), 0, ctx->stream, d_words, d_valid, d_offs, d_lens, i0,
                       i1, n_seq, st.tables, st.recs, st.groups, st.thr, nullptr, so, d_sites, cap);
  PENGK_HIP(hipGetLastError());
  return PENGK_OK;
}

int pengk_motif_best_sites(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                           const uint32_t* d_lens, uint64_t n_seq, uint64_t seq0, int n_motifs, const int32_t* h_S,
                           const int32_t* h_len, int both_strands, int32_t* d_best, uint64_t* d_site) {
  if (!ctx || n_motifs < 0 || (n_motifs && (!h_S || !h_len)) ||
      (n_seq && n_motifs && (!d_words || !d_offs || !d_lens || !d_best || !d_site)))
    return fail(PENGK_ERR_ARG, "pengk_motif_best_sites: bad argument");
  int rc = check_motifs("pengk_motif_best_sites", n_motifs, h_S, h_len);
  if (rc) return rc;
  SCORE_ENTER(ctx);
  if (n_seq == 0 || n_motifs == 0) return PENGK_OK;
  StagedMotifs st;
  rc = stage_motifs(ctx, n_motifs, h_S, h_len, both_strands ? 2 : 1, nullptr, &st);
  if (rc) return rc;
  const dim3 grid(grid_for(ctx, n_seq, SCAN_THREADS, 8), (unsigned)st.n_groups);
  unsigned long long* site = (unsigned long long*)d_site;
  if (both_strands)
    hipLaunchKernelGGL(motif_best_site_kernel<true>, grid, dim3(SCAN_THREADS), 0, ctx->stream, d_words, d_valid, d_offs, d_lens,
                       n_seq, seq0, st.tables, st.recs, st.groups, d_best, site);
  else
    hipLaunchKernelGGL(motif_best_site_kernel<false>, grid, dim3(SCAN_THREADS), 0, ctx->stream, d_words, d_valid, d_offs, d_lens,
                       n_seq, seq0, st.tables, st.recs, st.groups, d_best, site);
  PENGK_HIP(hipGetLastError());
  return PENGK_OK;
}

int pengk_centrality_histograms(pengk_ctx* ctx, int n_motifs, const int32_t* d_best, const uint64_t* d_site,
                                const uint32_t* d_lens, uint64_t n_seq, const int32_t* h_len, const int32_t* h_thr,
                                uint32_t max_len, uint64_t* d_hist_offsets, uint64_t* d_hist_lengths) {
  if (!ctx || n_motifs < 0 || max_len < 1 || max_len > PENGK_CENTRALITY_MAX_LEN ||
      (n_motifs && (!h_len || !h_thr || !d_hist_offsets || !d_hist_lengths)) || (n_seq && n_motifs && (!d_best || !d_site || !d_lens)))
    return fail(PENGK_ERR_ARG, "pengk_centrality_histograms: bad argument");
  for (int m = 0; m < n_motifs; ++m)
    if (h_len[m] < 1 || h_len[m] > PENGK_MAX_MOTIF_LEN)
      return fail(PENGK_ERR_ARG, "pengk_centrality_histograms: motif %d has width %d (1..%d)", m, h_len[m], PENGK_MAX_MOTIF_LEN);
  SCORE_ENTER(ctx);
  if (n_seq == 0 || n_motifs == 0) return PENGK_OK;
  std::vector<int32_t> wt(2 * (size_t)n_motifs);
  for (int m = 0; m < n_motifs; ++m) {
    wt[2 * m] = h_len[m];
    wt[2 * m + 1] = h_thr[m];
  }
  int rc = ensure_scratch(ctx, &ctx->d_misc, &ctx->misc_bytes, wt.size() * sizeof(int32_t));
  if (rc) return rc;
  PENGK_HIP(hipStreamSynchronize(ctx->stream));
  PENGK_HIP(hipMemcpy(ctx->d_misc, wt.data(), wt.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  const uint64_t per_motif = std::max<uint64_t>(1, std::min<uint64_t>((n_seq + HIST_THREADS - 1) / HIST_THREADS,
                                                                      (uint64_t)ctx->num_cu * 2 / (uint64_t)n_motifs + 1));
  const dim3 grid((unsigned)per_motif, (unsigned)n_motifs);
  const bool lds = 3ull * max_len + 2 <= (uint64_t)CENT_LDS_BINS && n_seq >= (uint64_t)HIST_THREADS * 16;
  const unsigned long long* site = (const unsigned long long*)d_site;
  unsigned long long* hd = (unsigned long long*)d_hist_offsets;
  unsigned long long* hl = (unsigned long long*)d_hist_lengths;
  if (lds)
    hipLaunchKernelGGL(centrality_hist_kernel<true>, grid, dim3(HIST_THREADS), 0, ctx->stream, d_best, site, d_lens, n_seq,
                       (const int32_t*)ctx->d_misc, max_len, hd, hl);
  else
    hipLaunchKernelGGL(centrality_hist_kernel<false>, grid, dim3(HIST_THREADS), 0, ctx->stream, d_best, site, d_lens, n_seq,
                       (const int32_t*)ctx->d_misc, max_len, hd, hl);
  PENGK_HIP(hipGetLastError());
  return PENGK_OK;
}

int pengk_binomial_log10_sf(uint64_t n, uint64_t k, double p, double* out) {
  if (!out || k > n || !(p >= 0.0 && p <= 1.0)) return fail(PENGK_ERR_ARG, "pengk_binomial_log10_sf: bad argument");
  *out = log10_binomial_sf(n, k, p);
  return PENGK_OK;
}

int pengk_centrality_summary(const uint64_t* h_hist_offsets, const uint64_t* h_hist_lengths, uint32_t max_len, int w,
                             int n_motifs, pengk_centrality* out) {
  if (!h_hist_offsets || !h_hist_lengths || !out || max_len < 1 || max_len > PENGK_CENTRALITY_MAX_LEN || w < 1 ||
      w > PENGK_MAX_MOTIF_LEN || n_motifs < 1)
    return fail(PENGK_ERR_ARG, "pengk_centrality_summary: bad argument");
  memset(out, 0, sizeof *out);
  const int64_t C0 = max_len;  // bin of d = 0
  // N, Dm and the sites' offsets against the lengths they can come from
  uint64_t N = 0, Nd = 0;
  int64_t Dm = -1;
  for (uint32_t L = 0; L <= max_len; ++L) {
    const uint64_t n = h_hist_lengths[L];
    if (!n) continue;
    if ((int64_t)L < w) return fail(PENGK_ERR_ARG, "pengk_centrality_summary: sites on a sequence shorter than the motif");
    N += n;
    Dm = (int64_t)L - w;
  }
  for (int64_t b = 0; b <= 2 * C0; ++b) {
    const uint64_t n = h_hist_offsets[b];
    if (!n) continue;
    if (std::abs(b - C0) > Dm) return fail(PENGK_ERR_ARG, "pengk_centrality_summary: offset beyond the longest sequence");
    Nd += n;
  }
  if (N != Nd) return fail(PENGK_ERR_ARG, "pengk_centrality_summary: the histograms hold different totals");
  out->sites = N;
  if (N == 0) return PENGK_OK;
  out->max_offset = (uint32_t)Dm;
  // N p(r) = sum_L n_L #{p : |2p + w - L| <= r} / (D + 1), D = L - w: #{...} = D + 1 for r >= D, else r + [r = D mod 2].
  // By D: N p(r) = r (A_0(r) + A_1(r)) + A_{r mod 2}(r) + B(r) with A_par(r) = sum over D > r, D = par (mod 2) of
  // n_D / (D + 1) and B(r) = sum over D <= r of n_D -- suffix and prefix sums: O(Dm + lengths), not their product.
  const size_t nD = (size_t)Dm + 1;
  std::vector<double> A0(nD + 1, 0.0), A1(nD + 1, 0.0);  // A_par over D >= r (shifted by one below)
  std::vector<uint64_t> cnt(nD, 0), hit0(nD + 1, 0), hit1(nD + 1, 0);  // n_D; sites of D >= r by parity
  for (int64_t D = 0; D <= Dm; ++D) cnt[D] = h_hist_lengths[D + w];
  for (int64_t D = Dm; D >= 0; --D) {
    const double c = (double)cnt[D] / (double)(D + 1);
    A0[D] = A0[D + 1] + ((D & 1) ? 0.0 : c);
    A1[D] = A1[D + 1] + ((D & 1) ? c : 0.0);
    hit0[D] = hit0[D + 1] + ((D & 1) ? 0 : cnt[D]);
    hit1[D] = hit1[D + 1] + ((D & 1) ? cnt[D] : 0);
  }
  uint64_t below = 0, K = h_hist_offsets[C0];
  double best = 0.0;
  bool have = false;
  for (int64_t r = 0; r <= Dm; ++r) {
    below += cnt[r];  // B(r)
    if (r) K += h_hist_offsets[C0 - r] + h_hist_offsets[C0 + r];
    // r is a window of its own only if a sequence has an offset of its parity at distance r: otherwise p(r) and K(r)
    // equal those of r - 1 exactly (and p(0) = K(0) = 0), a tie that the smaller r wins
    if (((r & 1) ? hit1[r] : hit0[r]) == 0) continue;
    const double a0 = A0[r + 1], a1 = A1[r + 1];
    const double np = (double)r * (a0 + a1) + ((r & 1) ? a1 : a0) + (double)below;
    const double pbar = std::min(1.0, np / (double)N);
    const double lp = log10_binomial_sf(N, K, pbar);
    if (!have || lp < best) {
      have = true;
      best = lp;
      out->window = (uint32_t)r;
      out->in_window = K;
      out->expected = np;
      out->log10_pvalue = lp;
    }
  }
  out->log10_evalue = out->log10_pvalue + std::log10((double)(Dm + 1)) + std::log10((double)n_motifs);
  return PENGK_OK;
}

int pengk_spacing_histograms(pengk_ctx* ctx, int n_motifs, const int32_t* d_best, const uint64_t* d_site,
                             const uint32_t* d_lens, uint64_t n_seq, const int32_t* h_len, const int32_t* h_thr,
                             uint32_t max_gap, uint32_t min_len, uint32_t max_len, uint64_t* d_hist_gaps,
                             uint64_t* d_hist_lengths, uint64_t* d_hist_motifs) {
  if (!ctx || n_motifs < 0 || (n_motifs && (!h_len || !h_thr || !d_hist_motifs)) ||
      (n_motifs > 1 && (!d_hist_gaps || !d_hist_lengths)) || (n_seq && n_motifs && (!d_best || !d_site || !d_lens)))
    return fail(PENGK_ERR_ARG, "pengk_spacing_histograms: bad argument");
  if (n_motifs > PENGK_SPACING_MAX_MOTIFS)
    return fail(PENGK_ERR_ARG, "pengk_spacing_histograms: %d motifs (at most %d)", n_motifs, PENGK_SPACING_MAX_MOTIFS);
  if (max_gap > PENGK_SPACING_MAX_GAP)
    return fail(PENGK_ERR_ARG, "pengk_spacing_histograms: max_gap %u (at most %d)", max_gap, PENGK_SPACING_MAX_GAP);
  if (max_len < 1 || max_len > PENGK_CENTRALITY_MAX_LEN)
    return fail(PENGK_ERR_ARG, "pengk_spacing_histograms: max_len %u (1..%d)", max_len, PENGK_CENTRALITY_MAX_LEN);
  for (int m = 0; m < n_motifs; ++m) {
    if (h_len[m] < 1 || h_len[m] > PENGK_MAX_MOTIF_LEN)
      return fail(PENGK_ERR_ARG, "pengk_spacing_histograms: motif %d has width %d (1..%d)", m, h_len[m], PENGK_MAX_MOTIF_LEN);
    if (min_len < (uint32_t)h_len[m])
      return fail(PENGK_ERR_ARG, "pengk_spacing_histograms: min_len %u below the width %d of motif %d", min_len, h_len[m], m);
  }
  SCORE_ENTER(ctx);
  if (n_seq == 0 || n_motifs == 0) return PENGK_OK;
  // LDS bins when a pair's bins fit and the input is large enough for a block to add to a bin more than once; a motif
  // with more earlier motifs than fit gets several rows.  Else one row per motif, global bins.
  const uint64_t per = 4ull * (max_gap + 1) + 2 + (uint64_t)max_len + 1;
  const bool lds = per <= (uint64_t)SPACE_LDS_BINS && n_seq >= (uint64_t)SPACE_THREADS * 16;
  const int fit = lds ? (int)((uint64_t)SPACE_LDS_BINS / per) : PENGK_SPACING_MAX_MOTIFS;
  std::vector<SpaceRow> rows;
  for (int b = 0; b < n_motifs; ++b)
    for (int a0 = 0; a0 == 0 || a0 < b; a0 += fit) rows.push_back(SpaceRow{b, a0, std::min(b, a0 + fit), 0});
  const size_t wb = 2 * (size_t)n_motifs * sizeof(int32_t);  // (a multiple of 8: the rows are 16 bytes each)
  std::vector<char> staged(wb + rows.size() * sizeof(SpaceRow));
  int32_t* wt = (int32_t*)staged.data();
  for (int m = 0; m < n_motifs; ++m) {
    wt[2 * m] = h_len[m];
    wt[2 * m + 1] = h_thr[m];
  }
  memcpy(staged.data() + wb, rows.data(), rows.size() * sizeof(SpaceRow));
  int rc = ensure_scratch(ctx, &ctx->d_misc, &ctx->misc_bytes, staged.size());
  if (rc) return rc;
  PENGK_HIP(hipStreamSynchronize(ctx->stream));
  PENGK_HIP(hipMemcpy(ctx->d_misc, staged.data(), staged.size(), hipMemcpyHostToDevice));
  // blocks per row: four per CU over all rows, and enough that no block's uint32 bin can wrap
  const uint64_t blocks = (n_seq + SPACE_THREADS - 1) / SPACE_THREADS;
  const uint64_t per_row = std::max<uint64_t>(std::min<uint64_t>(blocks, (uint64_t)ctx->num_cu * 4 / rows.size() + 1), (n_seq >> 31) + 1);
  const dim3 grid((unsigned)per_row, (unsigned)rows.size());
  const int32_t* d_wt = (const int32_t*)ctx->d_misc;
  const SpaceRow* d_rows = (const SpaceRow*)((const char*)ctx->d_misc + wb);
  const unsigned long long* site = (const unsigned long long*)d_site;
  unsigned long long* hg = (unsigned long long*)d_hist_gaps;
  unsigned long long* hl = (unsigned long long*)d_hist_lengths;
  unsigned long long* hm = (unsigned long long*)d_hist_motifs;
  if (lds)
    hipLaunchKernelGGL(spacing_hist_kernel<true>, grid, dim3(SPACE_THREADS), 0, ctx->stream, d_best, site, d_lens, n_seq, d_wt,
                       d_rows, max_gap, min_len, max_len, hg, hl, hm);
  else
    hipLaunchKernelGGL(spacing_hist_kernel<false>, grid, dim3(SPACE_THREADS), 0, ctx->stream, d_best, site, d_lens, n_seq, d_wt,
                       d_rows, max_gap, min_len, max_len, hg, hl, hm);
  PENGK_HIP(hipGetLastError());
  return PENGK_OK;
}

int pengk_spacing_summary(const uint64_t* h_gaps, const uint64_t* h_lengths, uint32_t max_gap, uint32_t max_len, int w_a,
                          int w_b, int n_classes, uint64_t n, uint64_t n_a, uint64_t n_b, int n_pairs, pengk_spacing* out) {
  if (!h_gaps || !h_lengths || !out || max_gap > PENGK_SPACING_MAX_GAP || max_len < 1 || max_len > PENGK_CENTRALITY_MAX_LEN ||
      w_a < 1 || w_a > PENGK_MAX_MOTIF_LEN || w_b < 1 || w_b > PENGK_MAX_MOTIF_LEN || (n_classes != 2 && n_classes != 4) ||
      n_a > n || n_b > n || n_pairs < 1)
    return fail(PENGK_ERR_ARG, "pengk_spacing_summary: bad argument");
  memset(out, 0, sizeof *out);
  const uint32_t G1 = max_gap + 1;
  uint64_t near = 0;
  for (uint32_t k = 0; k < 4 * G1; ++k) {
    if (h_gaps[k] && (int)(k / G1) >= n_classes)
      return fail(PENGK_ERR_ARG, "pengk_spacing_summary: a count in orientation %u of %d", k / G1, n_classes);
    near += h_gaps[k];
  }
  out->overlapping = h_gaps[4 * G1];
  out->far = h_gaps[4 * G1 + 1];
  out->apart = near + out->far;
  out->both = out->overlapping + out->apart;
  if (out->both > n_a || out->both > n_b) return fail(PENGK_ERR_ARG, "pengk_spacing_summary: more pairs than sites of a motif");
  // the apart sequences' lengths, ascending
  const int64_t ws = (int64_t)w_a + w_b;
  std::vector<uint32_t> Ls;
  uint64_t nl = 0;
  for (uint32_t L = 0; L <= max_len; ++L) {
    if (!h_lengths[L]) continue;
    if ((int64_t)L < ws) return fail(PENGK_ERR_ARG, "pengk_spacing_summary: two sites apart on a sequence shorter than both motifs");
    nl += h_lengths[L];
    Ls.push_back(L);
  }
  if (nl != out->apart) return fail(PENGK_ERR_ARG, "pengk_spacing_summary: the histograms hold different totals");
  if (n) {
    const double p_co = ((double)n_a / (double)n) * ((double)n_b / (double)n);
    out->expected_both = (double)n * p_co;
    out->log10_pvalue_both = log10_binomial_sf(n, out->both, p_co);
  }
  const uint64_t Na = out->apart;
  if (Na == 0) return PENGK_OK;
  std::vector<double> pg(G1, 0.0);
  for (uint32_t g = 0; g <= max_gap; ++g) {
    double s = 0.0;
    for (const uint32_t L : Ls) {
      const int64_t T = (int64_t)L - ws + 1, k = T - (int64_t)g;
      if (k > 0) s += (double)h_lengths[L] * (double)k / ((double)n_classes * (double)(T * (T + 1) / 2));
    }
    pg[g] = s / (double)Na;
    if (pg[g] > 0.0) {
      ++out->tested_gaps;
      continue;
    }
    for (int c = 0; c < n_classes; ++c)
      if (h_gaps[(uint32_t)c * G1 + g]) return fail(PENGK_ERR_ARG, "pengk_spacing_summary: gap %u on sequences too short for it", g);
  }
  bool have = false;
  for (int c = 0; c < n_classes; ++c)
    for (uint32_t g = 0; g <= max_gap; ++g) {
      if (!(pg[g] > 0.0)) continue;
      const uint64_t H = h_gaps[(uint32_t)c * G1 + g];
      const double lp = log10_binomial_sf(Na, H, std::min(1.0, pg[g]));
      if (!have || lp < out->log10_pvalue) {
        have = true;
        out->orientation = (uint32_t)c;
        out->gap = g;
        out->count = H;
        out->expected = (double)Na * pg[g];
        out->log10_pvalue = lp;
      }
    }
  out->log10_evalue =
      out->log10_pvalue + std::log10((double)n_classes * (double)out->tested_gaps) + std::log10((double)n_pairs);
  return PENGK_OK;
}

// pengk_site_profiles and (pairs) pengk_site_pair_profiles: the same arguments, checks, clamp and grid
static int site_profiles(const char* who, bool pairs, pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid,
                         const int64_t* d_offs, const uint32_t* d_lens, uint64_t n_seq, int n_motifs, const int32_t* d_best,
                         const uint64_t* d_site, const int32_t* h_len, const int32_t* h_thr, int flank, uint64_t* d_counts) {
  if (!ctx || n_motifs < 0 || flank < 0 || (n_motifs && (!h_len || !h_thr || !d_counts)) ||
      (n_seq && n_motifs && (!d_words || !d_offs || !d_lens || !d_best || !d_site)))
    return fail(PENGK_ERR_ARG, "%s: bad argument", who);
  for (int m = 0; m < n_motifs; ++m)
    if (h_len[m] < 1 || h_len[m] > PENGK_MAX_MOTIF_LEN)
      return fail(PENGK_ERR_ARG, "%s: motif %d has width %d (1..%d)", who, m, h_len[m], PENGK_MAX_MOTIF_LEN);
  SCORE_ENTER(ctx);
  if (n_seq == 0 || n_motifs == 0) return PENGK_OK;
  std::vector<int32_t> wtf(3 * (size_t)n_motifs);
  for (int m = 0; m < n_motifs; ++m) {
    wtf[3 * m] = h_len[m];
    wtf[3 * m + 1] = h_thr[m];
    wtf[3 * m + 2] = std::min(flank, (PENGK_MAX_MOTIF_LEN - h_len[m]) / 2);
  }
  int rc = ensure_scratch(ctx, &ctx->d_misc, &ctx->misc_bytes, wtf.size() * sizeof(int32_t));
  if (rc) return rc;
  PENGK_HIP(hipStreamSynchronize(ctx->stream));
  PENGK_HIP(hipMemcpy(ctx->d_misc, wtf.data(), wtf.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  // blocks per motif: enough to fill the device, and so many that a block's 32-bit LDS bins cannot wrap (< 2^31 each)
  const uint64_t need = (n_seq + PROF_THREADS - 1) / PROF_THREADS;
  const uint64_t fill = (uint64_t)ctx->num_cu * 8 / (uint64_t)n_motifs + 1;
  const uint64_t per_motif = std::max<uint64_t>(std::min(need, fill), (n_seq >> 31) + 1);
  const dim3 grid((unsigned)per_motif, (unsigned)n_motifs);
  hipLaunchKernelGGL(pairs ? site_pair_profile_kernel : site_profile_kernel, grid, dim3(PROF_THREADS), 0, ctx->stream, d_words,
                     d_valid, d_offs, d_lens, n_seq, d_best, (const unsigned long long*)d_site, (const int32_t*)ctx->d_misc,
                     (unsigned long long*)d_counts);
  PENGK_HIP(hipGetLastError());
  return PENGK_OK;
}

int pengk_site_profiles(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                        const uint32_t* d_lens, uint64_t n_seq, int n_motifs, const int32_t* d_best, const uint64_t* d_site,
                        const int32_t* h_len, const int32_t* h_thr, int flank, uint64_t* d_counts) {
  return site_profiles("pengk_site_profiles", false, ctx, d_words, d_valid, d_offs, d_lens, n_seq, n_motifs, d_best, d_site, h_len,
                       h_thr, flank, d_counts);
}

int pengk_profile_refine(const uint64_t* h_counts, int w, int flank, const float* h_bg, double min_ic, double* h_q,
                         double* h_ic, float* h_pwm, int32_t* first_out, int32_t* last_out, uint64_t* sites_out) {
  if (!h_counts || !h_bg || !first_out || !last_out || w < 1 || w > PENGK_MAX_MOTIF_LEN || flank < 0 || !(min_ic == min_ic))
    return fail(PENGK_ERR_ARG, "pengk_profile_refine: bad argument");
  for (int b = 0; b < 4; ++b)
    if (!(h_bg[b] > 0.0f)) return fail(PENGK_ERR_ARG, "pengk_profile_refine: background frequency %d is not positive", b);
  const int F = std::min(flank, (PENGK_MAX_MOTIF_LEN - w) / 2), C = w + 2 * F;
  int first = C, last = 0;  // [first, last): empty
  for (int c = 0; c < C; ++c) {
    const uint64_t* k = h_counts + (size_t)c * 5;
    const uint64_t n = ((k[0] + k[1]) + k[2]) + k[3];
    double ic = 0.0;
    for (int b = 0; b < 4; ++b) {
      const double g = (double)h_bg[b];
      const double q = ((double)k[b] + g) / ((double)n + 1.0);
      ic += q * std::log2(q / g);
      if (h_q) h_q[(size_t)c * 4 + b] = q;
    }
    if (h_ic) h_ic[c] = ic;
    if (ic >= min_ic) {
      if (first == C) first = c;
      last = c + 1;
    }
  }
  if (first == C) first = 0;
  if (h_pwm)
    for (int c = first; c < last; ++c) {
      const uint64_t* k = h_counts + (size_t)c * 5;
      const uint64_t n = ((k[0] + k[1]) + k[2]) + k[3];
      for (int b = 0; b < 4; ++b)
        h_pwm[(size_t)(c - first) * 4 + b] = (float)(((double)k[b] + (double)h_bg[b]) / ((double)n + 1.0));
    }
  *first_out = first;
  *last_out = last;
  if (sites_out) {  // every site adds 1 to one bin of every column: the first motif column's total
    const uint64_t* k = h_counts + (size_t)F * 5;
    *sites_out = k[0] + k[1] + k[2] + k[3] + k[4];
  }
  return PENGK_OK;
}

int pengk_site_pair_profiles(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                             const uint32_t* d_lens, uint64_t n_seq, int n_motifs, const int32_t* d_best, const uint64_t* d_site,
                             const int32_t* h_len, const int32_t* h_thr, int flank, uint64_t* d_counts) {
  return site_profiles("pengk_site_pair_profiles", true, ctx, d_words, d_valid, d_offs, d_lens, n_seq, n_motifs, d_best, d_site,
                       h_len, h_thr, flank, d_counts);
}

int pengk_dinuc_model(const uint64_t* h_counts1, const uint64_t* h_counts2, int w, int flank, const float* h_bg0,
                      const float* h_bg1, double alpha, double* h_q0, double* h_q1, double* h_mi, int32_t* h_S0, int32_t* h_D1,
                      int32_t* h_D0, uint64_t* sites_out) {
  if (!h_counts1 || !h_counts2 || !h_bg0 || !h_bg1 || w < 1 || w > PENGK_MAX_MOTIF_LEN || flank < 0 || !(alpha > 0.0) ||
      !(alpha <= 1.7976931348623157e308))
    return fail(PENGK_ERR_ARG, "pengk_dinuc_model: bad argument");
  for (int b = 0; b < 4; ++b)
    if (!(h_bg0[b] > 0.0f)) return fail(PENGK_ERR_ARG, "pengk_dinuc_model: background frequency %d is not positive", b);
  for (int b = 0; b < 16; ++b)
    if (!(h_bg1[b] > 0.0f)) return fail(PENGK_ERR_ARG, "pengk_dinuc_model: background conditional %d is not positive", b);
  const int F = std::min(flank, (PENGK_MAX_MOTIF_LEN - w) / 2), C = w + 2 * F;
  double g0[4], g1[16];
  for (int b = 0; b < 4; ++b) g0[b] = (double)h_bg0[b];
  for (int b = 0; b < 16; ++b) g1[b] = (double)h_bg1[b];
  for (int c = 0; c < C; ++c) {
    const uint64_t* k1 = h_counts1 + (size_t)c * 5;
    const uint64_t* k2 = h_counts2 + (size_t)c * 17;
    const uint64_t n1 = ((k1[0] + k1[1]) + k1[2]) + k1[3];
    double q0[4];
    for (int b = 0; b < 4; ++b) q0[b] = ((double)k1[b] + g0[b]) / ((double)n1 + 1.0);
    if (h_q0)
      for (int b = 0; b < 4; ++b) h_q0[(size_t)c * 4 + b] = q0[b];
    if (c == 0 && h_S0)
      for (int b = 0; b < 4; ++b) h_S0[b] = dinuc_log_odds(q0[b], g0[b]);
    uint64_t row[4], col[4];
    for (int a = 0; a < 4; ++a) row[a] = ((k2[4 * a] + k2[4 * a + 1]) + k2[4 * a + 2]) + k2[4 * a + 3];
    for (int b = 0; b < 4; ++b) col[b] = ((k2[b] + k2[4 + b]) + k2[8 + b]) + k2[12 + b];
    for (int a = 0; a < 4; ++a)
      for (int b = 0; b < 4; ++b) {
        const int x = 4 * a + b;
        const double q1 = c == 0 ? q0[b] : ((double)k2[x] + alpha * q0[b]) / ((double)row[a] + alpha);
        if (h_q1) h_q1[(size_t)c * 16 + x] = q1;
        if (h_D1) h_D1[(size_t)c * 16 + x] = c == 0 ? 0 : dinuc_log_odds(q1, g1[x]);
        if (h_D0) h_D0[(size_t)c * 16 + x] = c == 0 ? 0 : dinuc_log_odds(q0[b], g1[x]);
      }
    if (h_mi) {
      double mi = 0.0;
      const uint64_t N = ((row[0] + row[1]) + row[2]) + row[3];
      if (c > 0 && N > 0)
        for (int a = 0; a < 4; ++a)
          for (int b = 0; b < 4; ++b) {
            const uint64_t k = k2[4 * a + b];
            if (k == 0) continue;
            const double num = (double)k * (double)N, den = (double)row[a] * (double)col[b];
            mi += ((double)k / (double)N) * std::log2(num / den);
          }
      h_mi[c] = mi;
    }
  }
  if (sites_out) {
    const uint64_t* k = h_counts1 + (size_t)F * 5;
    *sites_out = k[0] + k[1] + k[2] + k[3] + k[4];
  }
  return PENGK_OK;
}

int pengk_motif_scan_dinuc(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                           const uint32_t* d_lens, uint64_t n_seq, int n_motifs, const int32_t* h_S0, const int32_t* h_D,
                           const int32_t* h_len, int both_strands, int32_t* d_best) {
  if (!ctx || n_motifs < 0 || (n_motifs && (!h_S0 || !h_D || !h_len)) ||
      (n_seq && n_motifs && (!d_words || !d_offs || !d_lens || !d_best)))
    return fail(PENGK_ERR_ARG, "pengk_motif_scan_dinuc: bad argument");
  for (int m = 0; m < n_motifs; ++m) {
    if (h_len[m] < 1 || h_len[m] > PENGK_MAX_MOTIF_LEN)
      return fail(PENGK_ERR_ARG, "pengk_motif_scan_dinuc: motif %d has width %d (1..%d)", m, h_len[m], PENGK_MAX_MOTIF_LEN);
    for (int j = 0; j < 4; ++j) {
      const int32_t v = h_S0[(size_t)m * 4 + j];
      if (v < -2000 || v > 2000) return fail(PENGK_ERR_ARG, "pengk_motif_scan_dinuc: motif %d: log-odds %d outside [-2000, 2000]", m, v);
    }
    for (int j = 16; j < h_len[m] * 16; ++j) {
      const int32_t v = h_D[(size_t)m * PENGK_MAX_MOTIF_LEN * 16 + j];
      if (v < -2000 || v > 2000) return fail(PENGK_ERR_ARG, "pengk_motif_scan_dinuc: motif %d: log-odds %d outside [-2000, 2000]", m, v);
    }
  }
  SCORE_ENTER(ctx);
  if (n_seq == 0 || n_motifs == 0) return PENGK_OK;
  StagedMotifs st;
  int rc = stage_motifs_dinuc(ctx, n_motifs, h_S0, h_D, h_len, both_strands ? 2 : 1, &st);
  if (rc) return rc;
  const dim3 grid(grid_for(ctx, n_seq, SCAN_THREADS, 8), (unsigned)st.n_groups);
  if (both_strands)
    hipLaunchKernelGGL(motif_scan_dinuc_kernel<true>, grid, dim3(SCAN_THREADS), 0, ctx->stream, d_words, d_valid, d_offs, d_lens,
                       n_seq, st.tables, st.recs, st.groups, d_best);
  else
    hipLaunchKernelGGL(motif_scan_dinuc_kernel<false>, grid, dim3(SCAN_THREADS), 0, ctx->stream, d_words, d_valid, d_offs, d_lens,
                       n_seq, st.tables, st.recs, st.groups, d_best);
  PENGK_HIP(hipGetLastError());
  return PENGK_OK;
}

}  // extern "C"
