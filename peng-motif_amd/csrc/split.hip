// split.hip -- a hold-out split of a scan layout's sequences on the device (--holdout), and the test a
// found motif gets on the share it was not fitted to.
//
//   split    the class of a sequence is one hash of its global index against a threshold; the two classes' offs / lens /
//            index leave compacted, in file order.  Three launches, none waits for another workgroup: the tiles' hold-out
//            counts, their exclusive sums (one workgroup), the compaction.  One wave takes 64 sequences at a time: the
//            class is a ballot, a lane's place the popcount below it.  The training places follow from the hold-out
//            ones: what stands before a sequence and is not held out is training.
//   summary  pure CPU: pengk_enrich_summary over the training histograms fixes the threshold, one Fisher tail over the
//            hold-out histograms at that threshold judges it.
// Integer throughout up to the summary: no float, no waiting between workgroups.
#include <string.h>

#include <cmath>

#include "pengk_internal.h"

namespace pengk {
namespace {

constexpr int SPLIT_THREADS = 256;
constexpr int SPLIT_WAVES = SPLIT_THREADS / 64;
constexpr int SPLIT_ROUNDS = 8;                            // elements per thread ...
constexpr int SPLIT_WAVE_SPAN = 64 * SPLIT_ROUNDS;         // ... a wave's consecutive elements ...
constexpr int SPLIT_TILE = SPLIT_THREADS * SPLIT_ROUNDS;   // ... and a workgroup's
constexpr int SPLIT_SCAN_PER = 8;

// Element e of tile b is sequence b * SPLIT_TILE + e; wave w of the workgroup owns elements [w * SPLIT_WAVE_SPAN,
// + SPLIT_WAVE_SPAN) and takes them 64 at a time, lane by lane: file order is (tile, wave, round, lane).
__device__ __forceinline__ uint64_t split_seq(uint32_t round) {
  return (uint64_t)blockIdx.x * SPLIT_TILE + (threadIdx.x >> 6) * SPLIT_WAVE_SPAN + round * 64u + (threadIdx.x & 63u);
}

// 1 (hold-out) or 0 (training) of sequence i < n
__device__ __forceinline__ bool split_class(uint64_t seed, uint64_t seq0, uint64_t threshold, const uint32_t* __restrict__ index,
                                            uint64_t i) {
  const uint64_t g = seq0 + (index ? (uint64_t)index[i] : i);
  return (mix64(seed + 0x9E3779B97F4A7C15ull * (g + 1ull)) >> 32) < threshold;
}

// tile_hold[b]: the hold-out sequences of tile b
__global__ __launch_bounds__(SPLIT_THREADS) void split_count_kernel(uint64_t seed, uint64_t seq0, uint64_t threshold,
                                                                    const uint32_t* __restrict__ index, uint64_t n,
                                                                    uint32_t* __restrict__ tile_hold) {
  __shared__ uint32_t wtot[SPLIT_WAVES];
  uint32_t run = 0;
  for (uint32_t r = 0; r < SPLIT_ROUNDS; ++r) {
    const uint64_t i = split_seq(r);
    run += (uint32_t)__popcll(__ballot(i < n && split_class(seed, seq0, threshold, index, i)));
  }
  if ((threadIdx.x & 63u) == 0) wtot[threadIdx.x >> 6] = run;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (int w = 0; w < SPLIT_WAVES; ++w) s += wtot[w];
    tile_hold[blockIdx.x] = s;
  }
}

// Exclusive sums in place of a[0 .. n) by one workgroup; *total receives the sum.  Every exclusive sum is below 2^32 (at
// most 2^32 sequences in all, the last tile's own not included); the total may be 2^32 itself and is kept in 64 bits.
__global__ __launch_bounds__(SPLIT_THREADS) void split_scan_kernel(uint32_t* __restrict__ a, uint64_t n,
                                                                   unsigned long long* __restrict__ total) {
  __shared__ uint32_t sh[SPLIT_THREADS];
  const int t = threadIdx.x;
  unsigned long long carry = 0;
  for (uint64_t b = 0; b < n; b += (uint64_t)SPLIT_THREADS * SPLIT_SCAN_PER) {
    uint32_t v[SPLIT_SCAN_PER], s = 0;
    const uint64_t k0 = b + (uint64_t)t * SPLIT_SCAN_PER;
    for (int r = 0; r < SPLIT_SCAN_PER; ++r) {
      v[r] = k0 + r < n ? a[k0 + r] : 0u;
      s += v[r];
    }
    sh[t] = s;  // (a round of the loop holds at most 2048 tiles of 2048: below 2^32)
    __syncthreads();
    for (int d = 1; d < SPLIT_THREADS; d <<= 1) {
      const uint32_t x = t >= d ? sh[t - d] : 0u;
      __syncthreads();
      sh[t] += x;
      __syncthreads();
    }
    unsigned long long e = carry + sh[t] - s;
    carry += sh[SPLIT_THREADS - 1];
    __syncthreads();
    for (int r = 0; r < SPLIT_SCAN_PER; ++r) {
      if (k0 + r < n) a[k0 + r] = (uint32_t)e;
      e += v[r];
    }
  }
  if (total && t == 0) *total = carry;
}

// both classes' offs / lens / index at their places.  A hold-out sequence: tile_hold (after its scan) + the held out
// before it in the tile.  A training sequence: the sequences before it, less the held out among them.
__global__ __launch_bounds__(SPLIT_THREADS) void split_write_kernel(
    uint64_t seed, uint64_t seq0, uint64_t threshold, const uint32_t* __restrict__ index, uint64_t n,
    const uint32_t* __restrict__ tile_hold, const int64_t* __restrict__ offs, const uint32_t* __restrict__ lens,
    uint8_t* __restrict__ cls, int64_t* __restrict__ offs0, uint32_t* __restrict__ lens0, uint32_t* __restrict__ index0,
    int64_t* __restrict__ offs1, uint32_t* __restrict__ lens1, uint32_t* __restrict__ index1) {
  __shared__ uint32_t wtot[SPLIT_WAVES];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const unsigned long long below = (1ull << lane) - 1ull;
  uint32_t pos[SPLIT_ROUNDS], run = 0;
  bool h[SPLIT_ROUNDS];
  for (uint32_t r = 0; r < SPLIT_ROUNDS; ++r) {
    const uint64_t i = split_seq(r);
    h[r] = i < n && split_class(seed, seq0, threshold, index, i);
    const unsigned long long m = __ballot(h[r]);
    pos[r] = run + (uint32_t)__popcll(m & below);  // the held out of this wave before the lane
    run += (uint32_t)__popcll(m);
  }
  if (lane == 0) wtot[wave] = run;
  __syncthreads();
  uint64_t base = tile_hold[blockIdx.x];
  for (uint32_t w = 0; w < wave; ++w) base += wtot[w];
  for (uint32_t r = 0; r < SPLIT_ROUNDS; ++r) {
    const uint64_t i = split_seq(r);
    if (i >= n) continue;
    const uint64_t before = base + pos[r];  // the held out among the sequences [0, i): <= i
    const int64_t o = offs[i];
    const uint32_t l = lens[i];
    if (h[r]) {
      offs1[before] = o;
      lens1[before] = l;
      index1[before] = (uint32_t)i;
    } else {
      const uint64_t at = i - before;  // (< n)
      offs0[at] = o;
      lens0[at] = l;
      index0[at] = (uint32_t)i;
    }
    if (cls) cls[i] = h[r] ? 1 : 0;
  }
}

// [a, a + na) and [b, b + nb) share a byte (either NULL: no)
bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  if (!a || !b || !na || !nb) return false;
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

}  // namespace
}  // namespace pengk

using namespace pengk;

extern "C" {

int pengk_split_sequences(pengk_ctx* ctx, uint64_t seed, uint64_t seq0, uint64_t n_seq, uint64_t threshold, const uint32_t* d_index,
                          const int64_t* d_offs, const uint32_t* d_lens, uint8_t* d_class, int64_t* d_offs0, uint32_t* d_lens0,
                          uint32_t* d_index0, uint64_t* n0_out, int64_t* d_offs1, uint32_t* d_lens1, uint32_t* d_index1,
                          uint64_t* n1_out) {
  if (!ctx || !n0_out || !n1_out ||
      (n_seq && (!d_offs || !d_lens || !d_offs0 || !d_lens0 || !d_index0 || !d_offs1 || !d_lens1 || !d_index1)))
    return fail(PENGK_ERR_ARG, "pengk_split_sequences: bad argument");
  const uint64_t lim = 1ull << 32;
  if (seq0 > lim || n_seq > lim - seq0)
    return fail(PENGK_ERR_ARG, "pengk_split_sequences: sequences beyond global index 2^32; shard the input");
  if (threshold > lim) return fail(PENGK_ERR_ARG, "pengk_split_sequences: threshold above 2^32");
  {
    const void* in[3] = {d_index, d_offs, d_lens};
    const size_t in_b[3] = {n_seq * sizeof(uint32_t), n_seq * sizeof(int64_t), n_seq * sizeof(uint32_t)};
    const void* out[7] = {d_class, d_offs0, d_lens0, d_index0, d_offs1, d_lens1, d_index1};
    const size_t out_b[7] = {n_seq, n_seq * sizeof(int64_t), n_seq * sizeof(uint32_t), n_seq * sizeof(uint32_t),
                             n_seq * sizeof(int64_t), n_seq * sizeof(uint32_t), n_seq * sizeof(uint32_t)};
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 7; ++b)
        if (overlap(in[a], in_b[a], out[b], out_b[b])) return fail(PENGK_ERR_ARG, "pengk_split_sequences: an output aliases an input");
  }
  int rc = enter(ctx);
  if (rc) return rc;
  *n0_out = 0;
  *n1_out = 0;
  if (n_seq == 0) return PENGK_OK;
  // scratch: the hold-out total (uint64) | hold-out counts by tile (uint32)
  const uint64_t n_tiles = (n_seq + SPLIT_TILE - 1) / SPLIT_TILE;
  rc = ensure_scratch(ctx, &ctx->d_sites, &ctx->sites_bytes, sizeof(uint64_t) + n_tiles * sizeof(uint32_t));
  if (rc) return rc;
  unsigned long long* d_total = (unsigned long long*)ctx->d_sites;
  uint32_t* d_hold = (uint32_t*)((char*)ctx->d_sites + sizeof(uint64_t));
  const dim3 tiles((unsigned)n_tiles), block(SPLIT_THREADS);
  hipLaunchKernelGGL(split_count_kernel, tiles, block, 0, ctx->stream, seed, seq0, threshold, d_index, n_seq, d_hold);
  hipLaunchKernelGGL(split_scan_kernel, dim3(1), block, 0, ctx->stream, d_hold, n_tiles, d_total);
  hipLaunchKernelGGL(split_write_kernel, tiles, block, 0, ctx->stream, seed, seq0, threshold, d_index, n_seq,
                     (const uint32_t*)d_hold, d_offs, d_lens, d_class, d_offs0, d_lens0, d_index0, d_offs1, d_lens1, d_index1);
  PENGK_HIP(hipGetLastError());
  unsigned long long total = 0;
  PENGK_HIP(hipMemcpyAsync(&total, d_total, sizeof total, hipMemcpyDeviceToHost, ctx->stream));
  PENGK_HIP(hipStreamSynchronize(ctx->stream));
  *n1_out = total;
  *n0_out = n_seq - total;
  return PENGK_OK;
}

int pengk_holdout_summary(const uint64_t* h_train_pos, const uint64_t* h_train_neg, const uint64_t* h_hold_pos,
                          const uint64_t* h_hold_neg, uint64_t nbins, int32_t thr, uint64_t n_train_pos, uint64_t n_train_neg,
                          uint64_t n_hold_pos, uint64_t n_hold_neg, pengk_holdout* out) {
  if (!out || (nbins && (!h_hold_pos || !h_hold_neg)) || n_hold_pos + n_hold_neg < n_hold_pos)
    return fail(PENGK_ERR_ARG, "pengk_holdout_summary: bad argument");
  pengk_enrichment tr;
  int rc = pengk_enrich_summary(h_train_pos, h_train_neg, nbins, thr, n_train_pos, n_train_neg, &tr);
  if (rc) return rc;
  uint64_t a = 0, b = 0;
  for (uint64_t k = 0; k < nbins; ++k) {
    if (h_hold_pos[k] > n_hold_pos - a || h_hold_neg[k] > n_hold_neg - b)
      return fail(PENGK_ERR_ARG, "pengk_holdout_summary: more hits than scored sequences");
    a += h_hold_pos[k];
    b += h_hold_neg[k];
  }
  memset(out, 0, sizeof *out);
  out->threshold = tr.threshold;
  out->n_thresholds = tr.n_thresholds;
  out->train_pos_hits = tr.pos_hits;
  out->train_neg_hits = tr.neg_hits;
  out->train_log10_adj_pvalue = tr.log10_adj_pvalue;
  a = b = 0;
  if (tr.n_thresholds) {  // (a tried threshold is a bin: thr <= threshold < thr + nbins)
    for (uint64_t k = (uint64_t)((int64_t)tr.threshold - (int64_t)thr); k < nbins; ++k) {
      a += h_hold_pos[k];
      b += h_hold_neg[k];
    }
    rc = pengk_hypergeom_log10_sf(n_hold_pos + n_hold_neg, a + b, n_hold_pos, a, &out->hold_log10_pvalue);
    if (rc) return rc;
  }
  out->hold_pos_hits = a;
  out->hold_neg_hits = b;
  out->hold_enrichment = (((double)a + 1.0) / ((double)n_hold_pos + 1.0)) / (((double)b + 1.0) / ((double)n_hold_neg + 1.0));
  return PENGK_OK;
}

}  // extern "C"
