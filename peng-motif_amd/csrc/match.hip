// match.hip -- a real control set matched to the input by GC content and length, on the device (--score-negatives control,
// DESIGN.md 22).
//
//   strata   one thread per sequence, like every scan kernel: the valid bases and the C / G among them by popcounts over
//            the sequence's words, the stratum (length bin x GC bin) stored per sequence and counted in an LDS histogram,
//            one global atomic per non-empty bin and workgroup.
//   select   the stable rank of every sequence within its stratum, in file order over all shards, decides whether it is
//            kept: ((r + 1) q) / c > (r q) / c keeps exactly q of c, evenly spaced.  Five launches, none waits for
//            another workgroup: the tiles' stratum counts, their exclusive sums over the tiles (one workgroup per
//            stratum), the keep flags and their tile sums, the exclusive sums of those (one workgroup), the compaction.
// Integer throughout: no float, no waiting between workgroups.
#include <string.h>

#include "pengk_internal.h"
#include "scan_walk.h"

namespace pengk {
namespace {

constexpr int MATCH_THREADS = 256;
constexpr int MATCH_STRATA = 256;                       // 16 length bins x up to 16 GC bins
constexpr int SEL_WAVES = MATCH_THREADS / 64;
constexpr int SEL_ROUNDS = 8;                           // elements per thread ...
constexpr int SEL_WAVE_SPAN = 64 * SEL_ROUNDS;          // ... a wave's consecutive elements ...
constexpr int SEL_TILE = MATCH_THREADS * SEL_ROUNDS;    // ... and a workgroup's: 10^7 sequences x 256 strata = 5 MB of counts
constexpr int PS_PER = 8;
static_assert(MATCH_THREADS == MATCH_STRATA, "one thread per stratum zeroes and flushes the LDS histograms");
enum { PAR_COUNT = 0, PAR_QUOTA = MATCH_STRATA, PAR_RANK0 = 2 * MATCH_STRATA, PAR_N = 3 * MATCH_STRATA };

// ---- pengk_seq_strata -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MATCH_THREADS) void seq_strata_kernel(const uint64_t* __restrict__ words,
                                                                   const uint32_t* __restrict__ valid,
                                                                   const int64_t* __restrict__ offs,
                                                                   const uint32_t* __restrict__ lens, uint64_t n_seq, uint32_t G,
                                                                   uint32_t use_length, uint16_t* __restrict__ stratum,
                                                                   unsigned long long* __restrict__ hist) {
  __shared__ uint32_t sh[MATCH_STRATA];
  sh[threadIdx.x] = 0;
  __syncthreads();
  for (uint64_t i = blockIdx.x * (uint64_t)MATCH_THREADS + threadIdx.x; i < n_seq; i += (uint64_t)gridDim.x * MATCH_THREADS) {
    const uint32_t L = lens[i];
    const uint32_t nw = (L >> 5) + ((L & 31u) ? 1u : 0u);
    const uint64_t w0 = (uint64_t)offs[i] >> 5;
    uint32_t gc = 0, n = valid ? 0u : L;
    for (uint32_t j = 0; j < nw; ++j) {
      const uint64_t w = words[w0 + j];
      gc += (uint32_t)__popcll((w ^ (w >> 1)) & 0x5555555555555555ull);  // (C = 1, G = 2: the two bits differ)
      if (valid) {
        const uint32_t rem = L - 32u * j;
        n += (uint32_t)__popc(valid[w0 + j] & (rem >= 32u ? 0xFFFFFFFFu : ((1u << rem) - 1u)));
      }
    }
    uint32_t s = 0xFFFFu;
    if (n) {
      const uint64_t q = ((uint64_t)gc * G) / n;
      const uint32_t g = q < G - 1u ? (uint32_t)q : G - 1u;
      uint32_t lb = 0;
      if (use_length) {
        const int l = 31 - __clz((int)L);  // (n > 0: L >= 1)
        const int h = 2 * l + (l ? (int)((L >> (l - 1)) & 1u) : 0) - 10;
        lb = (uint32_t)(h < 0 ? 0 : (h > 15 ? 15 : h));
      }
      s = lb * G + g;
      atomicAdd(&sh[s], 1u);
    }
    stratum[i] = (uint16_t)s;
  }
  __syncthreads();
  if (sh[threadIdx.x]) atomicAdd(&hist[threadIdx.x], (unsigned long long)sh[threadIdx.x]);
}

// ---- pengk_select_strata ----------------------------------------------------------------------------------------------
// Element e of tile b is sequence b * SEL_TILE + e; wave w of the workgroup owns elements [w * SEL_WAVE_SPAN, + SEL_WAVE_SPAN)
// and takes them 64 at a time, lane by lane: file order is (tile, wave, round, lane).
__device__ __forceinline__ uint64_t sel_seq(uint32_t round) {
  return (uint64_t)blockIdx.x * SEL_TILE + (threadIdx.x >> 6) * SEL_WAVE_SPAN + round * 64u + (threadIdx.x & 63u);
}

// counts[s * n_tiles + b]: the sequences of stratum s in tile b
__global__ __launch_bounds__(MATCH_THREADS) void sel_count_kernel(const uint16_t* __restrict__ stratum, uint64_t n,
                                                                  uint64_t n_tiles, uint32_t* __restrict__ counts) {
  __shared__ uint32_t sh[MATCH_STRATA];
  sh[threadIdx.x] = 0;
  __syncthreads();
  for (uint32_t r = 0; r < SEL_ROUNDS; ++r) {
    const uint64_t i = sel_seq(r);
    const uint32_t s = i < n ? stratum[i] : 0xFFFFu;
    if (s < MATCH_STRATA) atomicAdd(&sh[s], 1u);
  }
  __syncthreads();
  counts[(uint64_t)threadIdx.x * n_tiles + blockIdx.x] = sh[threadIdx.x];
}

// inclusive sum over the workgroup (sh: MATCH_THREADS entries; every thread calls it)
__device__ __forceinline__ uint32_t group_inclusive_sum(uint32_t v, uint32_t* sh, uint32_t* total) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int d = 1; d < MATCH_THREADS; d <<= 1) {
    const uint32_t x = t >= d ? sh[t - d] : 0u;
    __syncthreads();
    sh[t] += x;
    __syncthreads();
  }
  const uint32_t r = sh[t];
  *total = sh[MATCH_THREADS - 1];
  __syncthreads();
  return r;
}

// Exclusive sums in place of the rows of a (gridDim.x rows of n entries, one workgroup per row), each from first[row] on
// (NULL: from 0); total[row], where given, receives the row's sum without first[row].  All sums stay below 2^32.
__global__ __launch_bounds__(MATCH_THREADS) void sel_rowscan_kernel(uint32_t* __restrict__ a, uint64_t n,
                                                                    const unsigned long long* __restrict__ first,
                                                                    unsigned long long* __restrict__ total) {
  __shared__ uint32_t sh[MATCH_THREADS];
  uint32_t* p = a + (uint64_t)blockIdx.x * n;
  const uint32_t base = first ? (uint32_t)first[blockIdx.x] : 0u;
  uint32_t carry = 0;
  for (uint64_t b = 0; b < n; b += (uint64_t)MATCH_THREADS * PS_PER) {
    uint32_t v[PS_PER], s = 0;
    const uint64_t k0 = b + (uint64_t)threadIdx.x * PS_PER;
    for (int r = 0; r < PS_PER; ++r) {
      v[r] = k0 + r < n ? p[k0 + r] : 0u;
      s += v[r];
    }
    uint32_t t = 0;
    uint32_t e = base + carry + group_inclusive_sum(s, sh, &t) - s;
    for (int r = 0; r < PS_PER; ++r) {
      if (k0 + r < n) p[k0 + r] = e;
      e += v[r];
    }
    carry += t;
  }
  if (total && threadIdx.x == 0) total[blockIdx.x] = carry;
}

// keep[i] and the tiles' kept counts.  The rank of a sequence within its stratum: what the earlier ranks and tiles hold
// (counts, after the row scan), what the lower waves of this tile hold (wcnt, complete after the barrier) and what this
// wave has seen before it -- the wave's running count of the stratum, taken and advanced by the first lane of every group
// of equal strata of a round, plus the lanes of the group below this one.
__global__ __launch_bounds__(MATCH_THREADS) void sel_flag_kernel(const uint16_t* __restrict__ stratum, uint64_t n,
                                                                 uint64_t n_tiles, const uint32_t* __restrict__ counts,
                                                                 const unsigned long long* __restrict__ par,
                                                                 uint8_t* __restrict__ keep, uint32_t* __restrict__ tile_kept) {
  __shared__ uint32_t wcnt[SEL_WAVES][MATCH_STRATA];
  __shared__ uint32_t kept;
  for (int w = 0; w < SEL_WAVES; ++w) wcnt[w][threadIdx.x] = 0;
  if (threadIdx.x == 0) kept = 0;
  __syncthreads();
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const unsigned long long below = (1ull << lane) - 1ull;
  uint32_t st[SEL_ROUNDS], rk[SEL_ROUNDS];
  for (uint32_t r = 0; r < SEL_ROUNDS; ++r) {
    const uint64_t i = sel_seq(r);
    const uint32_t s = i < n ? stratum[i] : 0xFFFFu;
    const bool active = s < MATCH_STRATA;
    unsigned long long todo = __ballot(active), grp = 1ull << lane;
    while (todo) {  // (wave-uniform: one turn per distinct stratum among the 64)
      const uint32_t s0 = (uint32_t)__shfl((int)s, __builtin_ctzll(todo));
      const unsigned long long m = __ballot(active && s == s0);
      if (active && s == s0) grp = m;
      todo &= ~m;
    }
    const int lead = __builtin_ctzll(grp);
    uint32_t old = 0;
    if (active && (int)lane == lead) old = atomicAdd(&wcnt[wave][s], (uint32_t)__popcll(grp));
    old = (uint32_t)__shfl((int)old, lead);
    st[r] = s;
    rk[r] = old + (uint32_t)__popcll(grp & below);
  }
  __syncthreads();
  uint32_t mine = 0;
  for (uint32_t r = 0; r < SEL_ROUNDS; ++r) {
    const uint64_t i = sel_seq(r);
    if (i >= n) continue;
    const uint32_t s = st[r];
    uint8_t k = 0;
    if (s < MATCH_STRATA) {
      unsigned long long rank = (unsigned long long)counts[(uint64_t)s * n_tiles + blockIdx.x] + rk[r];
      for (uint32_t w = 0; w < wave; ++w) rank += wcnt[w][s];
      const unsigned long long q = par[PAR_QUOTA + s], c = par[PAR_COUNT + s];
      if (rank < c) k = ((rank + 1ull) * q) / c > (rank * q) / c ? 1 : 0;  // (rank < c < 2^32, q <= c: no overflow)
    }
    keep[i] = k;
    mine += k;
  }
  if (mine) atomicAdd(&kept, mine);
  __syncthreads();
  if (threadIdx.x == 0) tile_kept[blockIdx.x] = kept;
}

// the kept sequences' offs / lens / index at their places: tile_kept (after its row scan) + the kept before it in the tile
__global__ __launch_bounds__(MATCH_THREADS) void sel_write_kernel(const uint8_t* __restrict__ keep, uint64_t n,
                                                                  const uint32_t* __restrict__ tile_kept,
                                                                  const int64_t* __restrict__ offs, const uint32_t* __restrict__ lens,
                                                                  int64_t* __restrict__ sel_offs, uint32_t* __restrict__ sel_lens,
                                                                  uint32_t* __restrict__ sel_index) {
  __shared__ uint32_t wtot[SEL_WAVES];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const unsigned long long below = (1ull << lane) - 1ull;
  uint32_t pos[SEL_ROUNDS], run = 0;
  bool k[SEL_ROUNDS];
  for (uint32_t r = 0; r < SEL_ROUNDS; ++r) {
    const uint64_t i = sel_seq(r);
    k[r] = i < n && keep[i];
    const unsigned long long m = __ballot(k[r]);
    pos[r] = run + (uint32_t)__popcll(m & below);
    run += (uint32_t)__popcll(m);
  }
  if (lane == 0) wtot[wave] = run;
  __syncthreads();
  uint64_t base = tile_kept[blockIdx.x];
  for (uint32_t w = 0; w < wave; ++w) base += wtot[w];
  for (uint32_t r = 0; r < SEL_ROUNDS; ++r) {
    if (!k[r]) continue;
    const uint64_t i = sel_seq(r), o = base + pos[r];  // (o < the kept of this call <= n)
    sel_offs[o] = offs[i];
    sel_lens[o] = lens[i];
    sel_index[o] = (uint32_t)i;
  }
}

}  // namespace
}  // namespace pengk

using namespace pengk;

extern "C" {

int pengk_seq_strata(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                     const uint32_t* d_lens, uint64_t n_seq, int gc_bins, int use_length, uint16_t* d_stratum, uint64_t* d_hist) {
  if (!ctx || (n_seq && (!d_words || !d_offs || !d_lens || !d_stratum || !d_hist)))
    return fail(PENGK_ERR_ARG, "pengk_seq_strata: bad argument");
  if (gc_bins < 1 || gc_bins > 16) return fail(PENGK_ERR_ARG, "pengk_seq_strata: gc_bins %d out of range [1,16]", gc_bins);
  if (use_length != 0 && use_length != 1) return fail(PENGK_ERR_ARG, "pengk_seq_strata: use_length must be 0 or 1");
  if (n_seq >= (1ull << 32)) return fail(PENGK_ERR_ARG, "pengk_seq_strata: 2^32 sequences or more; shard the input");
  int rc = enter(ctx);
  if (rc) return rc;
  if (n_seq == 0) return PENGK_OK;
  hipLaunchKernelGGL(seq_strata_kernel, dim3(grid_for(ctx, n_seq, MATCH_THREADS, 16)), dim3(MATCH_THREADS), 0, ctx->stream, d_words,
                     d_valid, d_offs, d_lens, n_seq, (uint32_t)gc_bins, (uint32_t)use_length, d_stratum,
                     (unsigned long long*)d_hist);
  PENGK_HIP(hipGetLastError());
  return PENGK_OK;
}

int pengk_match_quotas(const uint64_t* h_in, const uint64_t* h_ctrl, uint64_t ratio, uint64_t* h_quota, uint64_t* shortfall_out) {
  if (!h_in || !h_ctrl || !h_quota || !shortfall_out || ratio < 1) return fail(PENGK_ERR_ARG, "pengk_match_quotas: bad argument");
  const uint64_t lim = 1ull << 63;
  uint64_t shortfall = 0;
  for (int s = 0; s < MATCH_STRATA; ++s) {
    if (h_in[s] && ratio > lim / h_in[s]) return fail(PENGK_ERR_RANGE, "pengk_match_quotas: ratio x input count exceeds 2^63");
    const uint64_t want = ratio * h_in[s];
    h_quota[s] = h_ctrl[s] < want ? h_ctrl[s] : want;
    if (want - h_quota[s] > lim - shortfall) return fail(PENGK_ERR_RANGE, "pengk_match_quotas: the shortfall exceeds 2^63");
    shortfall += want - h_quota[s];
  }
  *shortfall_out = shortfall;
  return PENGK_OK;
}

int pengk_select_strata(pengk_ctx* ctx, const uint16_t* d_stratum, uint64_t n_seq, const uint64_t* h_count, const uint64_t* h_quota,
                        const uint64_t* h_rank0, const int64_t* d_offs, const uint32_t* d_lens, int64_t* d_sel_offs,
                        uint32_t* d_sel_lens, uint32_t* d_sel_index, uint64_t* n_sel_out) {
  if (!ctx || !h_count || !h_quota || !h_rank0 || !n_sel_out ||
      (n_seq && (!d_stratum || !d_offs || !d_lens || !d_sel_offs || !d_sel_lens || !d_sel_index)))
    return fail(PENGK_ERR_ARG, "pengk_select_strata: bad argument");
  *n_sel_out = 0;
  if (n_seq >= (1ull << 32)) return fail(PENGK_ERR_ARG, "pengk_select_strata: 2^32 sequences or more; shard the control");
  unsigned long long par[PAR_N];
  for (int s = 0; s < MATCH_STRATA; ++s) {
    if (h_quota[s] > h_count[s]) return fail(PENGK_ERR_ARG, "pengk_select_strata: quota of stratum %d above its count", s);
    if (h_count[s] >= (1ull << 32) || h_rank0[s] > h_count[s])
      return fail(PENGK_ERR_ARG, "pengk_select_strata: count or first rank of stratum %d out of range", s);
    par[PAR_COUNT + s] = h_count[s];
    par[PAR_QUOTA + s] = h_quota[s];
    par[PAR_RANK0 + s] = h_rank0[s];
  }
  int rc = enter(ctx);
  if (rc) return rc;
  if (n_seq == 0) return PENGK_OK;
  // scratch: parameters and the kept total (uint64) | stratum counts by tile, kept counts by tile (uint32) | keep flags
  const uint64_t n_tiles = (n_seq + SEL_TILE - 1) / SEL_TILE;
  const size_t head = (PAR_N + 1) * sizeof(uint64_t), table = (MATCH_STRATA + 1) * n_tiles * sizeof(uint32_t);
  rc = ensure_scratch(ctx, &ctx->d_sites, &ctx->sites_bytes, head + table + n_seq);
  if (rc) return rc;
  unsigned long long* d_par = (unsigned long long*)ctx->d_sites;
  unsigned long long* d_total = d_par + PAR_N;
  uint32_t* d_counts = (uint32_t*)((char*)ctx->d_sites + head);
  uint32_t* d_kept = d_counts + MATCH_STRATA * n_tiles;
  uint8_t* d_keep = (uint8_t*)ctx->d_sites + head + table;
  // (synchronous, like the motif staging of score.hip: the scratch may still be read by an earlier call on the stream)
  PENGK_HIP(hipStreamSynchronize(ctx->stream));
  PENGK_HIP(hipMemcpy(d_par, par, sizeof par, hipMemcpyHostToDevice));
  const dim3 tiles((unsigned)n_tiles), block(MATCH_THREADS);
  hipLaunchKernelGGL(sel_count_kernel, tiles, block, 0, ctx->stream, d_stratum, n_seq, n_tiles, d_counts);
  hipLaunchKernelGGL(sel_rowscan_kernel, dim3(MATCH_STRATA), block, 0, ctx->stream, d_counts, n_tiles,
                     (const unsigned long long*)(d_par + PAR_RANK0), (unsigned long long*)nullptr);
  hipLaunchKernelGGL(sel_flag_kernel, tiles, block, 0, ctx->stream, d_stratum, n_seq, n_tiles, (const uint32_t*)d_counts,
                     (const unsigned long long*)d_par, d_keep, d_kept);
  hipLaunchKernelGGL(sel_rowscan_kernel, dim3(1), block, 0, ctx->stream, d_kept, n_tiles, (const unsigned long long*)nullptr, d_total);
  hipLaunchKernelGGL(sel_write_kernel, tiles, block, 0, ctx->stream, (const uint8_t*)d_keep, n_seq, (const uint32_t*)d_kept, d_offs,
                     d_lens, d_sel_offs, d_sel_lens, d_sel_index);
  PENGK_HIP(hipGetLastError());
  unsigned long long total = 0;
  PENGK_HIP(hipMemcpyAsync(&total, d_total, sizeof total, hipMemcpyDeviceToHost, ctx->stream));
  PENGK_HIP(hipStreamSynchronize(ctx->stream));
  *n_sel_out = total;
  return PENGK_OK;
}

}  // extern "C"
