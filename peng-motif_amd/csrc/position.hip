// position.hip -- k-mers with a position bias counted on the device (--positional): the table defined in
// include/pengk.h ("positional words").
//
//   tile     64 consecutive positions of one sequence, one wave, one position per lane.  A lane reads the window of
//            tile_walk.h with K-1 bases behind it (its own word and the K-1 <= 6 words that may stand before it lie in
//            the first 2K-1 <= 13 of its 16 bases) and the validity bits from the window's start on; st = v & v>>1 & .. & v>>(K-1) says for every base of the window whether a word stands there.  Standing,
//            clump head, coordinate and bin are decided in registers, in 32-bit arithmetic throughout.
//   clumps   two words have the same key iff the code of one is the code of the other or, on both strands, its reverse
//            complement: no predecessor is folded, each is compared with the lane's code and its reverse complement.
//   groups   the position bins in groups of at most 2^15 / 4^K (64 at most); a workgroup owns one group (blockIdx.y) and
//            keeps its tables in LDS, 4^K uint32 bins a position bin: 128 KiB at most.  Bins are bumped with non-returning
//            LDS adds.  Inside a workgroup a word is its code as the words hold it (first base lowest), on both strands
//            the smaller of the code and its reverse complement; the flush turns a bin's code into the public key (first
//            base highest), folds it again in that order and adds the bin to the uint64 table with a plain vector atomic;
//            empty bins add nothing, so no entry that is not canonical is ever written.
//   tiles    only the tiles of a sequence that hold a position whose coordinate lies under bin_size * n_bins are walked:
//            one contiguous range of them under every anchor (a superset is taken: the lane decides).  Their counts per
//            sequence -> exclusive sums, then every wave of a fixed grid walks one contiguous share of the tiles: the
//            plan, the share and the cursor of tile_walk.h.  Every wave of the grid runs the same number of rounds, so
//            the barriers of the flush sit in workgroup-uniform control flow.  A tile none of whose positions can fall into
//            the workgroup's bins is left before anything is loaded (one range of a sequence under start and end, two
//            under centre).
//   wrap     a position bumps at most one bin of a workgroup once, a round holds at most 1024 positions, and the tables are
//            flushed every POS_FLUSH_ROUNDS = 2^21 rounds: no bin exceeds 2^31 between two flushes.
// Nothing of size positions x bins is written to HBM.
#include <algorithm>
#include <cmath>
#include <vector>

#include "pengk_internal.h"
#include "tile_walk.h"

namespace pengk {
namespace {

constexpr int POS_THREADS = 1024;
constexpr int POS_WAVES = POS_THREADS / 64;
constexpr int POS_LDS_BINS = 1 << 15;            // uint32 bins a workgroup holds at most: 128 KiB
constexpr uint32_t POS_FLUSH_ROUNDS = 1u << 21;  // x 1024 positions a round = 2^31 per bin at most
static_assert(POS_LDS_BINS * 4 <= 160 * 1024, "a group's tables fit in LDS");
static_assert(2 * PENGK_POSITION_MAX_K - 1 <= 16, "a position's words lie in one window of 16 bases");
static_assert((uint64_t)PENGK_POSITION_MAX_BIN_SIZE * PENGK_POSITION_MAX_BINS <= (1ull << 22), "the coordinates under test fit 32 bits");

__host__ __device__ constexpr int pos_max_per_group(int K) {
  return (POS_LDS_BINS >> (2 * K)) < PENGK_POSITION_MAX_BINS ? (POS_LDS_BINS >> (2 * K)) : PENGK_POSITION_MAX_BINS;
}

// the tiles of a sequence of L bases that may hold a position with a coordinate below R: nt of them from tile k0 on
struct PosTiles {
  uint32_t k0, nt;
};
__host__ __device__ __forceinline__ PosTiles pos_tiles(uint32_t L, int K, int anchor, uint32_t R) {
  PosTiles t = {0u, 0u};
  if (L < (uint32_t)K) return t;
  const int64_t D = (int64_t)L - K;  // the last position
  int64_t lo = 0, hi = D;
  if (anchor == 0) {
    hi = D < (int64_t)R - 1 ? D : (int64_t)R - 1;
  } else if (anchor == 1) {
    lo = D - ((int64_t)R - 1) > 0 ? D - ((int64_t)R - 1) : 0;
  } else {  // |2p - D| < 2R: (D - 2R) / 2 < p < (D + 2R) / 2, rounded outwards
    const int64_t a = (D - 2 * (int64_t)R) >> 1, b = (D + 2 * (int64_t)R + 1) >> 1;
    lo = a > 0 ? a : 0;
    hi = b < D ? b : D;
  }
  t.k0 = (uint32_t)(lo >> 6);
  t.nt = (uint32_t)(hi >> 6) - t.k0 + 1u;
  return t;
}

struct PosTilesOf {
  int K, anchor;
  uint32_t R;
  __device__ __forceinline__ PosTiles operator()(uint32_t L) const { return pos_tiles(L, K, anchor, R); }
};

// ---- the count ----------------------------------------------------------------------------------------------------------
// the coordinate of position p <= D in a sequence whose last position is D.  32 bits throughout: with h = D >> 1 and
// r = D & 1, |2p - D| >> 1 is h - p up to h and p - h - r behind it, and 2p is never formed
__device__ __forceinline__ uint32_t pos_coordinate(int anchor, uint32_t p, uint32_t D) {
  if (anchor == 0) return p;
  if (anchor == 1) return D - p;
  const uint32_t h = D >> 1, r = D & 1u;
  return p > h ? p - h - r : h - p;
}

// One tile: the positions [64 k, 64 k + 64) of a sequence of L >= K bases whose words / validity words begin at wp / vp (vp
// NULL: every base valid), under the coordinates [c0, c1) of this workgroup's bins; bins: its tables.
template <int K, bool BOTH>
__device__ __forceinline__ void pos_tile(const uint64_t* __restrict__ wp, const uint32_t* __restrict__ vp, uint32_t L, uint32_t k,
                                         int anchor, uint32_t S, uint32_t c0, uint32_t c1, uint32_t* bins) {
  constexpr uint32_t MASK = (1u << (2 * K)) - 1u;
  const uint32_t D = L - (uint32_t)K;  // the last position
  {  // (wave-uniform) can a position of the tile fall into [c0, c1)?  The coordinate is monotone on either side of the centre
    const uint32_t P0 = k << 6;  // (k < 2^26)
    if (P0 > D) return;
    const uint32_t P1 = D - P0 < 63u ? D : P0 + 63u;
    const uint32_t a = pos_coordinate(anchor, P0, D), b = pos_coordinate(anchor, P1, D);
    const uint32_t most = a > b ? a : b;
    uint32_t least = a < b ? a : b;
    if (anchor == 2 && P0 <= (D >> 1) && (D >> 1) <= P1) least = 0u;
    if (least >= c1 || most < c0) return;
  }
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t p = (k << 6) + lane;  // (k < 2^26)
  // the window from q = max(p - (K-1), 0) on: the lane's word and the K-1 that may stand before it, 2K-1 <= 13 bases
  const tile::Window win = tile::window(wp, vp, L, p, (uint32_t)(K - 1));
  const uint32_t lo = win.lo, v = win.v, off = win.off;
  uint32_t st = v;  // bit i: a word stands at q + i
#pragma unroll
  for (int d = 1; d < K; ++d) st &= v >> d;
  const uint32_t code = (lo >> (2u * off)) & MASK;
  const uint32_t rc = BOTH ? revcomp32(code, K) : code;
  bool on = (st >> off) & 1u;
#pragma unroll
  for (int d = 1; d < K; ++d) {  // an equal word standing at p - d: not a clump head
    if ((uint32_t)d <= off) {
      const uint32_t i = off - (uint32_t)d;
      const uint32_t ci = (lo >> (2u * i)) & MASK;
      if (((st >> i) & 1u) && (ci == code || (BOTH && ci == rc))) on = false;
    }
  }
  const uint32_t c = pos_coordinate(anchor, p, D);  // (junk where p > D: no word stands there)
  if (on && c >= c0 && c < c1) {
    const uint32_t b = (c - c0) / S;
    atomicAdd(&bins[(b << (2 * K)) + (rc < code ? rc : code)], 1u);
  }
}

// the public key of a bin: the K digits of its code in reverse order (first base highest), folded on both strands
template <int K, bool BOTH>
__device__ __forceinline__ uint32_t pos_public_key(uint32_t code) {
  const uint32_t key = revcomp32(~code, K);
  if (!BOTH) return key;
  const uint32_t rc = revcomp32(key, K);
  return rc < key ? rc : key;
}

template <int K, bool BOTH>
__device__ __forceinline__ void pos_flush(uint32_t* bins, int b0, int nb, unsigned long long* __restrict__ counts) {
  constexpr int NK = 1 << (2 * K);
  __syncthreads();
  for (int q = threadIdx.x; q < nb * NK; q += POS_THREADS) {
    const uint32_t c = bins[q];
    if (c) {
      bins[q] = 0u;
      atomicAdd(&counts[(uint64_t)(b0 + q / NK) * NK + pos_public_key<K, BOTH>((uint32_t)q % NK)], (unsigned long long)c);
    }
  }
  __syncthreads();
}

template <int K, bool BOTH>
__global__ __launch_bounds__(POS_THREADS) void pos_count_kernel(const uint64_t* __restrict__ words, const uint32_t* __restrict__ valid,
                                                                const int64_t* __restrict__ offs, const uint32_t* __restrict__ lens,
                                                                uint64_t n_seq, int anchor, uint32_t S, int n_bins, int per_group,
                                                                const unsigned long long* __restrict__ excl,
                                                                const unsigned long long* __restrict__ boff, uint64_t n_groups,
                                                                unsigned long long* __restrict__ counts) {
  constexpr int NK = 1 << (2 * K);
  extern __shared__ __attribute__((aligned(16))) uint32_t sh[];  // (b1 - b0) tables
  const int b0 = (int)blockIdx.y * per_group, b1 = std::min(n_bins, b0 + per_group), nb = b1 - b0;
  const uint32_t c0 = (uint32_t)b0 * S, c1 = (uint32_t)b1 * S, R = (uint32_t)n_bins * S;
  // this wave's share of the tiles; `per` rounds for every wave of the grid
  const tile::Share share = tile::share<POS_WAVES>(boff, n_groups);
  if (share.block_empty) return;  // (the whole workgroup: nothing to zero, nothing to flush)
  for (int q = threadIdx.x; q < nb * NK; q += POS_THREADS) sh[q] = 0u;
  __syncthreads();
  uint64_t g = share.g;
  tile::Cursor<PosTilesOf> c{lens, n_seq, PosTilesOf{K, anchor, R}};
  if (g < share.gend) c.locate(g, excl, boff, n_groups);
  uint32_t since = 0;
  for (uint64_t round = 0; round < share.per; ++round) {  // (per, and so every barrier below, is the same for the whole grid)
    if (g < share.gend) {
      if (c.next()) {
        const uint64_t w0 = (uint64_t)offs[c.i] >> 5;
        pos_tile<K, BOTH>(words + w0, valid ? valid + w0 : nullptr, c.L, c.t.k0 + c.k, anchor, S, c0, c1, sh);
      }
      ++c.k;
      ++g;
    }
    if (++since == POS_FLUSH_ROUNDS) {
      pos_flush<K, BOTH>(sh, b0, nb, counts);
      since = 0;
    }
  }
  if (since) pos_flush<K, BOTH>(sh, b0, nb, counts);
}

template <int K, bool BOTH>
int pos_launch(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs, const uint32_t* d_lens,
               uint64_t n_seq, int anchor, uint32_t S, int n_bins, const unsigned long long* excl, const unsigned long long* boff,
               uint64_t n_groups, uint64_t* d_counts) {
  // the bins in equal groups of at most pos_max_per_group(K): 20 bins at K = 6 are 3 x 7
  const int bin_groups = (n_bins + pos_max_per_group(K) - 1) / pos_max_per_group(K);
  const int per_group = (n_bins + bin_groups - 1) / bin_groups;
  const size_t lds = ((size_t)per_group << (2 * K)) * sizeof(uint32_t);
  const unsigned per_cu = lds * 2 <= 160 * 1024 ? 2u : 1u;  // (32 waves a CU: two workgroups of 1024 threads at most)
  const dim3 grid((unsigned)ctx->num_cu * per_cu, (unsigned)bin_groups);
  PENGK_HIP(hipFuncSetAttribute((const void*)pos_count_kernel<K, BOTH>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((pos_count_kernel<K, BOTH>), grid, dim3(POS_THREADS), lds, ctx->stream, d_words, d_valid, d_offs, d_lens, n_seq,
                     anchor, S, n_bins, per_group, excl, boff, n_groups, (unsigned long long*)d_counts);
  PENGK_HIP(hipGetLastError());
  return PENGK_OK;
}

// ---- the pair table (--positional-null composition) -------------------------------------------------------
// The same tiles in the same static shares.  A position's bin is decided in the lane as in the count; what it adds is one of
// 16 pair values (two on both strands), and a poly-A run is 64 lanes on one counter: no lane adds for itself.  The lanes of a
// tile are consecutive positions, so a bin is a run of lanes (two under the centre anchor): the first lane of a run takes
// the run's lane mask, the wave ballots each pair value that occurs in the tile, and the run's first lane adds the popcount
// of ballot & mask to its bin's counter -- at most 16 LDS adds a lane and tile, each by the few lanes that begin a run, none
// where the value does not occur.  One table of n_bins x 16 uint32 a workgroup (4 KiB at most), shared by its waves.
constexpr uint32_t POS_PAIR_FLUSH_ROUNDS = 1u << 20;  // x 1024 positions a round x 2 strands = 2^31 per counter at most
constexpr uint32_t POS_NO_BIN = 0xFFFFFFFFu;

template <int K, bool BOTH>
__device__ __forceinline__ void pos_pair_tile(const uint64_t* __restrict__ wp, const uint32_t* __restrict__ vp, uint32_t L, uint32_t k,
                                              int anchor, uint32_t S, uint32_t R, uint32_t* tab) {
  constexpr uint32_t ALL = (1u << K) - 1u;
  const uint32_t D = L - (uint32_t)K;  // the last position
  const uint32_t P0 = k << 6;          // (k < 2^26)
  if (P0 > D) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t p = P0 + lane;
  // the window from p on: the word at p is the first K <= 7 of its bases
  const tile::Window win = tile::window(wp, vp, L, p, 0u);
  const uint32_t lo = win.lo, v = win.v;
  const uint32_t c = p <= D ? pos_coordinate(anchor, p, D) : R;
  const uint32_t bin = c < R ? c / S : POS_NO_BIN;
  const bool on = bin != POS_NO_BIN && (v & ALL) == ALL;  // (a word that stands ends inside the sequence: p <= D)
  if (__builtin_amdgcn_ballot_w64(on) == 0ull) return;
  const uint32_t fwd = ((lo & 3u) << 2) | ((lo >> 2) & 3u);                                                   // 4 s[p] + s[p+1]
  const uint32_t rev = (((~lo >> (2 * (K - 1))) & 3u) << 2) | ((~lo >> (2 * (K - 2))) & 3u);  // 4 (3 - s[p+K-1]) + 3 - s[p+K-2]
  // runs of one bin: a lane begins one where the lane before it has another bin
  const uint32_t before = (uint32_t)__shfl_up((int)bin, 1);
  const bool first = lane == 0u || before != bin;
  const uint64_t firsts = __builtin_amdgcn_ballot_w64(first);
  const uint64_t behind = lane == 63u ? 0ull : firsts & ~((2ull << lane) - 1ull);  // the runs that begin behind this lane
  const uint32_t next = behind ? (uint32_t)__builtin_ctzll(behind) : 64u;
  const uint64_t upto = next == 64u ? ~0ull : (1ull << next) - 1ull;
  const uint64_t run = upto & ~((1ull << lane) - 1ull);  // the lanes [lane, next)
  const bool adds = first && bin != POS_NO_BIN;
  uint32_t* row = tab + ((adds ? bin : 0u) << 4);
#pragma unroll
  for (uint32_t x = 0; x < 16u; ++x) {
    const uint64_t mf = __builtin_amdgcn_ballot_w64(on && fwd == x);
    const uint64_t mr = BOTH ? __builtin_amdgcn_ballot_w64(on && rev == x) : 0ull;
    if ((mf | mr) == 0ull) continue;  // (wave-uniform)
    const uint32_t n = (uint32_t)__builtin_popcountll(mf & run) + (BOTH ? (uint32_t)__builtin_popcountll(mr & run) : 0u);
    if (adds && n) atomicAdd(&row[x], n);
  }
}

__device__ __forceinline__ void pos_pair_flush(uint32_t* tab, int n, unsigned long long* __restrict__ pairs) {
  __syncthreads();
  for (int q = threadIdx.x; q < n; q += POS_THREADS) {
    const uint32_t c = tab[q];
    if (c) {
      tab[q] = 0u;
      atomicAdd(&pairs[q], (unsigned long long)c);
    }
  }
  __syncthreads();
}

template <int K, bool BOTH>
__global__ __launch_bounds__(POS_THREADS) void pos_pairs_kernel(const uint64_t* __restrict__ words, const uint32_t* __restrict__ valid,
                                                                const int64_t* __restrict__ offs, const uint32_t* __restrict__ lens,
                                                                uint64_t n_seq, int anchor, uint32_t S, int n_bins,
                                                                const unsigned long long* __restrict__ excl,
                                                                const unsigned long long* __restrict__ boff, uint64_t n_groups,
                                                                unsigned long long* __restrict__ pairs) {
  __shared__ uint32_t tab[PENGK_POSITION_MAX_BINS * 16];
  const int n_tab = n_bins * 16;
  const uint32_t R = (uint32_t)n_bins * S;
  // this wave's share of the tiles, as in pos_count_kernel; `per` rounds for every wave of the grid
  const tile::Share share = tile::share<POS_WAVES>(boff, n_groups);
  if (share.block_empty) return;  // (the whole workgroup)
  for (int q = threadIdx.x; q < n_tab; q += POS_THREADS) tab[q] = 0u;
  __syncthreads();
  uint64_t g = share.g;
  tile::Cursor<PosTilesOf> c{lens, n_seq, PosTilesOf{K, anchor, R}};
  if (g < share.gend) c.locate(g, excl, boff, n_groups);
  uint32_t since = 0;
  for (uint64_t round = 0; round < share.per; ++round) {  // (per, and so every barrier below, is the same for the whole grid)
    if (g < share.gend) {
      if (c.next()) {
        const uint64_t w0 = (uint64_t)offs[c.i] >> 5;
        pos_pair_tile<K, BOTH>(words + w0, valid ? valid + w0 : nullptr, c.L, c.t.k0 + c.k, anchor, S, R, tab);
      }
      ++c.k;
      ++g;
    }
    if (++since == POS_PAIR_FLUSH_ROUNDS) {
      pos_pair_flush(tab, n_tab, pairs);
      since = 0;
    }
  }
  if (since) pos_pair_flush(tab, n_tab, pairs);
}

template <int K, bool BOTH>
int pos_pairs_launch(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs, const uint32_t* d_lens,
                     uint64_t n_seq, int anchor, uint32_t S, int n_bins, const unsigned long long* excl, const unsigned long long* boff,
                     uint64_t n_groups, uint64_t* d_pairs) {
  const dim3 grid((unsigned)ctx->num_cu * 2u);  // (32 waves a CU: two workgroups of 1024 threads)
  hipLaunchKernelGGL((pos_pairs_kernel<K, BOTH>), grid, dim3(POS_THREADS), 0, ctx->stream, d_words, d_valid, d_offs, d_lens, n_seq, anchor,
                     S, n_bins, excl, boff, n_groups, (unsigned long long*)d_pairs);
  PENGK_HIP(hipGetLastError());
  return PENGK_OK;
}

// the argument checks, enter(ctx) and the plan of the tiles (tile_walk.h) that pengk_position_count and pengk_position_pairs share
int pos_prepare(pengk_ctx* ctx, const char* fn, const uint64_t* d_words, const int64_t* d_offs, const uint32_t* d_lens, uint64_t n_seq, int K,
                int anchor, int bin_size, int n_bins, int both_strands, const uint64_t* d_table, tile::Plan* plan) {
  if (!ctx || (n_seq && (!d_words || !d_offs || !d_lens || !d_table))) return fail(PENGK_ERR_ARG, "%s: bad argument", fn);
  if (K < PENGK_POSITION_MIN_K || K > PENGK_POSITION_MAX_K)
    return fail(PENGK_ERR_ARG, "%s: K %d out of range [%d,%d]", fn, K, PENGK_POSITION_MIN_K, PENGK_POSITION_MAX_K);
  if (anchor < 0 || anchor > 2) return fail(PENGK_ERR_ARG, "%s: anchor must be 0 (start), 1 (end) or 2 (centre)", fn);
  if (bin_size < 1 || bin_size > PENGK_POSITION_MAX_BIN_SIZE)
    return fail(PENGK_ERR_ARG, "%s: bin_size %d out of range [1,%d]", fn, bin_size, PENGK_POSITION_MAX_BIN_SIZE);
  if (n_bins < 1 || n_bins > PENGK_POSITION_MAX_BINS)
    return fail(PENGK_ERR_ARG, "%s: n_bins %d out of range [1,%d]", fn, n_bins, PENGK_POSITION_MAX_BINS);
  if (both_strands != 0 && both_strands != 1) return fail(PENGK_ERR_ARG, "%s: both_strands must be 0 or 1", fn);
  if (n_seq >> 32) return fail(PENGK_ERR_ARG, "%s: 2^32 sequences or more; shard the input", fn);
  int rc = enter(ctx);
  if (rc) return rc;
  if (n_seq == 0) return PENGK_OK;
  rc = ensure_scratch(ctx, &ctx->d_sites, &ctx->sites_bytes, tile::plan_bytes(n_seq));
  if (rc) return rc;
  *plan = tile::plan(ctx, ctx->d_sites, d_lens, n_seq, PosTilesOf{K, anchor, (uint32_t)bin_size * (uint32_t)n_bins});
  return PENGK_OK;
}

inline uint64_t pos_keys(int K, int both) {
  const uint64_t all = 1ull << (2 * K);
  if (!both) return all;
  return (K & 1) ? all / 2 : (all + (1ull << K)) / 2;
}

}  // namespace
}  // namespace pengk

using namespace pengk;

extern "C" {

int pengk_position_count(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs, const uint32_t* d_lens,
                         uint64_t n_seq, int K, int anchor, int bin_size, int n_bins, int both_strands, uint64_t* d_counts) {
  tile::Plan plan;
  const int rc = pos_prepare(ctx, "pengk_position_count", d_words, d_offs, d_lens, n_seq, K, anchor, bin_size, n_bins, both_strands, d_counts,
                             &plan);
  if (rc || n_seq == 0) return rc;
#define PENGK_POS_CASE(k)                                                                                                               \
  case k:                                                                                                                               \
    return both_strands ? pos_launch<k, true>(ctx, d_words, d_valid, d_offs, d_lens, n_seq, anchor, (uint32_t)bin_size, n_bins, plan.excl,  \
                                              plan.boff, plan.n_groups, d_counts)                                                       \
                        : pos_launch<k, false>(ctx, d_words, d_valid, d_offs, d_lens, n_seq, anchor, (uint32_t)bin_size, n_bins, plan.excl, \
                                               plan.boff, plan.n_groups, d_counts)
  switch (K) {
    PENGK_POS_CASE(4);
    PENGK_POS_CASE(5);
    PENGK_POS_CASE(6);
    PENGK_POS_CASE(7);
  }
#undef PENGK_POS_CASE
  return PENGK_OK;
}

int pengk_position_pairs(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs, const uint32_t* d_lens,
                         uint64_t n_seq, int K, int anchor, int bin_size, int n_bins, int both_strands, uint64_t* d_pairs) {
  tile::Plan plan;
  const int rc = pos_prepare(ctx, "pengk_position_pairs", d_words, d_offs, d_lens, n_seq, K, anchor, bin_size, n_bins, both_strands, d_pairs,
                             &plan);
  if (rc || n_seq == 0) return rc;
#define PENGK_POS_CASE(k)                                                                                                                     \
  case k:                                                                                                                                     \
    return both_strands ? pos_pairs_launch<k, true>(ctx, d_words, d_valid, d_offs, d_lens, n_seq, anchor, (uint32_t)bin_size, n_bins, plan.excl,  \
                                                    plan.boff, plan.n_groups, d_pairs)                                                        \
                        : pos_pairs_launch<k, false>(ctx, d_words, d_valid, d_offs, d_lens, n_seq, anchor, (uint32_t)bin_size, n_bins, plan.excl, \
                                                     plan.boff, plan.n_groups, d_pairs)
  switch (K) {
    PENGK_POS_CASE(4);
    PENGK_POS_CASE(5);
    PENGK_POS_CASE(6);
    PENGK_POS_CASE(7);
  }
#undef PENGK_POS_CASE
  return PENGK_OK;
}

int pengk_position_summary_null(const uint64_t* h_counts, const uint64_t* h_pairs, int K, int n_bins, int both_strands, uint64_t min_count,
                                double max_evalue, pengk_position_word* out, uint64_t capacity, uint64_t* n_out) {
  if (!h_counts || !n_out || (capacity && !out)) return fail(PENGK_ERR_ARG, "pengk_position_summary: bad argument");
  if (K < PENGK_POSITION_MIN_K || K > PENGK_POSITION_MAX_K)
    return fail(PENGK_ERR_ARG, "pengk_position_summary: K %d out of range [%d,%d]", K, PENGK_POSITION_MIN_K, PENGK_POSITION_MAX_K);
  if (n_bins < 1 || n_bins > PENGK_POSITION_MAX_BINS)
    return fail(PENGK_ERR_ARG, "pengk_position_summary: n_bins %d out of range [1,%d]", n_bins, PENGK_POSITION_MAX_BINS);
  if (both_strands != 0 && both_strands != 1) return fail(PENGK_ERR_ARG, "pengk_position_summary: both_strands must be 0 or 1");
  if (!(max_evalue > 0.0)) return fail(PENGK_ERR_ARG, "pengk_position_summary: max_evalue must be positive");
  *n_out = 0;
  const uint32_t NK = 1u << (2 * K);
  std::vector<uint64_t> N((size_t)n_bins, 0), C(NK, 0);
  uint64_t Nt = 0;
  for (int b = 0; b < n_bins; ++b)
    for (uint32_t key = 0; key < NK; ++key) {
      const uint64_t c = h_counts[(size_t)b * NK + key];
      N[b] += c;
      C[key] += c;
    }
  for (int b = 0; b < n_bins; ++b) Nt += N[b];
  if (Nt == 0) return PENGK_OK;
  std::vector<double> q((size_t)n_bins);
  for (int b = 0; b < n_bins; ++b) q[b] = (double)N[b] / (double)Nt;
  // the composition null: a bin's first-order chain from its pair table -- f[x], T[x][y] --, a word's probability under it
  std::vector<double> chain_f, chain_T;
  std::vector<char> chain_has;
  if (h_pairs) {
    chain_f.assign((size_t)n_bins * 4, 0.0);
    chain_T.assign((size_t)n_bins * 16, 0.0);
    chain_has.assign((size_t)n_bins, 0);
    for (int b = 0; b < n_bins; ++b) {
      uint64_t n1[4] = {0, 0, 0, 0}, all = 0;
      for (int x = 0; x < 4; ++x)
        for (int y = 0; y < 4; ++y) n1[x] += h_pairs[(size_t)b * 16 + 4 * x + y];
      for (int x = 0; x < 4; ++x) all += n1[x];
      if (all == 0) continue;
      chain_has[b] = 1;
      for (int x = 0; x < 4; ++x) {
        chain_f[(size_t)b * 4 + x] = (double)n1[x] / (double)all;
        for (int y = 0; y < 4; ++y)
          chain_T[(size_t)b * 16 + 4 * x + y] = (double)(h_pairs[(size_t)b * 16 + 4 * x + y] + 1) / (double)(n1[x] + 4);
      }
    }
  }
  auto word_probability = [&](int b, uint32_t w) {
    uint32_t x = (w >> (2 * (K - 1))) & 3u;
    double P = chain_f[(size_t)b * 4 + x];
    for (int i = 1; i < K; ++i) {
      const uint32_t y = (w >> (2 * (K - 1 - i))) & 3u;
      P *= chain_T[(size_t)b * 16 + 4 * x + y];
      x = y;
    }
    return P;
  };
  const double log_tests = std::log10((double)((uint64_t)n_bins * pos_keys(K, both_strands)));
  const double log_max = std::log10(max_evalue);
  std::vector<pengk_position_word> rep;
  for (uint32_t key = 0; key < NK; ++key) {
    if (C[key] == 0) continue;
    if (h_pairs) {  // q[b] of this key: its shares g_b / G
      double G = 0.0;
      for (int b = 0; b < n_bins; ++b) {
        double P = 0.0;
        if (chain_has[b]) {
          P = word_probability(b, key);
          if (both_strands) P = P + word_probability(b, revcomp32(key, K));
        }
        q[b] = (double)N[b] * P;
        G += q[b];
      }
      if (G == 0.0) continue;
      for (int b = 0; b < n_bins; ++b) q[b] = q[b] / G;
    }
    pengk_position_word best = {};
    bool have = false;
    uint32_t significant = 0;
    for (int b = 0; b < n_bins; ++b) {
      const uint64_t c = h_counts[(size_t)b * NK + key];
      if (c == 0 || c < min_count) continue;
      const double expected = (double)C[key] * q[b];
      if (!((double)c > expected)) continue;
      pengk_position_word w;
      w.key = key;
      w.bin = (uint32_t)b;
      w.count = c;
      w.total = C[key];
      w.bin_positions = N[b];
      w.expected = expected;
      const int rc = pengk_binomial_log10_sf(C[key], c, q[b], &w.log10_pvalue);
      if (rc) return rc;
      w.log10_evalue = w.log10_pvalue + log_tests;
      if (w.log10_evalue <= log_max) ++significant;
      if (!have || w.log10_evalue < best.log10_evalue) {
        best = w;
        have = true;
      }
    }
    if (!have || !(best.log10_evalue <= log_max)) continue;
    best.bins_significant = significant;
    best.family = 0;
    best.is_head = 0;
    rep.push_back(best);
  }
  std::sort(rep.begin(), rep.end(), [](const pengk_position_word& x, const pengk_position_word& y) {
    if (x.log10_evalue != y.log10_evalue) return x.log10_evalue < y.log10_evalue;
    if (x.bin != y.bin) return x.bin < y.bin;
    return x.key < y.key;
  });
  // families: the word as letters 0 .. 3; the heads so far, each tried at the offsets -2 .. 2
  auto letters = [K](uint32_t key, bool rc, uint8_t* s) {
    if (rc) key = revcomp32(key, K);
    for (int c = 0; c < K; ++c) s[c] = (uint8_t)((key >> (2 * (K - 1 - c))) & 3u);
  };
  auto related = [K](const uint8_t* X, const uint8_t* Y) {
    for (int o = -2; o <= 2; ++o) {
      int same = 0;
      bool clash = false;
      for (int c = 0; c < K; ++c) {
        const int cy = c - o;
        if (cy < 0 || cy >= K) continue;
        if (X[c] == Y[cy]) ++same;
        else clash = true;
      }
      if (!clash && same >= 4) return true;
    }
    return false;
  };
  std::vector<uint32_t> heads;  // indices into rep
  for (size_t k = 0; k < rep.size(); ++k) {
    uint8_t Y[2][8], X[8];
    letters(rep[k].key, false, Y[0]);
    if (both_strands) letters(rep[k].key, true, Y[1]);
    uint32_t fam = 0;
    for (uint32_t h : heads) {
      const uint32_t far = rep[h].bin > rep[k].bin ? rep[h].bin - rep[k].bin : rep[k].bin - rep[h].bin;
      if (far > 1u) continue;
      letters(rep[h].key, false, X);
      if (related(X, Y[0]) || (both_strands && related(X, Y[1]))) {
        fam = h + 1u;
        break;
      }
    }
    if (!fam) {
      heads.push_back((uint32_t)k);
      fam = (uint32_t)k + 1u;
      rep[k].is_head = 1;
    }
    rep[k].family = fam;
  }
  *n_out = rep.size();
  for (size_t k = 0; k < rep.size() && k < capacity; ++k) out[k] = rep[k];
  return PENGK_OK;
}

int pengk_position_summary(const uint64_t* h_counts, int K, int n_bins, int both_strands, uint64_t min_count, double max_evalue,
                           pengk_position_word* out, uint64_t capacity, uint64_t* n_out) {
  return pengk_position_summary_null(h_counts, nullptr, K, n_bins, both_strands, min_count, max_evalue, out, capacity, n_out);
}

}  // extern "C"
