// dyad.hip -- spaced trinucleotide pairs counted on the device (--dyads): the tables defined in
// include/pengk.h ("spaced dyads").
//
//   tile     64 consecutive positions of one sequence, one wave, one position per lane.  A lane reads the 32 bases from its
//            position on (they lie in the word of the position and the one after it: a dyad spans at most 6 +
//            PENGK_DYAD_MAX_GAP = 32 bases) and the validity bits of the same bases; r = their run of ones from bit 0 on
//            decides every gap of the position at once (r >= 6 + g is monotone in g).
//   groups   the gaps 0 .. max_gap in groups of at most DYAD_GROUP = 8; a workgroup owns one group (blockIdx.y) and keeps
//            its tables in LDS, 4096 uint32 bins (16 KiB) a gap: 128 KiB at most, one workgroup of 1024 threads a CU.
//            Bins are bumped with non-returning LDS adds; the first group also counts the triplets (64 bins).
//   keys     inside a workgroup a dyad is the 12 bits  e(a) | e(b) << 6,  e the triplet as the words hold it (first base
//            lowest), so a is the low six bits of the lane's window and b a six-bit field of it.  The reverse complement of
//            that code is the six-digit reverse complement of the 12 bits; with the window's 32-digit reverse complement
//            taken once per position it is two more fields.  On both strands the smaller of the two codes is bumped.  The
//            flush turns a bin's code into the public key (first base highest), folds it again in that order -- a pair
//            {code, its reverse complement} is one bin here and one there -- and adds the bin to the uint64 table with a
//            plain vector atomic; empty bins add nothing, so no entry that is not canonical is ever written.
//   tiles    tile counts per sequence -> exclusive sums, then every wave of a fixed grid walks one contiguous share of
//            the tiles: the plan, the share and the cursor of tile_walk.h.  Every wave of the grid runs the same number
//            of rounds, so the barriers of the flush sit in workgroup-uniform control flow.
//   wrap     a position bumps a bin at most once, a round of a workgroup holds at most 1024 positions, and the tables are
//            flushed every DYAD_FLUSH_ROUNDS = 2^21 rounds: no bin exceeds 2^31 between two flushes.
// Nothing of size positions x gaps is written to HBM.
#include <algorithm>
#include <cmath>
#include <vector>

#include "pengk_internal.h"
#include "tile_walk.h"

namespace pengk {
namespace {

constexpr int DYAD_THREADS = 1024;
constexpr int DYAD_WAVES = DYAD_THREADS / 64;
constexpr int DYAD_GROUP = 8;                     // gaps a workgroup holds at most
constexpr int DYAD_BINS = 4096;
constexpr uint32_t DYAD_FLUSH_ROUNDS = 1u << 21;  // x 1024 positions a round = 2^31 per bin at most
static_assert(6 + PENGK_DYAD_MAX_GAP == 32, "a position's span lies in its word and the next");
static_assert(DYAD_GROUP * DYAD_BINS * 4 + 256 <= 160 * 1024, "a group's tables and the triplets fit in LDS");

__host__ __device__ __forceinline__ uint32_t dyad_tiles(uint32_t L) { return L < 3u ? 0u : ((L - 3u) >> 6) + 1u; }

struct DyadTilesOf {
  __device__ __forceinline__ tile::Tiles operator()(uint32_t L) const { return tile::Tiles{dyad_tiles(L)}; }
};

// ---- the count ----------------------------------------------------------------------------------------------------------
// the reverse complement of 32 bases (first base lowest): the digits complemented and in reverse order
__device__ __forceinline__ uint64_t dyad_rc64(uint64_t x) {
  uint32_t lo = __brev(~(uint32_t)(x >> 32)), hi = __brev(~(uint32_t)x);
  lo = ((lo & 0xAAAAAAAAu) >> 1) | ((lo & 0x55555555u) << 1);  // un-reverse the two bits of each digit
  hi = ((hi & 0xAAAAAAAAu) >> 1) | ((hi & 0x55555555u) << 1);
  return (uint64_t)lo | ((uint64_t)hi << 32);
}

// One tile: the positions [64 k, 64 k + 64) of a sequence of L bases whose words / validity words begin at wp / vp (vp
// NULL: every base valid), under the gaps [g0, g1) and max_gap; bins: this workgroup's (g1 - g0) tables, mono: its 64
// triplet bins (NULL: another group counts them).
template <bool BOTH>
__device__ __forceinline__ void dyad_tile(const uint64_t* __restrict__ wp, const uint32_t* __restrict__ vp, uint32_t L, uint32_t k,
                                          int g0, int g1, uint32_t* bins, uint32_t* mono) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t nw = (L + 31u) >> 5;
  const uint32_t j = 2u * k + (lane >> 5);  // the word of this lane's position (k < 2^26)
  const uint32_t s = lane & 31u;            // ... and its place in it
  const uint64_t W0 = j < nw ? wp[j] : 0ull, W1 = j + 1u < nw ? wp[j + 1u] : 0ull;
  const uint32_t V0 = tile::valid_word(vp, L, nw, j), V1 = tile::valid_word(vp, L, nw, j + 1u);
  const uint64_t x = s ? (W0 >> (2u * s)) | (W1 << (64u - 2u * s)) : W0;  // the 32 bases from the position on
  const uint32_t v = s ? (V0 >> s) | (V1 << (32u - s)) : V0;              // ... and their validity bits
  const uint32_t r = v == 0xFFFFFFFFu ? 32u : (uint32_t)__builtin_ctz(~v);
  const uint32_t ea = (uint32_t)x & 63u;
  if (mono && r >= 3u) atomicAdd(&mono[ea], 1u);
  // this position's gaps: g with 6 + g <= r, within [g0, g1)
  const int hi = r >= 6u ? std::min<int>((int)r - 5, g1) : 0;
  uint64_t xs = x >> (6 + 2 * g0);
  uint64_t ys = 0;
  uint32_t rca = 0;
  if (BOTH) {
    const uint64_t y = dyad_rc64(x);
    rca = (uint32_t)(y >> 58) << 6;
    ys = y << (6 + 2 * g0);
  }
  uint32_t* b = bins;
  for (int g = g0; g < g1; ++g) {
    const bool on = g < hi;
    if (__ballot(on) == 0ull) break;  // (hi falls with nothing: no later gap has a lane either)
    uint32_t code = ea | (((uint32_t)xs & 63u) << 6);
    if (BOTH) {
      const uint32_t rc = (uint32_t)(ys >> 58) | rca;
      code = rc < code ? rc : code;
    }
    if (on) atomicAdd(&b[code], 1u);
    xs >>= 2;
    ys <<= 2;
    b += DYAD_BINS;
  }
}

// the public key of a bin: the six digits of its code in reverse order (first base highest), folded on both strands
template <bool BOTH>
__device__ __forceinline__ uint32_t dyad_public_key(uint32_t code) {
  const uint32_t key = revcomp32(~code, 6);
  if (!BOTH) return key;
  const uint32_t rc = revcomp32(key, 6);
  return rc < key ? rc : key;
}

template <bool BOTH>
__device__ __forceinline__ void dyad_flush(uint32_t* bins, uint32_t* mono, int g0, int ng, bool with_mono,
                                           unsigned long long* __restrict__ counts, unsigned long long* __restrict__ mono_out) {
  __syncthreads();
  for (int q = threadIdx.x; q < ng * DYAD_BINS; q += DYAD_THREADS) {
    const uint32_t c = bins[q];
    if (c) {
      bins[q] = 0u;
      atomicAdd(&counts[(uint64_t)(g0 + q / DYAD_BINS) * DYAD_BINS + dyad_public_key<BOTH>((uint32_t)q % DYAD_BINS)], (unsigned long long)c);
    }
  }
  if (with_mono && threadIdx.x < 64) {
    const uint32_t e = threadIdx.x, c = mono[e];
    mono[e] = 0u;
    if (c) atomicAdd(&mono_out[((e & 3u) << 4) | (e & 12u) | (e >> 4)], (unsigned long long)c);
  }
  __syncthreads();
}

template <bool BOTH>
__global__ __launch_bounds__(DYAD_THREADS) void dyad_count_kernel(const uint64_t* __restrict__ words, const uint32_t* __restrict__ valid,
                                                                  const int64_t* __restrict__ offs, const uint32_t* __restrict__ lens,
                                                                  uint64_t n_seq, int n_gaps, int per_group,
                                                                  const unsigned long long* __restrict__ excl,
                                                                  const unsigned long long* __restrict__ boff, uint64_t n_groups,
                                                                  unsigned long long* __restrict__ counts,
                                                                  unsigned long long* __restrict__ mono_out) {
  extern __shared__ __attribute__((aligned(16))) uint32_t sh[];  // (g1 - g0) tables | 64 triplet bins
  const int g0 = (int)blockIdx.y * per_group, g1 = std::min(n_gaps, g0 + per_group), ng = g1 - g0;
  uint32_t* bins = sh;
  uint32_t* mono = sh + ng * DYAD_BINS;
  const bool with_mono = blockIdx.y == 0;
  // this wave's share of the tiles; `per` rounds for every wave of the grid
  const tile::Share share = tile::share<DYAD_WAVES>(boff, n_groups);
  if (share.block_empty) return;  // (the whole workgroup: nothing to zero, nothing to flush)
  for (int q = threadIdx.x; q < ng * DYAD_BINS + 64; q += DYAD_THREADS) sh[q] = 0u;
  __syncthreads();
  uint64_t g = share.g;
  tile::Cursor<DyadTilesOf> c{lens, n_seq, DyadTilesOf{}};
  if (g < share.gend) c.locate(g, excl, boff, n_groups);
  uint32_t since = 0;
  for (uint64_t round = 0; round < share.per; ++round) {  // (per, and so every barrier below, is the same for the whole grid)
    if (g < share.gend) {
      if (c.next()) {
        const uint64_t w0 = (uint64_t)offs[c.i] >> 5;
        dyad_tile<BOTH>(words + w0, valid ? valid + w0 : nullptr, c.L, c.k, g0, g1, bins, with_mono ? mono : nullptr);
      }
      ++c.k;
      ++g;
    }
    if (++since == DYAD_FLUSH_ROUNDS) {
      dyad_flush<BOTH>(bins, mono, g0, ng, with_mono, counts, mono_out);
      since = 0;
    }
  }
  if (since) dyad_flush<BOTH>(bins, mono, g0, ng, with_mono, counts, mono_out);
}

}  // namespace
}  // namespace pengk

using namespace pengk;

extern "C" {

int pengk_dyad_count(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs, const uint32_t* d_lens,
                     uint64_t n_seq, int max_gap, int both_strands, uint64_t* d_counts, uint64_t* d_mono) {
  if (!ctx || (n_seq && (!d_words || !d_offs || !d_lens || !d_counts || !d_mono)))
    return fail(PENGK_ERR_ARG, "pengk_dyad_count: bad argument");
  if (max_gap < 0 || max_gap > PENGK_DYAD_MAX_GAP)
    return fail(PENGK_ERR_ARG, "pengk_dyad_count: max_gap %d out of range [0,%d]", max_gap, PENGK_DYAD_MAX_GAP);
  if (both_strands != 0 && both_strands != 1) return fail(PENGK_ERR_ARG, "pengk_dyad_count: both_strands must be 0 or 1");
  if (n_seq >> 32) return fail(PENGK_ERR_ARG, "pengk_dyad_count: 2^32 sequences or more; shard the input");
  int rc = enter(ctx);
  if (rc) return rc;
  if (n_seq == 0) return PENGK_OK;
  rc = ensure_scratch(ctx, &ctx->d_sites, &ctx->sites_bytes, tile::plan_bytes(n_seq));
  if (rc) return rc;
  // the gaps in equal groups of at most DYAD_GROUP: 21 gaps are 3 x 7, 27 are 4 x 7
  const int n_gaps = max_gap + 1;
  const int gap_groups = (n_gaps + DYAD_GROUP - 1) / DYAD_GROUP;
  const int per_group = (n_gaps + gap_groups - 1) / gap_groups;
  const size_t lds = (size_t)per_group * DYAD_BINS * sizeof(uint32_t) + 64 * sizeof(uint32_t);
  const unsigned per_cu = lds * 2 <= 160 * 1024 ? 2u : 1u;  // (32 waves a CU: two workgroups of 1024 threads at most)
  const dim3 grid((unsigned)ctx->num_cu * per_cu, (unsigned)gap_groups);
  const tile::Plan plan = tile::plan(ctx, ctx->d_sites, d_lens, n_seq, DyadTilesOf{});
  if (both_strands) {
    PENGK_HIP(hipFuncSetAttribute((const void*)dyad_count_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(dyad_count_kernel<true>, grid, dim3(DYAD_THREADS), lds, ctx->stream, d_words, d_valid, d_offs, d_lens, n_seq,
                       n_gaps, per_group, plan.excl, plan.boff, plan.n_groups, (unsigned long long*)d_counts, (unsigned long long*)d_mono);
  } else {
    PENGK_HIP(hipFuncSetAttribute((const void*)dyad_count_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(dyad_count_kernel<false>, grid, dim3(DYAD_THREADS), lds, ctx->stream, d_words, d_valid, d_offs, d_lens, n_seq,
                       n_gaps, per_group, plan.excl, plan.boff, plan.n_groups, (unsigned long long*)d_counts, (unsigned long long*)d_mono);
  }
  PENGK_HIP(hipGetLastError());
  return PENGK_OK;
}

int pengk_dyad_summary(const uint64_t* h_counts, const uint64_t* h_mono, int max_gap, int both_strands, uint64_t min_count,
                       double max_evalue, pengk_dyad* out, uint64_t capacity, uint64_t* n_out) {
  if (!h_counts || !h_mono || !n_out || (capacity && !out)) return fail(PENGK_ERR_ARG, "pengk_dyad_summary: bad argument");
  if (max_gap < 0 || max_gap > PENGK_DYAD_MAX_GAP)
    return fail(PENGK_ERR_ARG, "pengk_dyad_summary: max_gap %d out of range [0,%d]", max_gap, PENGK_DYAD_MAX_GAP);
  if (both_strands != 0 && both_strands != 1) return fail(PENGK_ERR_ARG, "pengk_dyad_summary: both_strands must be 0 or 1");
  if (!(max_evalue > 0.0)) return fail(PENGK_ERR_ARG, "pengk_dyad_summary: max_evalue must be positive");
  *n_out = 0;
  uint64_t M = 0;
  for (int x = 0; x < 64; ++x) M += h_mono[x];
  if (M == 0) return PENGK_OK;
  double f[64];
  for (uint32_t x = 0; x < 64; ++x)
    f[x] = both_strands ? (double)(h_mono[x] + h_mono[revcomp32(x, 3)]) / (2.0 * (double)M) : (double)h_mono[x] / (double)M;
  const int n_gaps = max_gap + 1;
  const double log_tests = std::log10((double)((uint64_t)n_gaps * (both_strands ? 2080u : 4096u)));
  const double log_max = std::log10(max_evalue);
  std::vector<pengk_dyad> rep;
  for (int g = 0; g < n_gaps; ++g) {
    const uint64_t* row = h_counts + (size_t)g * DYAD_BINS;
    uint64_t T = 0;
    for (int key = 0; key < DYAD_BINS; ++key) T += row[key];
    for (uint32_t key = 0; key < (uint32_t)DYAD_BINS; ++key) {
      const uint64_t c = row[key];
      if (c == 0 || c < min_count) continue;
      double p = f[key >> 6] * f[key & 63u];
      if (both_strands && revcomp32(key, 6) != key) p *= 2.0;
      const double expected = (double)T * p;
      if (!((double)c > expected)) continue;
      pengk_dyad d;
      d.gap = (uint32_t)g;
      d.key = key;
      d.count = c;
      d.positions = T;
      d.p = p;
      d.expected = expected;
      const int rc = pengk_binomial_log10_sf(T, c, p, &d.log10_pvalue);
      if (rc) return rc;
      d.log10_evalue = d.log10_pvalue + log_tests;
      if (!(d.log10_evalue <= log_max)) continue;
      uint64_t other = 0;
      for (int h = 0; h < n_gaps; ++h)
        if (h != g) other += h_counts[(size_t)h * DYAD_BINS + key];
      d.other_gaps_mean = max_gap ? (double)other / (double)max_gap : 0.0;
      d.family = 0;
      d.is_head = 0;
      rep.push_back(d);
    }
  }
  std::sort(rep.begin(), rep.end(), [](const pengk_dyad& x, const pengk_dyad& y) {
    if (x.log10_evalue != y.log10_evalue) return x.log10_evalue < y.log10_evalue;
    if (x.gap != y.gap) return x.gap < y.gap;
    return x.key < y.key;
  });
  // families: the dyad as letters 0 .. 3 and 4 for n; the heads so far, each tried at the offsets -2 .. 2
  auto letters = [](uint32_t key, uint32_t g, bool rc, uint8_t* s) {
    if (rc) key = revcomp32(key, 6);
    const uint32_t n = 6u + g;
    for (uint32_t c = 0; c < n; ++c) s[c] = 4;
    for (uint32_t c = 0; c < 3; ++c) {
      s[c] = (uint8_t)((key >> (10u - 2u * c)) & 3u);
      s[3u + g + c] = (uint8_t)((key >> (4u - 2u * c)) & 3u);
    }
    return n;
  };
  auto related = [](const uint8_t* X, int nx, const uint8_t* Y, int ny) {
    for (int o = -2; o <= 2; ++o) {
      int same = 0;
      bool clash = false;
      for (int c = 0; c < nx; ++c) {
        const int cy = c - o;
        if (cy < 0 || cy >= ny || X[c] == 4 || Y[cy] == 4) continue;
        if (X[c] == Y[cy]) ++same;
        else clash = true;
      }
      if (!clash && same >= 4) return true;
    }
    return false;
  };
  std::vector<uint32_t> heads;  // indices into rep
  for (size_t k = 0; k < rep.size(); ++k) {
    uint8_t Y[2][32], X[32];
    const int ny = (int)letters(rep[k].key, rep[k].gap, false, Y[0]);
    if (both_strands) letters(rep[k].key, rep[k].gap, true, Y[1]);
    uint32_t fam = 0;
    for (uint32_t h : heads) {
      const int nx = (int)letters(rep[h].key, rep[h].gap, false, X);
      if (related(X, nx, Y[0], ny) || (both_strands && related(X, nx, Y[1], ny))) {
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

}  // extern "C"
