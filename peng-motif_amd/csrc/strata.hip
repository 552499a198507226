// strata.hip -- the background counters of every GC stratum of a scan layout (pengk_strata_bg_count,
// --stratified-background): 84 (k+1)-mer counters a stratum and its windows, in one pass over the words.
//
//   tile     64 consecutive positions of one sequence, one wave, one position per lane: the window of tile_walk.h with
//            two bases behind the position, 16 bases and 32 validity bits from q = max(p - 2, 0) on.  The lane's key is the 3-mer ending at p in BaMM order -- its low 4 bits are the
//            2-mer, its low 2 bits the base -- and three flags say which of the three orders stand there.
//   counts   no atomic per base.  Six ballots give the key's bits over the wave; lane b selects the lanes whose key is
//            b (six ands of a ballot or its complement) and counts them under the three flags' ballots with a
//            population count: lane b carries the count of 3-mer b, lanes 0..15 those of the 2-mers, lanes 0..3 those
//            of the bases, in registers, over all tiles of the sequence.  All A costs what any other input costs.
//   strata   a wave works on one sequence at a time (sequence i goes to wave i mod waves), so its stratum is uniform:
//            at the sequence's end every lane adds its three registers to the wave's OWN histogram in LDS -- n_strata
//            rows of 84 counters and the windows, uint32 -- with plain reads and writes: no other wave touches them.
//   flush    at the end the workgroup adds its waves' histograms (uint64) and sends one global atomic per non-zero
//            counter.  A wave whose next sequence would take it beyond 2^25 tiles since its last flush (2^31 positions: no
//            uint32 counter can wrap) sends its own histogram first.
// d_bg holds n_strata x 84 uint64 and is ADDED to; nothing else is written but d_windows.
#include "pengk_internal.h"
#include "scan_walk.h"
#include "tile_walk.h"

namespace pengk {
namespace {

constexpr int SBG_THREADS = 512;
constexpr int SBG_WAVES = SBG_THREADS / 64;
constexpr int SBG_ROW = 85;                      // 84 counters and the stratum's windows
constexpr uint32_t SBG_FLUSH_TILES = 1u << 25;   // x 64 positions = 2^31 per counter at most between two flushes
constexpr int SBG_PER_CU = 4;                    // workgroups a CU: 32 waves (16 strata take 43.5 KB of LDS each: three)
static_assert(SBG_WAVES * 16 * SBG_ROW * 4 <= 64 * 1024, "a workgroup's histograms fit in the LDS a launch may ask for");

__device__ __forceinline__ unsigned long long sbg_pick(unsigned long long ballot, uint32_t bit) { return bit ? ballot : ~ballot; }

// the wave's own histogram -> the global tables (skips what is zero), and zeroes it
__device__ __forceinline__ void sbg_wave_flush(uint32_t* mine, int n_strata, unsigned long long* __restrict__ bg,
                                               unsigned long long* __restrict__ windows) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t q = lane; q < (uint32_t)(n_strata * SBG_ROW); q += 64u) {
    const uint32_t c = mine[q];
    if (!c) continue;
    mine[q] = 0u;
    const uint32_t s = q / SBG_ROW, b = q % SBG_ROW;
    if (b < 84u)
      atomicAdd(&bg[s * 84u + b], (unsigned long long)c);
    else if (windows)
      atomicAdd(&windows[s], (unsigned long long)c);
  }
}

__global__ __launch_bounds__(SBG_THREADS) void strata_bg_kernel(const uint64_t* __restrict__ words, const uint32_t* __restrict__ valid,
                                                                const int64_t* __restrict__ offs, const uint32_t* __restrict__ lens,
                                                                uint64_t n_seq, const uint16_t* __restrict__ stratum, int n_strata,
                                                                int W, unsigned long long* __restrict__ bg,
                                                                unsigned long long* __restrict__ windows) {
  extern __shared__ __attribute__((aligned(16))) uint32_t sh[];  // SBG_WAVES x n_strata x SBG_ROW
  const int per_wave = n_strata * SBG_ROW;
  for (int q = threadIdx.x; q < SBG_WAVES * per_wave; q += SBG_THREADS) sh[q] = 0u;
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave_in = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint32_t* mine = sh + wave_in * per_wave;
  const uint64_t n_waves = (uint64_t)gridDim.x * SBG_WAVES;
  const uint32_t wmask = (1u << W) - 1u;  // (W <= 14)
  const uint32_t b0 = lane & 1u, b1 = (lane >> 1) & 1u, b2 = (lane >> 2) & 1u, b3 = (lane >> 3) & 1u, b4 = (lane >> 4) & 1u,
                 b5 = (lane >> 5) & 1u;
  uint32_t since = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * SBG_WAVES + wave_in; i < n_seq; i += n_waves) {
    const uint32_t s = (uint32_t)__builtin_amdgcn_readfirstlane((int)stratum[i]);
    if (s >= (uint32_t)n_strata) continue;
    const uint32_t L = (uint32_t)__builtin_amdgcn_readfirstlane((int)lens[i]);
    if (L == 0u) continue;
    const uint64_t w0 = (uint64_t)offs[i] >> 5;
    const uint64_t* wp = words + w0;
    const uint32_t* vp = valid ? valid + w0 : nullptr;
    const uint32_t n_tiles = ((L - 1u) >> 6) + 1u;
    uint32_t c1 = 0, c2 = 0, c3 = 0, win = 0;  // (a sequence holds fewer than 2^32 positions)
    for (uint32_t t = 0; t < n_tiles; ++t) {
      const uint32_t p = (t << 6) + lane;  // (p < L + 64: L <= 2^32 - 64 is checked by no one; p wraps only beyond it)
      const tile::Window w = tile::window(wp, vp, L, p, 2u);
      const uint32_t lo = w.lo, v = w.v, off = w.off;  // (off: 2 but at the sequence's start)
      // the bases x_{p-2} x_{p-1} x_p, older base more significant; what lies before the sequence reads as A and stands nowhere
      const uint32_t three = lo & 63u;  // first base lowest
      const uint32_t x0 = three & 3u, x1 = (three >> 2) & 3u, x2 = three >> 4;
      const uint32_t key = off == 2u ? (x0 << 4) | (x1 << 2) | x2 : (off == 1u ? (x0 << 2) | x1 : x0);
      const bool ok1 = (v >> off) & 1u;
      const bool ok2 = ok1 && off >= 1u && ((v >> (off - 1u)) & 1u);
      const bool ok3 = ok2 && off >= 2u && (v & 1u);
      const bool okw = ((v >> off) & wmask) == wmask;
      const unsigned long long m2 = sbg_pick(__ballot(key & 1u), b0) & sbg_pick(__ballot(key & 2u), b1);
      const unsigned long long m4 = m2 & sbg_pick(__ballot(key & 4u), b2) & sbg_pick(__ballot(key & 8u), b3);
      const unsigned long long m6 = m4 & sbg_pick(__ballot(key & 16u), b4) & sbg_pick(__ballot(key & 32u), b5);
      c1 += (uint32_t)__popcll(m2 & __ballot(ok1));
      c2 += (uint32_t)__popcll(m4 & __ballot(ok2));
      c3 += (uint32_t)__popcll(m6 & __ballot(ok3));
      win += (uint32_t)__popcll(__ballot(okw));
    }
    if (since + n_tiles > SBG_FLUSH_TILES) {  // (n_tiles <= 2^26: a sequence alone stays below 2^32 as well)
      sbg_wave_flush(mine, n_strata, bg, windows);
      since = 0;
    }
    since += n_tiles;
    uint32_t* row = mine + s * SBG_ROW;
    if (lane < 4u) row[lane] += c1;
    if (lane < 16u) row[4u + lane] += c2;
    row[20u + lane] += c3;
    if (lane == 0u) row[84] += win;
  }
  __syncthreads();
  for (int q = threadIdx.x; q < per_wave; q += SBG_THREADS) {
    unsigned long long c = 0;
    for (int w = 0; w < SBG_WAVES; ++w) c += sh[w * per_wave + q];
    if (!c) continue;
    const int s = q / SBG_ROW, b = q % SBG_ROW;
    if (b < 84)
      atomicAdd(&bg[s * 84 + b], c);
    else if (windows)
      atomicAdd(&windows[s], c);
  }
}

}  // namespace
}  // namespace pengk

using namespace pengk;

extern "C" {

int pengk_strata_bg_count(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                          const uint32_t* d_lens, uint64_t n_seq, const uint16_t* d_stratum, int n_strata, int W, uint64_t* d_bg,
                          uint64_t* d_windows) {
  if (!ctx || (n_seq && (!d_words || !d_offs || !d_lens || !d_stratum || !d_bg)))
    return fail(PENGK_ERR_ARG, "pengk_strata_bg_count: bad argument");
  if (n_strata < 1 || n_strata > 16) return fail(PENGK_ERR_ARG, "pengk_strata_bg_count: n_strata %d out of range [1,16]", n_strata);
  if (!valid_w(W)) return fail(PENGK_ERR_ARG, "pengk_strata_bg_count: pattern length %d unsupported", W);
  if (n_seq >= (1ull << 32)) return fail(PENGK_ERR_ARG, "pengk_strata_bg_count: 2^32 sequences or more; shard the input");
  int rc = enter(ctx);
  if (rc) return rc;
  if (n_seq == 0) return PENGK_OK;
  const size_t lds = (size_t)SBG_WAVES * n_strata * SBG_ROW * sizeof(uint32_t);
  const size_t fit = (size_t)160 * 1024 / lds;
  const int grid = grid_for(ctx, n_seq, SBG_WAVES, fit < (size_t)SBG_PER_CU ? (uint32_t)fit : (uint32_t)SBG_PER_CU);
  hipLaunchKernelGGL(strata_bg_kernel, dim3(grid), dim3(SBG_THREADS), lds, ctx->stream, d_words, d_valid, d_offs, d_lens, n_seq,
                     d_stratum, n_strata, W, (unsigned long long*)d_bg, (unsigned long long*)d_windows);
  PENGK_HIP(hipGetLastError());
  return PENGK_OK;
}

}  // extern "C"
