// bg_order.hip -- the background counters of orders 0 .. K <= 5 of a scan layout (pengk_bg_count_order,
// --high-order-background): (4^(K+2) - 4) / 3 (k+1)-mer counters in one pass over the words.
//
//   tile     64 consecutive positions of one sequence, one wave, one position per lane: the window of tile_walk.h with
//            five bases behind the position, 16 bases and 32 validity bits from q = max(p - 5, 0) on.
//   longest  a position with a valid base sends ONE LDS atomic: to the table of its longest available order
//            m = min(K, valid bases right behind it, p), at the (m+1)-mer ending at p in BaMM order.  (strata.hip's ballots
//            stop at 64 keys; order 5 has 4096.)  Lanes that hold the key of the wave's first counting lane -- all of them
//            in a homopolymer run -- are taken out by a ballot and added by one lane; the others send their own.
//   fold     the lower orders follow at the flush: count_k(y) = longest_k(y) + sum over b of count_{k+1}(b y), from
//            k = K - 1 down, in LDS; then one global atomic per non-zero counter.
//   flush    the workgroup's waves share ONE histogram (5460 uint32 at K = 5, 21.8 KB).  The sequence loop is uniform over
//            the workgroup: a round gives each wave one sequence and a CHUNK of at most BGO_CHUNK_TILES of its tiles, every
//            wave reads the round's lengths, and the workgroup flushes together before a round that would take it beyond
//            2^25 tiles since the last flush (2^31 positions: no uint32 counter, folded or not, can wrap).
// d_bg is ADDED to; nothing else is written.
#include "pengk_internal.h"
#include "scan_walk.h"
#include "tile_walk.h"

namespace pengk {
namespace {

constexpr int BGO_THREADS = 512;
constexpr int BGO_WAVES = BGO_THREADS / 64;
constexpr int BGO_MAX_K = 5;
constexpr uint32_t BGO_FLUSH_TILES = 1u << 25;                     // x 64 positions = 2^31 per counter at most between two flushes
constexpr uint32_t BGO_CHUNK_TILES = BGO_FLUSH_TILES / BGO_WAVES;  // a round: at most BGO_FLUSH_TILES tiles over the waves
constexpr int BGO_PER_CU = 4;                                      // workgroups a CU: 32 waves, 87 KB of LDS at K = 5


// the 16 two-bit digits of e in reverse order
__device__ __forceinline__ uint32_t bgo_reverse_digits(uint32_t e) {
  const uint32_t r = __builtin_bitreverse32(e);
  return ((r >> 1) & 0x55555555u) | ((r & 0x55555555u) << 1);
}

// the workgroup's histogram (longest orders) -> every order's counters -> the global table; leaves it zeroed.
// Called by all threads of the workgroup.
__device__ __forceinline__ void bgo_flush(uint32_t* sh, int K, unsigned long long* __restrict__ bg) {
  __syncthreads();
  for (int k = K - 1; k >= 0; --k) {
    const uint32_t ny = 1u << (2 * (k + 1)), at = order_table_at(k), up = order_table_at(k + 1);
    for (uint32_t y = threadIdx.x; y < ny; y += BGO_THREADS)
      sh[at + y] += sh[up + y] + sh[up + ny + y] + sh[up + 2u * ny + y] + sh[up + 3u * ny + y];
    __syncthreads();
  }
  const uint32_t total = order_table_at(K + 1);
  for (uint32_t q = threadIdx.x; q < total; q += BGO_THREADS) {
    const uint32_t c = sh[q];
    if (!c) continue;
    sh[q] = 0u;
    atomicAdd(&bg[q], (unsigned long long)c);
  }
  __syncthreads();
}

__global__ __launch_bounds__(BGO_THREADS) void bg_order_kernel(const uint64_t* __restrict__ words, const uint32_t* __restrict__ valid,
                                                               const int64_t* __restrict__ offs, const uint32_t* __restrict__ lens,
                                                               uint64_t n_seq, int K, unsigned long long* __restrict__ bg) {
  extern __shared__ __attribute__((aligned(16))) uint32_t sh[];  // order_table_at(K + 1) counters
  const uint32_t total = order_table_at(K + 1);
  for (uint32_t q = threadIdx.x; q < total; q += BGO_THREADS) sh[q] = 0u;
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave_in = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint64_t n_waves = (uint64_t)gridDim.x * BGO_WAVES;
  const uint32_t uK = (uint32_t)K;
  uint32_t since = 0;
  for (uint64_t base = (uint64_t)blockIdx.x * BGO_WAVES; base < n_seq; base += n_waves) {  // (uniform over the workgroup)
    // the round's sequences: every wave reads all of their lengths, so that chunks and flushes are the workgroup's
    uint32_t most = 0;
    for (int w = 0; w < BGO_WAVES; ++w) {
      if (base + (uint64_t)w >= n_seq) break;
      const uint32_t Lw = (uint32_t)__builtin_amdgcn_readfirstlane((int)lens[base + w]);
      const uint32_t tw = Lw ? ((Lw - 1u) >> 6) + 1u : 0u;
      most = tw > most ? tw : most;
    }
    const uint64_t i = base + wave_in;
    const bool mine = i < n_seq;
    const uint32_t L = mine ? (uint32_t)__builtin_amdgcn_readfirstlane((int)lens[i]) : 0u;
    const uint32_t n_tiles = L ? ((L - 1u) >> 6) + 1u : 0u;
    const uint64_t w0 = L ? (uint64_t)offs[i] >> 5 : 0ull;
    const uint64_t* wp = words + w0;
    const uint32_t* vp = valid ? valid + w0 : nullptr;
    for (uint32_t t0 = 0; t0 < most; t0 += BGO_CHUNK_TILES) {  // (one chunk but for sequences beyond 2^28 bases)
      const uint32_t left = most - t0;
      const uint32_t round_tiles = (left < BGO_CHUNK_TILES ? left : BGO_CHUNK_TILES) * (uint32_t)BGO_WAVES;  // (an upper bound, <= BGO_FLUSH_TILES)
      if (since + round_tiles > BGO_FLUSH_TILES) {
        bgo_flush(sh, K, bg);
        since = 0;
      }
      since += round_tiles;
      const uint32_t t1 = t0 + BGO_CHUNK_TILES < n_tiles ? t0 + BGO_CHUNK_TILES : n_tiles;
      for (uint32_t t = t0; t < t1; ++t) {
        const uint32_t p = (t << 6) + lane;
        const tile::Window w = tile::window(wp, vp, L, p, (uint32_t)BGO_MAX_K);
        const uint32_t lo = w.lo, v = w.v, off = w.off;  // (off: 5 but at the sequence's start)
        const bool ok = (v >> off) & 1u;  // (beyond the sequence's end: no bit)
        // valid bases from p downwards, p included: what lies before q is shifted in as zero, so the run ends at the
        // sequence's start as well
        const uint32_t run = (uint32_t)__builtin_clz(~(v << (31u - off)) | 1u);  // (off <= 5: bit 0 of the shifted word is free)
        const uint32_t m = ok ? (run - 1u < uK ? run - 1u : uK) : 0u;
        // the (m+1)-mer ending at p, older base more significant: the window's digits off - m .. off, reversed
        const uint32_t e = (lo >> (2u * (off - m))) & ((1u << (2u * (m + 1u))) - 1u);
        const uint32_t y = bgo_reverse_digits(e) >> (32u - 2u * (m + 1u));
        const uint32_t idx = order_table_at((int)m) + y;  // (< order_table_at(K + 1): m <= K, y < 4^(m+1))
        const unsigned long long counting = __ballot(ok);
        if (counting == 0ull) continue;
        const uint32_t lead = (uint32_t)__ffsll((long long)counting) - 1u;  // the first lane that counts, and those with its key
        const uint32_t lead_idx = (uint32_t)__builtin_amdgcn_readlane((int)idx, (int)lead);
        const unsigned long long same = __ballot(ok && idx == lead_idx);
        if (lane == lead)
          atomicAdd(&sh[lead_idx], (uint32_t)__popcll(same));
        else if (ok && idx != lead_idx)
          atomicAdd(&sh[idx], 1u);
      }
    }
  }
  bgo_flush(sh, K, bg);
}

}  // namespace
}  // namespace pengk

using namespace pengk;

extern "C" {

int pengk_bg_count_order(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                         const uint32_t* d_lens, uint64_t n_seq, int K, uint64_t* d_bg) {
  if (!ctx || (n_seq && (!d_words || !d_offs || !d_lens || !d_bg))) return fail(PENGK_ERR_ARG, "pengk_bg_count_order: bad argument");
  if (K < 0 || K > BGO_MAX_K) return fail(PENGK_ERR_ARG, "pengk_bg_count_order: order %d out of range [0,%d]", K, BGO_MAX_K);
  if (n_seq >= (1ull << 32)) return fail(PENGK_ERR_ARG, "pengk_bg_count_order: 2^32 sequences or more; shard the input");
  int rc = enter(ctx);
  if (rc) return rc;
  if (n_seq == 0) return PENGK_OK;
  const size_t lds = (size_t)order_table_at(K + 1) * sizeof(uint32_t);
  const int grid = grid_for(ctx, n_seq, BGO_WAVES, BGO_PER_CU);
  hipLaunchKernelGGL(bg_order_kernel, dim3(grid), dim3(BGO_THREADS), lds, ctx->stream, d_words, d_valid, d_offs, d_lens, n_seq, K,
                     (unsigned long long*)d_bg);
  PENGK_HIP(hipGetLastError());
  return PENGK_OK;
}

}  // extern "C"
