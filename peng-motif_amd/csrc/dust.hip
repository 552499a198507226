// dust.hip -- masking low-complexity stretches on the device (--mask-low-complexity): this project's
// statement of the symmetric DUST criterion, defined in include/pengk.h ("masking low-complexity stretches").
//
//   tile     256 consecutive bases of one sequence, one wave: lane j owns the DUST_K = 4 starts 4j .. 4j+3 of the tile in
//            registers.  The tile's first 64 bases (not in a sequence's first tile) are the left halo of the cover's running
//            maximum, its last 64 starts the right halo of the recurrence: a tile writes the validity words of 128 bases
//            (192 in a sequence's first tile, everything to the end in its last), always whole 32-base words, so no word
//            has two writers.  A sequence of up to 256 bases is one tile.
//   step     l = 2 .. 62: c(i,l) = c(i+1,l-1) + [t[i] == t[i+l-1]], num += c, and the largest score inside, M, as a
//            fraction; the shift by one start is a register rename inside a lane and one ds_bpermute (c, M packed into
//            one word) at the lane's last slot.  No table of triplet counters, no LDS array, no barrier.
//   cover    end(i) = i + lmax(i) + 2; base b is covered iff the running maximum of end over the starts <= b exceeds b
//            (a wave prefix maximum: six shuffles).
//   tiles    tile counts per sequence -> exclusive sums (the plan of tile_walk.h), then every wave of a fixed grid takes
//            one contiguous share of the tiles: a binary search for its first tile, then a walk.  Static: nothing is
//            handed out at run time.  The walk is written out here and not tile_walk.h's cursor: under the cursor this
//            kernel measured 1.7 % slower (profiles/tile_walk_probe.log), though its step loop compiles the same.
// What lies beyond the right halo is wrong by construction and flows only into starts whose results are not used:
// (i, l) reads (i+1, l-1) and nothing else of another start.  Registers only: no address depends on such a value.
#include <algorithm>

#include "pengk_internal.h"
#include "scan_walk.h"
#include "tile_walk.h"

namespace pengk {
namespace {

constexpr int DUST_THREADS = 256;
constexpr int DUST_WAVES = DUST_THREADS / 64;
constexpr int DUST_K = 4;                       // starts per lane
constexpr uint32_t DUST_TILE = 64 * DUST_K;     // starts (= bases) per tile
constexpr uint32_t DUST_HALO = PENGK_DUST_WINDOW;  // bases in front of a tile's first written word (a multiple of 32)
constexpr uint32_t DUST_FIRST = DUST_TILE - 64; // bases the first tile of a longer sequence writes (right halo 61 -> 64)
constexpr uint32_t DUST_STEP = DUST_TILE - 64 - DUST_HALO;  // ... and every later one
constexpr uint32_t DUST_MAX_L = PENGK_DUST_WINDOW - 2;
static_assert(DUST_K == 4 && DUST_HALO % 32 == 0 && DUST_STEP % 32 == 0 && DUST_FIRST % 32 == 0, "tiles write whole words");

// tiles of a sequence of L bases: tile 0 holds the bases [0, 256), tile k >= 1 the bases [128 k, 128 k + 256)
__host__ __device__ __forceinline__ uint32_t dust_tiles(uint32_t L) {
  if (L == 0) return 0;
  if (L <= DUST_TILE) return 1;
  const uint32_t two = DUST_FIRST - DUST_HALO + DUST_TILE;  // what two tiles reach: 384
  return 2u + ((L > two ? L - two : 0u) + DUST_STEP - 1u) / DUST_STEP;
}

struct DustTilesOf {
  __device__ __forceinline__ tile::Tiles operator()(uint32_t L) const { return tile::Tiles{dust_tiles(L)}; }
};
// beside the tile counts: flag[i] = 0
struct DustClearFlag {
  uint32_t* flag;
  __device__ __forceinline__ void operator()(uint64_t i) const { flag[i] = 0u; }
};

// ---- the mask ---------------------------------------------------------------------------------------------------------
// One tile: the bases [s0, s0 + 256) of a sequence of L bases whose words / validity words begin at wp / vp (vp NULL:
// every base valid); writes the words that hold the bases [o0, o1) (o0 a multiple of 32, o1 one or L) to op.
// Returns (in every lane) the bits this lane's stores cleared.
__device__ __forceinline__ uint32_t dust_tile(const uint64_t* __restrict__ wp, const uint32_t* __restrict__ vp, uint32_t L,
                                              uint64_t s0, uint64_t o0, uint64_t o1, uint32_t T, uint32_t* __restrict__ op) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t nw = (L + 31u) >> 5;
  const uint64_t b0 = s0 + DUST_K * lane;          // this lane's first start (may lie beyond the end: nothing stands there)
  const uint64_t k0 = b0 >> 5;                     // ... its word
  const uint32_t s = (uint32_t)b0 & 31u;           // ... and its place in it (a multiple of 4, <= 28)
  // bases b0 .. b0+95 as A0 | A1 | A2 (b0+66 is the last one read: inside the three words from k0 on) and the validity
  // bits of b0 .. b0+63 (v) and b0+64 .. (vh)
  uint64_t W[3];
  uint32_t V[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const bool in = k0 + q < nw;
    W[q] = in ? wp[k0 + q] : 0ull;
    V[q] = in ? tile::valid_word(vp, L, nw, (uint32_t)(k0 + q)) : 0u;
  }
  uint64_t A0 = W[0], A1 = W[1], A2 = W[2];
  const uint64_t vlo = (uint64_t)V[0] | ((uint64_t)V[1] << 32);
  uint64_t v = vlo;
  if (s) {
    A0 = (W[0] >> (2u * s)) | (W[1] << (64u - 2u * s));
    A1 = (W[1] >> (2u * s)) | (W[2] << (64u - 2u * s));
    A2 = W[2] >> (2u * s);
    v = (vlo >> s) | ((uint64_t)V[2] << (64u - s));
  }
  const uint64_t vh = (uint64_t)(V[2] >> s);
  // standing triplets from b0 on: bit m = the triplet at b0 + m (m <= 64), and every slot's run of them (<= 62)
  const uint64_t st = v & ((v >> 1) | (vh << 63)) & ((v >> 2) | (vh << 62));
  const uint64_t st64 = (vh & 7u) == 7u ? 1ull : 0ull;
  uint32_t ti[DUST_K], run[DUST_K], c[DUST_K], num[DUST_K], Mn[DUST_K], Md[DUST_K], lm[DUST_K];
#pragma unroll
  for (int k = 0; k < DUST_K; ++k) {
    const uint64_t sk = k ? (st >> k) | (st64 << (64 - k)) : st;
    const uint32_t r = (uint32_t)__builtin_ctzll(~sk | (1ull << 63));
    run[k] = r < DUST_MAX_L ? r : DUST_MAX_L;
    ti[k] = (uint32_t)(A0 >> (2 * k)) & 63u;
    c[k] = num[k] = Mn[k] = lm[k] = 0u;
    Md[k] = 1u;
  }
  for (uint32_t l = 2; l <= DUST_MAX_L; ++l) {
    const uint32_t d = l - 1u, Td10 = T * d / 10u;  // 10 num > T d iff num > floor(T d / 10)
    A0 = (A0 >> 2) | (A1 << 62);  // the bases from b0 + l - 1 on
    A1 = (A1 >> 2) | (A2 << 62);
    A2 >>= 2;
    // (i+1, l-1) of the lane's last slot: the next lane's slot 0 as it stands (lane 63 reads its own: beyond the right halo)
    const uint32_t pk = __shfl_down(c[0] | (Mn[0] << 6) | (Md[0] << 17), 1);
    const uint32_t a0 = (uint32_t)A0;
#pragma unroll
    for (int k = 0; k < DUST_K; ++k) {
      const uint32_t cin = k + 1 < DUST_K ? c[(k + 1) % DUST_K] : pk & 63u;
      const uint32_t nn = k + 1 < DUST_K ? Mn[(k + 1) % DUST_K] : (pk >> 6) & 2047u;
      const uint32_t nd = k + 1 < DUST_K ? Md[(k + 1) % DUST_K] : pk >> 17;
      const uint32_t cn = cin + (ti[k] == __builtin_amdgcn_ubfe(a0, 2 * k, 6) ? 1u : 0u);
      const uint32_t n = num[k] + cn;
      const uint32_t on = Mn[k], od = Md[k];
      // the larger of the two M's first: S >= both iff S >= the larger (four products a start and step, not six)
      const bool nb = __umul24(nn, od) > __umul24(on, nd);
      const uint32_t bn = nb ? nn : on, bd = nb ? nd : od;
      const bool ge = __umul24(n, bd) >= __umul24(bn, d);
      const bool perfect = ge & (n > Td10) & (run[k] >= l);
      lm[k] = perfect ? l : lm[k];
      c[k] = cn;
      num[k] = n;
      Mn[k] = ge ? n : bn;
      Md[k] = ge ? d : bd;
    }
  }
  // end(i) relative to s0, its running maximum over the tile's starts, the cover bits of this lane's four bases
  uint32_t p[DUST_K];
#pragma unroll
  for (int k = 0; k < DUST_K; ++k) {
    const uint32_t e = lm[k] ? DUST_K * lane + k + lm[k] + 2u : 0u;
    p[k] = k ? (e > p[(k + DUST_K - 1) % DUST_K] ? e : p[(k + DUST_K - 1) % DUST_K]) : e;
  }
  uint32_t incl = p[DUST_K - 1];
#pragma unroll
  for (int dlt = 1; dlt < 64; dlt <<= 1) {
    const uint32_t x = __shfl_up(incl, dlt);
    if (lane >= (uint32_t)dlt && x > incl) incl = x;
  }
  uint32_t before = __shfl_up(incl, 1);
  if (lane == 0) before = 0u;
  uint32_t cov = 0u;
#pragma unroll
  for (int k = 0; k < DUST_K; ++k) {
    const uint32_t m = p[k] > before ? p[k] : before;
    if (m > DUST_K * lane + k) cov |= 1u << k;
  }
  // eight lanes' nibbles -> one word, in the lane with (lane & 7) == 0
  uint32_t word = cov << (4u * (lane & 7u));
  word |= __shfl_xor(word, 1);
  word |= __shfl_xor(word, 2);
  word |= __shfl_xor(word, 4);
  uint32_t cleared = 0u;
  const uint64_t kw = (s0 >> 5) + (lane >> 3);  // the sequence's word this lane group holds
  if ((lane & 7u) == 0u && 32ull * kw >= o0 && 32ull * kw < o1) {
    const uint32_t in = tile::valid_word(vp, L, nw, (uint32_t)kw);
    op[kw] = in & ~word;
    cleared = (uint32_t)__popc(in & word);
  }
  return cleared;
}

__global__ __launch_bounds__(DUST_THREADS) void dust_mask_kernel(const uint64_t* __restrict__ words,
                                                                 const uint32_t* __restrict__ valid,
                                                                 const int64_t* __restrict__ offs,
                                                                 const uint32_t* __restrict__ lens, uint64_t n_seq, uint32_t T,
                                                                 const unsigned long long* __restrict__ excl,
                                                                 const unsigned long long* __restrict__ boff, uint64_t n_groups,
                                                                 uint32_t* __restrict__ flag, uint32_t* __restrict__ out,
                                                                 unsigned long long* __restrict__ masked) {
  __shared__ unsigned long long bsum;
  if (threadIdx.x == 0) bsum = 0;
  __syncthreads();
  // this wave's share of the tiles: [g, g1) (what tile::share and tile::Cursor do, written out: see the header comment)
  const uint64_t total = boff[n_groups];
  const uint64_t n_waves = (uint64_t)gridDim.x * DUST_WAVES;
  const uint64_t wave = (uint64_t)blockIdx.x * DUST_WAVES + (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t per = (total + n_waves - 1) / n_waves;
  uint64_t g = wave * per;
  const uint64_t g1 = g + per < total ? g + per : total;
  unsigned long long mine = 0;
  if (g < g1) {
    // the sequence and the tile of it that g is: the last group with boff <= g, the last sequence of it with excl <= rest
    uint64_t lo = 0, hi = n_groups;  // boff[lo] <= g < boff[hi]
    while (hi - lo > 1) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (boff[mid] <= g) lo = mid;
      else hi = mid;
    }
    const uint64_t rest = g - boff[lo];
    uint64_t i = lo * tile::PLAN_THREADS, ihi = std::min<uint64_t>(n_seq, i + tile::PLAN_THREADS);
    while (ihi - i > 1) {
      const uint64_t mid = i + (ihi - i) / 2;
      if (excl[mid] <= rest) i = mid;
      else ihi = mid;
    }
    uint32_t k = (uint32_t)(rest - excl[i]);
    uint32_t L = lens[i], nt = dust_tiles(L);
    for (; g < g1; ++g) {
      while (k >= nt) {  // the next sequence that has a tile (there is one: g < total)
        if (++i >= n_seq) break;
        L = lens[i];
        nt = dust_tiles(L);
        k = 0;
      }
      if (i >= n_seq) break;
      const uint64_t w0 = (uint64_t)offs[i] >> 5;
      const uint64_t s0 = (uint64_t)k * DUST_STEP;
      const uint64_t o0 = k ? s0 + DUST_HALO : 0;
      const uint64_t o1 = s0 + DUST_TILE >= L ? L : o0 + (k ? DUST_STEP : DUST_FIRST);
      const uint32_t cleared = dust_tile(words + w0, valid ? valid + w0 : nullptr, L, s0, o0, o1, T, out + w0);
      if (cleared) {
        flag[i] = 1u;  // (every writer stores the same value)
        mine += cleared;
      }
      ++k;
    }
  }
  if (mine) atomicAdd(&bsum, mine);
  __syncthreads();
  if (threadIdx.x == 0 && bsum) atomicAdd(masked, bsum);
}

// the sequences that lost a base: the sum of flag, one atomic per workgroup at most
__global__ __launch_bounds__(DUST_THREADS) void dust_touched_kernel(const uint32_t* __restrict__ flag, uint64_t n_seq,
                                                                    unsigned long long* __restrict__ touched) {
  __shared__ unsigned long long bsum;
  if (threadIdx.x == 0) bsum = 0;
  __syncthreads();
  unsigned long long mine = 0;
  for (uint64_t i = blockIdx.x * (uint64_t)DUST_THREADS + threadIdx.x; i < n_seq; i += (uint64_t)gridDim.x * DUST_THREADS)
    mine += flag[i];
  if (mine) atomicAdd(&bsum, mine);
  __syncthreads();
  if (threadIdx.x == 0 && bsum) atomicAdd(touched, bsum);
}

}  // namespace
}  // namespace pengk

using namespace pengk;

extern "C" {

int pengk_mask_low_complexity(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                              const uint32_t* d_lens, uint64_t n_seq, int threshold, uint32_t* d_out_valid, uint64_t* d_masked) {
  if (!ctx || (n_seq && (!d_words || !d_offs || !d_lens || !d_out_valid || !d_masked)))
    return fail(PENGK_ERR_ARG, "pengk_mask_low_complexity: bad argument");
  if (threshold < 1 || threshold > 1000)
    return fail(PENGK_ERR_ARG, "pengk_mask_low_complexity: threshold %d out of range [1,1000]", threshold);
  if (n_seq >> 32) return fail(PENGK_ERR_ARG, "pengk_mask_low_complexity: 2^32 sequences or more; shard the input");
  if (n_seq && d_out_valid == d_valid)
    return fail(PENGK_ERR_ARG, "pengk_mask_low_complexity: the output buffer must differ from the input");
  int rc = enter(ctx);
  if (rc) return rc;
  if (n_seq == 0) return PENGK_OK;
  // scratch: excl | boff (tile_walk.h) | flag (n_seq uint32)
  rc = ensure_scratch(ctx, &ctx->d_sites, &ctx->sites_bytes, tile::plan_bytes(n_seq) + n_seq * sizeof(uint32_t));
  if (rc) return rc;
  uint32_t* flag = (uint32_t*)((char*)ctx->d_sites + tile::plan_bytes(n_seq));
  unsigned long long* masked = (unsigned long long*)d_masked;
  const tile::Plan plan = tile::plan(ctx, ctx->d_sites, d_lens, n_seq, DustTilesOf{}, DustClearFlag{flag});
  hipLaunchKernelGGL(dust_mask_kernel, dim3((unsigned)ctx->num_cu * 8u), dim3(DUST_THREADS), 0, ctx->stream, d_words, d_valid, d_offs,
                     d_lens, n_seq, (uint32_t)threshold, plan.excl, plan.boff, plan.n_groups, flag, d_out_valid, masked);
  hipLaunchKernelGGL(dust_touched_kernel, dim3(grid_for(ctx, n_seq, DUST_THREADS, 16)), dim3(DUST_THREADS), 0, ctx->stream, flag,
                     n_seq, masked + 1);
  PENGK_HIP(hipGetLastError());
  return PENGK_OK;
}

}  // extern "C"
