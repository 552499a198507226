// tile_walk.h -- what every kernel that gives a WAVE a tile of a sequence shares (dust.hip, dyad.hip, position.hip,
// strata.hip, bg_order.hip; erase.hip takes valid_word): a tile is a run of consecutive positions of one sequence of the
// scan layout, one position (dust: four) per lane.  The validity word, the lane's window of 16 bases, and for the kernels
// that walk tiles in static shares (mask, dyad count, positional count and pair table) the tile counts with their exclusive
// sums, the plan that launches them, a wave's share of the tiles and the cursor it walks them with (the mask takes the plan
// and keeps the share and the walk written out: dust.hip says why).  The tile bodies, the loops over a share, the flushes
// and the LDS layouts are the kernels' own.  DESIGN.md 23.
#pragma once
#include <algorithm>

#include "pengk_internal.h"

namespace pengk {
namespace tile {

constexpr int PLAN_THREADS = 256;  // sequences in a group of the exclusive sums

// validity word j of a sequence of L bases and nw = ceil(L / 32) words under the caller's words vp (NULL: every base
// valid); bits at and beyond L, and words at and beyond nw: 0.  valid_word_in: for a caller whose j is below nw.
__device__ __forceinline__ uint32_t valid_word_in(const uint32_t* vp, uint32_t L, uint32_t j) {
  const uint32_t rem = L - 32u * j;
  const uint32_t in = rem >= 32u ? 0xFFFFFFFFu : ((1u << rem) - 1u);
  return vp ? vp[j] & in : in;
}
__device__ __forceinline__ uint32_t valid_word(const uint32_t* vp, uint32_t L, uint32_t nw, uint32_t j) {
  if (j >= nw) return 0u;
  return valid_word_in(vp, L, j);
}

// The lane's window: the 16 bases (lo, first base lowest) and the 32 validity bits (v) from q = max(p - back, 0) on, and
// the lane's own place in it, off = p - q: `back` but at the sequence's start.  The words are read as halves of 16 bases --
// the window lies in the half of q and the next one --, one funnel shift each; what lies beyond the end reads as 0.
// back is a compile-time or wave-uniform value.
struct Window {
  uint32_t lo, v, off;
};
__device__ __forceinline__ Window window(const uint64_t* wp, const uint32_t* vp, uint32_t L, uint32_t p, uint32_t back) {
  const uint32_t q = p >= back ? p - back : 0u;
  Window w;
  w.off = p < back ? p : back;  // (= p - q: `back` but at the sequence's start)
  const uint32_t* hp = reinterpret_cast<const uint32_t*>(wp);
  const uint32_t nh = (L + 15u) >> 4, h = q >> 4;
  const uint32_t H0 = h < nh ? hp[h] : 0u, H1 = h + 1u < nh ? hp[h + 1u] : 0u;
  w.lo = __builtin_amdgcn_alignbit(H1, H0, (q & 15u) << 1);
  const uint32_t nw = (L + 31u) >> 5, j = q >> 5;
  const uint32_t V0 = valid_word(vp, L, nw, j), V1 = valid_word(vp, L, nw, j + 1u);
  w.v = __builtin_amdgcn_alignbit(V1, V0, q & 31u);
  return w;
}

// ---- tile counts and their exclusive sums -----------------------------------------------------------------------------
// tiles_of(L): a record of the tiles of a sequence of L bases whose member nt is their number (Tiles, or a kernel's own).
struct Tiles {
  uint32_t nt;
};
struct NoEach {
  __device__ __forceinline__ void operator()(uint64_t) const {}
};

__device__ __forceinline__ unsigned long long group_inclusive_sum(unsigned long long v, unsigned long long* sh) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int d = 1; d < PLAN_THREADS; d <<= 1) {
    const unsigned long long x = t >= d ? sh[t - d] : 0ull;
    __syncthreads();
    sh[t] += x;
    __syncthreads();
  }
  const unsigned long long r = sh[t];
  __syncthreads();
  return r;
}

// excl[i]: the tiles of the sequences in front of i within its group of 256; boff[b]: the tiles of group b; each(i) once
// per sequence for what an entry keeps beside them
template <class TilesOf, class Each>
__global__ __launch_bounds__(PLAN_THREADS) void tiles_kernel(const uint32_t* __restrict__ lens, uint64_t n_seq, TilesOf tiles_of,
                                                             unsigned long long* __restrict__ excl,
                                                             unsigned long long* __restrict__ boff, Each each) {
  __shared__ unsigned long long sh[PLAN_THREADS];
  const uint64_t i = (uint64_t)blockIdx.x * PLAN_THREADS + threadIdx.x;
  const unsigned long long nt = i < n_seq ? tiles_of(lens[i]).nt : 0u;
  const unsigned long long incl = group_inclusive_sum(nt, sh);
  if (i < n_seq) {
    excl[i] = incl - nt;
    each(i);
  }
  if (threadIdx.x == PLAN_THREADS - 1) boff[blockIdx.x] = incl;
}

// boff[0 .. n_groups) -> exclusive sums in place, boff[n_groups] = the total; one workgroup (a template only so that a
// translation unit that plans no walk holds no copy of it)
template <class = void>
__global__ __launch_bounds__(PLAN_THREADS) void groups_kernel(unsigned long long* __restrict__ boff, uint64_t n_groups) {
  __shared__ unsigned long long sh[PLAN_THREADS];
  unsigned long long carry = 0;
  for (uint64_t b = 0; b < n_groups; b += PLAN_THREADS) {
    const uint64_t k = b + threadIdx.x;
    const unsigned long long v = k < n_groups ? boff[k] : 0ull;
    const unsigned long long incl = group_inclusive_sum(v, sh);
    if (k < n_groups) boff[k] = carry + incl - v;
    sh[threadIdx.x] = incl;  // (the last thread's is the chunk's total)
    __syncthreads();
    carry += sh[PLAN_THREADS - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) boff[n_groups] = carry;
}

// ---- the plan on the host ---------------------------------------------------------------------------------------------
// scratch = excl (n_seq uint64) | boff (n_groups + 1 uint64), plan_bytes(n_seq) in all; the two launches on the context's
// stream.  Checks nothing: the entry has checked its arguments, entered the context and sized the scratch (n_seq >= 1).
struct Plan {
  unsigned long long *excl, *boff;
  uint64_t n_groups;
};
inline uint64_t groups_of(uint64_t n_seq) { return (n_seq + PLAN_THREADS - 1) / PLAN_THREADS; }
inline size_t plan_bytes(uint64_t n_seq) { return (n_seq + groups_of(n_seq) + 1) * sizeof(uint64_t); }

template <class TilesOf, class Each = NoEach>
inline Plan plan(pengk_ctx* ctx, void* scratch, const uint32_t* d_lens, uint64_t n_seq, TilesOf tiles_of, Each each = Each{}) {
  Plan p;
  p.n_groups = groups_of(n_seq);
  p.excl = (unsigned long long*)scratch;
  p.boff = p.excl + n_seq;
  hipLaunchKernelGGL((tiles_kernel<TilesOf, Each>), dim3((unsigned)p.n_groups), dim3(PLAN_THREADS), 0, ctx->stream, d_lens, n_seq, tiles_of,
                     p.excl, p.boff, each);
  hipLaunchKernelGGL(groups_kernel<>, dim3(1), dim3(PLAN_THREADS), 0, ctx->stream, p.boff, p.n_groups);
  return p;
}

// ---- a wave's share of the tiles and its cursor -------------------------------------------------------------------------
// Every wave of a fixed grid of workgroups of WAVES waves takes one contiguous share [g, gend) of the tiles, `per` of them
// but for the last that has any.  Static: nothing is handed out at run time, and per is the same for the whole grid, so a
// loop of per rounds has its barriers in workgroup-uniform control flow.  block_empty: the share of the workgroup's first
// wave is empty, and so are those of its others.
struct Share {
  uint64_t per, g, gend;
  bool block_empty;
};
template <int WAVES>
__device__ __forceinline__ Share share(const unsigned long long* __restrict__ boff, uint64_t n_groups) {
  const uint64_t total = boff[n_groups];
  const uint64_t n_waves = (uint64_t)gridDim.x * WAVES;
  const uint64_t per = (total + n_waves - 1) / n_waves;
  const uint64_t wave = (uint64_t)blockIdx.x * WAVES + (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t g = wave * per;
  return Share{per, g, g + per < total ? g + per : total, (uint64_t)blockIdx.x * WAVES * per >= total};
}

// Where a wave stands: tile k of sequence i, of L bases and the tiles t.  A walk is locate(g) at the first tile of a
// non-empty share, then for every tile of it next(), the tile's work, ++k.
template <class TilesOf>
struct Cursor {
  const uint32_t* __restrict__ lens;
  uint64_t n_seq;
  TilesOf tiles_of;
  uint64_t i = 0;
  uint32_t k = 0, L = 0;
  decltype(tiles_of(0u)) t = {};

  // the sequence and the tile of it that g < total is: the last group with boff <= g, the last sequence of it with
  // excl <= rest (a sequence without tiles shares its excl with the next one: the last one is the one that has g)
  __device__ __forceinline__ void locate(uint64_t g, const unsigned long long* __restrict__ excl,
                                         const unsigned long long* __restrict__ boff, uint64_t n_groups) {
    uint64_t lo = 0, hi = n_groups;  // boff[lo] <= g < boff[hi]
    while (hi - lo > 1) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (boff[mid] <= g) lo = mid;
      else hi = mid;
    }
    const uint64_t rest = g - boff[lo];
    i = lo * PLAN_THREADS;
    uint64_t ihi = std::min<uint64_t>(n_seq, i + PLAN_THREADS);
    while (ihi - i > 1) {
      const uint64_t mid = i + (ihi - i) / 2;
      if (excl[mid] <= rest) i = mid;
      else ihi = mid;
    }
    k = (uint32_t)(rest - excl[i]);
    L = lens[i];
    t = tiles_of(L);
  }
  // the next sequence: false where there is none
  __device__ __forceinline__ bool step() {
    if (++i >= n_seq) return false;
    L = lens[i];
    t = tiles_of(L);
    k = 0;
    return true;
  }
  // the next sequence that has a tile, where the current one has no tile k (inside a share there is one); false: none.
  // The first step stands outside the loop: it is the one nearly every call takes, and there its load of lens is scalar.
  __device__ __forceinline__ bool next() {
    if (k < t.nt) return true;
    if (!step()) return false;
    while (t.nt == 0)
      if (!step()) return false;
    return true;
  }
};

}  // namespace tile
}  // namespace pengk
