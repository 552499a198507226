// shuffle_core.h -- one sequence of pengk_shuffle_sequences (include/pengk.h, "dinucleotide-preserving shuffle";
// DESIGN.md 16): the body of shuffle_sequences_kernel, written so that a host compiler takes it too
// (tests/tools/shuffle_core_driver.cpp runs it on the CPU against tests/motif_shuffle_model.py).
//
// The whole state of a sequence is its 25 doublet counters cnt[u][v] over the letters 0..4 (4 = not A/C/G/T), uint32
// at c[(5 u + v) * STRIDE]: the kernel keeps them in LDS with STRIDE = the workgroup's size (runtime-indexed, so not in
// registers; bank = thread % 32 whatever the index), the host driver in a plain array with STRIDE = 1.  What is left
// to draw from a letter, rem[u], is the sum of its row, so it is not stored; the last-edge tree is two bit fields.
#ifndef PENGK_SHUFFLE_CORE_H_
#define PENGK_SHUFFLE_CORE_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define PENGK_SHUFFLE_FN __host__ __device__ __forceinline__
#else
#define PENGK_SHUFFLE_FN inline
#endif

namespace pengk {

// draw(c) of the sequence whose global index g is in g32 = g << 32: the high half of splitmix64's finalizer
PENGK_SHUFFLE_FN uint32_t shuffle_draw(uint64_t seed, uint64_t g32, uint64_t c) {
  uint64_t x = seed + 0x9E3779B97F4A7C15ull * (g32 + c);
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return (uint32_t)(x >> 32);
}

// a letter's row of counters; pick draws k in [0, sum) and sel finds the smallest v with c[0] + .. + c[v] > k
struct ShuffleRow {
  uint32_t c0, c1, c2, c3, c4;
  PENGK_SHUFFLE_FN uint32_t sum() const { return c0 + c1 + c2 + c3 + c4; }
  PENGK_SHUFFLE_FN uint32_t sel(uint32_t k) const {
    const uint32_t p0 = c0, p1 = p0 + c1, p2 = p1 + c2, p3 = p2 + c3;
    return (uint32_t)(k >= p0) + (uint32_t)(k >= p1) + (uint32_t)(k >= p2) + (uint32_t)(k >= p3);
  }
  PENGK_SHUFFLE_FN uint32_t at(uint32_t v) const { return v == 0 ? c0 : v == 1 ? c1 : v == 2 ? c2 : v == 3 ? c3 : c4; }
};

template <int STRIDE>
PENGK_SHUFFLE_FN ShuffleRow shuffle_row(const uint32_t* c, uint32_t u) {
  const uint32_t* r = c + u * (5u * STRIDE);
  return ShuffleRow{r[0], r[STRIDE], r[2 * STRIDE], r[3 * STRIDE], r[4 * STRIDE]};
}

PENGK_SHUFFLE_FN uint32_t shuffle_pick(uint32_t r, uint32_t n) { return (uint32_t)(((uint64_t)r * n) >> 32); }

// wp / vp: the sequence's words and validity words (vp = NULL: every base valid), L > 0 its length, g its global index;
// op / ovp: its output words (ovp = NULL: not written).  c: this thread's 25 counters, STRIDE apart.
template <int STRIDE>
PENGK_SHUFFLE_FN void shuffle_sequence(uint64_t seed, uint64_t g, const uint64_t* wp, const uint32_t* vp, uint32_t L,
                                       uint32_t* c, uint64_t* op, uint32_t* ovp) {
  const uint64_t g32 = g << 32;
  const uint32_t nw = (L + 31u) >> 5;
  for (int k = 0; k < 25; ++k) c[k * STRIDE] = 0;
  // doublet counts; s[0] and f = s[L-1]
  uint32_t first = 0, prev = 0;
  for (uint32_t j = 0; j < nw; ++j) {
    uint64_t w = wp[j];
    uint32_t vm = vp ? vp[j] : 0xFFFFFFFFu;
    const uint32_t n = L - 32u * j < 32u ? L - 32u * j : 32u;
    for (uint32_t k = 0; k < n; ++k) {
      const uint32_t a = (vm & 1u) ? (uint32_t)w & 3u : 4u;
      if (j | k) c[(prev * 5u + a) * STRIDE] += 1;
      else first = a;
      prev = a;
      w >>= 2;
      vm >>= 1;
    }
  }
  const uint32_t f = prev;
  // last-edge tree into f (Wilson's loop-erased walk): next[u] in bits [3u, 3u + 3), in_tree one bit per letter
  uint32_t in_tree = 1u << f, next = 0;
  uint64_t t = 0;
  for (uint32_t u0 = 0; u0 < 5; ++u0) {
    if ((in_tree >> u0) & 1u || shuffle_row<STRIDE>(c, u0).sum() == 0) continue;
    uint32_t u = u0;
    while (!((in_tree >> u) & 1u)) {
      const ShuffleRow row = shuffle_row<STRIDE>(c, u);  // (a letter reached here has a successor: its sum is not 0)
      const uint32_t v = row.sel(shuffle_pick(shuffle_draw(seed, g32, 0x80000000ull + t), row.sum()));
      ++t;
      next = (next & ~(7u << (3u * u))) | (v << (3u * u));
      u = v;
    }
    u = u0;
    while (!((in_tree >> u) & 1u)) {
      in_tree |= 1u << u;
      u = (next >> (3u * u)) & 7u;
    }
  }
  // reserve every letter's last edge
  for (uint32_t u = 0; u < 5; ++u)
    if (u != f && shuffle_row<STRIDE>(c, u).sum() != 0) c[(u * 5u + ((next >> (3u * u)) & 7u)) * STRIDE] -= 1;
  // the walk: a letter's other edges without replacement, then its last edge; 32 bases per output word
  uint32_t u = first;
  for (uint32_t j = 0; j < nw; ++j) {
    uint64_t w = 0;
    uint32_t vm = 0;
    const uint32_t n = L - 32u * j < 32u ? L - 32u * j : 32u;
    for (uint32_t k = 0; k < n; ++k) {
      if (j | k) {
        const ShuffleRow row = shuffle_row<STRIDE>(c, u);
        const uint32_t rem = row.sum();
        uint32_t v = (next >> (3u * u)) & 7u;
        if (rem) {
          v = row.sel(shuffle_pick(shuffle_draw(seed, g32, 32u * j + k), rem));
          c[(u * 5u + v) * STRIDE] = row.at(v) - 1u;
        }
        u = v;
      }
      if (u < 4u) {
        w |= (uint64_t)u << (2u * k);
        vm |= 1u << k;
      }
    }
    op[j] = w;
    if (ovp) ovp[j] = vm;
  }
}

}  // namespace pengk

#endif
