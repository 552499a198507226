// stats_common.h -- what the pattern-space sweeps share (stats.hip, stats_strata.hip): the Markov products of one pattern
// from a V table in LDS, the statistics of one pattern from its aggregated probability and its count, and the control
// policy (the second null of pengk_pattern_stats_control).  Float semantics: the header of stats.hip.
#pragma once
#include "pengk_internal.h"

namespace pengk {
namespace sweep {

template <int W>
__device__ __forceinline__ void bg_products(uint32_t x, const float* __restrict__ sV, float& p0, float& p1, float& p2,
                                            int max_k) {
  // digits x_0..x_{W-1}; BaMM ids are big-endian: (x_{i-2} x_{i-1} x_i)
  const uint32_t d0 = x & 3u;
  const float v0 = sV[d0];
  p0 = 1.0f * v0;
  p1 = p0;
  p2 = p0;
  uint32_t prev1 = d0;  // x_{i-1}
  uint32_t prev2 = 0;   // x_{i-2}
#pragma unroll
  for (int i = 1; i < W; ++i) {
    const uint32_t d = (x >> (2 * i)) & 3u;
    p0 *= sV[d];
    const float v1 = sV[4 + ((prev1 << 2) | d)];
    if (max_k >= 1) p1 *= v1;
    if (max_k >= 2) {
      if (i == 1)
        p2 *= v1;  // order-1 factor while only one base of context exists
      else
        p2 *= sV[20 + ((prev2 << 4) | (prev1 << 2) | d)];
    }
    prev2 = prev1;
    prev1 = d;
  }
}

// What the sweep leaves for one pattern from its aggregated probabilities and its count: expected, log-p, z
// (src/base_pattern.cpp:231-265; float / double semantics: the header of stats.hip).
__device__ __forceinline__ void pattern_statistics(float pk, float fl, uint32_t n, float& mu, float& lp, float& zz) {
  mu = pk * fl;
  if (n == 0) {
    lp = __builtin_inff();
  } else {
    const float fn = (float)n;
    const float frac = (float)(1.0 - (double)(mu / (float)((unsigned long long)n + 1ull)));  // (the reference adds the 1 to a size_t: n = 2^32 - 1 must not wrap)
    if (fn > mu && n > 5u) {
      const double dn = (double)n;
      lp = (float)(dn * log((double)(mu / fn)) + dn - (double)mu - 0.5 * log(6.283 * dn * (double)frac * (double)frac));
    } else {
      lp = 0.0f;
    }
  }
  zz = (float)((double)((float)n - mu) / sqrt((double)mu));
}

// The second null (pengk_pattern_stats_control): a control set's own counts.  Every order's aggregated
// probability p_o[x] is raised to the control's share of the pattern, q_o[x] = (float)fmax((double)p_o[x], (c[x] + a) / Lc)
// -- sum and quotient in fp64, ONE rounding to float32 -- and everything downstream (bgprob, expected, log-p, z) is made
// of q.  The quotient does not depend on the order: one fp64 division per pattern.  Lc == 0 (an empty control): q = p.
// The kernels take the control as an OPTIONAL last argument (a parameter pack of none or one): without it they have the
// signature and the code they had -- same instructions, same registers, same LDS.
struct Control {
  const uint32_t* __restrict__ counts;
  const unsigned long long* __restrict__ ltot_p;
  double a;
};

__device__ __forceinline__ double control_share(uint32_t c, double a, double lc) {
  return lc == 0.0 ? -__builtin_inf() : ((double)c + a) / lc;
}
__device__ __forceinline__ float control_max(float p, double share) { return (float)fmax((double)p, share); }
__device__ __forceinline__ const Control& the_control(const Control& c) { return c; }

}  // namespace sweep
}  // namespace pengk
