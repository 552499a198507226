// stats_order.hip -- the pattern-space sweep under a Markov null of order K <= 5 (pengk_pattern_stats_order,
// --high-order-background): one thread per pattern, as stats_kernel of stats.hip.
//
// Two V tables in LDS: the 84 floats of the run's own model, from which slots o < max_k of bgprob are made exactly as the
// plain sweep makes them (bg_products of stats_common.h), and the orders 0 .. K of the high-order model ((4^(K+2) - 4) / 3
// floats, 21.8 KB at K = 5), from which slot max_k is made: the factor of position i is V_c[x_{i-c} .. x_i], c = min(i, K),
// the products float32 in position order from 1.0f * v0, the reverse complement added in float32 as the plain sweep adds
// it.  Behind that the control policy and pattern_statistics are the plain sweep's.  There is one kernel: the twin tiles of
// stats.hip at W >= 12 are not repeated here, so the option sweep_pairs changes nothing.
#include "pengk_internal.h"
#include "stats_common.h"

namespace pengk {
namespace {

using namespace sweep;

constexpr int SO_MAX_K = 5;

// the order-K probability of pattern x (digits x_0 .. x_{W-1}, x_0 lowest) from the tables sVK
template <int W>
__device__ __forceinline__ float order_product(uint32_t x, const float* __restrict__ sVK, int K) {
  uint32_t word = x & 3u;  // x_{i-c} .. x_i, older base more significant
  float p = 1.0f * sVK[word];
#pragma unroll
  for (int i = 1; i < W; ++i) {
    const int c = i < K ? i : K;
    const uint32_t d = (x >> (2 * i)) & 3u;
    word = ((word << 2) | d) & ((1u << (2 * (c + 1))) - 1u);
    p *= sVK[order_table_at(c) + word];
  }
  return p;
}

template <int W, class... Ctrl>
__global__ __launch_bounds__(256) void stats_order_kernel(int both, int k, int max_k, const float* __restrict__ V, int K,
                                                          const float* __restrict__ VK, const unsigned long long* __restrict__ ltot_p,
                                                          const uint32_t* __restrict__ counts, float* __restrict__ bgprob,
                                                          float* __restrict__ expected, float* __restrict__ logp,
                                                          float* __restrict__ z, const Ctrl... ctrl_arg) {
  __shared__ float sV[84];
  extern __shared__ __attribute__((aligned(16))) float sVK[];  // order_table_at(K + 1) floats
  if (threadIdx.x < 84) sV[threadIdx.x] = V[threadIdx.x];
  const uint32_t nv = order_table_at(K + 1);
  for (uint32_t t = threadIdx.x; t < nv; t += blockDim.x) sVK[t] = VK[t];
  __syncthreads();
  constexpr uint32_t NP = 1u << (2 * W);
  const float fl = (float)(*ltot_p);
  constexpr bool CTRL = sizeof...(Ctrl) != 0;
  [[maybe_unused]] double lc = 0.0;
  if constexpr (CTRL) lc = (double)(*the_control(ctrl_arg...).ltot_p);
  for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < NP; x += gridDim.x * blockDim.x) {
    const uint32_t r = revcomp32(x, W);
    const bool twin = both && r != x;
    float p[3];
    bg_products<W>(x, sV, p[0], p[1], p[2], max_k);
    float pK = order_product<W>(x, sVK, K);
    if (twin) {
      float q[3];
      bg_products<W>(r, sV, q[0], q[1], q[2], max_k);
      p[0] += q[0];
      p[1] += q[1];
      p[2] += q[2];
      pK += order_product<W>(r, sVK, K);
    }
    if (max_k == 0)
      p[0] = pK;
    else if (max_k == 1)
      p[1] = pK;
    else
      p[2] = pK;
    if constexpr (CTRL) {
      const Control& ctrl = the_control(ctrl_arg...);
      const double share = control_share(ctrl.counts[x], ctrl.a, lc);
      p[0] = control_max(p[0], share);
      p[1] = control_max(p[1], share);
      p[2] = control_max(p[2], share);
    }
    bgprob[x] = p[0];
    if (max_k >= 1) bgprob[(size_t)NP + x] = p[1];
    if (max_k >= 2) bgprob[2 * (size_t)NP + x] = p[2];
    const float pk = k == 0 ? p[0] : (k == 1 ? p[1] : p[2]);
    float mu, lp, zz;
    pattern_statistics(pk, fl, counts[x], mu, lp, zz);
    expected[x] = mu;
    logp[x] = lp;
    z[x] = zz;
  }
}

template <int W, class... Ctrl>
int launch_w(pengk_ctx* ctx, int both, int k, int max_k, const float* d_V, int K, const float* d_VK, const uint64_t* d_ltot,
             const uint32_t* d_counts, float* d_bgprob, float* d_expected, float* d_logp, float* d_z, const Ctrl... ctrl) {
  const uint32_t np = 1u << (2 * W);
  const uint32_t need = (np + 255) / 256;
  const uint32_t cap = (uint32_t)ctx->num_cu * 16u;
  hipLaunchKernelGGL((stats_order_kernel<W, Ctrl...>), dim3(need < cap ? need : cap), dim3(256), order_table_at(K + 1) * sizeof(float),
                     ctx->stream, both, k, max_k, d_V, K, d_VK, (const unsigned long long*)d_ltot, d_counts, d_bgprob, d_expected,
                     d_logp, d_z, ctrl...);
  PENGK_HIP(hipGetLastError());
  return PENGK_OK;
}

template <class... Ctrl>
int launch_with(pengk_ctx* ctx, int W, int both, int k, int max_k, const float* d_V, int K, const float* d_VK, const uint64_t* d_ltot,
                const uint32_t* d_counts, float* d_bgprob, float* d_expected, float* d_logp, float* d_z, const Ctrl... ctrl) {
  switch (W) {
    case 2: return launch_w<2>(ctx, both, k, max_k, d_V, K, d_VK, d_ltot, d_counts, d_bgprob, d_expected, d_logp, d_z, ctrl...);
    case 4: return launch_w<4>(ctx, both, k, max_k, d_V, K, d_VK, d_ltot, d_counts, d_bgprob, d_expected, d_logp, d_z, ctrl...);
    case 6: return launch_w<6>(ctx, both, k, max_k, d_V, K, d_VK, d_ltot, d_counts, d_bgprob, d_expected, d_logp, d_z, ctrl...);
    case 8: return launch_w<8>(ctx, both, k, max_k, d_V, K, d_VK, d_ltot, d_counts, d_bgprob, d_expected, d_logp, d_z, ctrl...);
    case 10: return launch_w<10>(ctx, both, k, max_k, d_V, K, d_VK, d_ltot, d_counts, d_bgprob, d_expected, d_logp, d_z, ctrl...);
    case 12: return launch_w<12>(ctx, both, k, max_k, d_V, K, d_VK, d_ltot, d_counts, d_bgprob, d_expected, d_logp, d_z, ctrl...);
    case 14: return launch_w<14>(ctx, both, k, max_k, d_V, K, d_VK, d_ltot, d_counts, d_bgprob, d_expected, d_logp, d_z, ctrl...);
    default: return fail(PENGK_ERR_ARG, "pattern length %d unsupported", W);
  }
}

}  // namespace
}  // namespace pengk

using namespace pengk;

extern "C" {

int pengk_pattern_stats_order(pengk_ctx* ctx, int W, int both, int k, int max_k, const float* d_V, int K, const float* d_VK,
                              const uint64_t* d_ltot, const uint32_t* d_counts, const uint32_t* d_ctrl_counts,
                              const uint64_t* d_ctrl_ltot, double pseudocount, float* d_bgprob, float* d_expected, float* d_logp,
                              float* d_z) {
  if (!ctx || !d_V || !d_VK || !d_ltot || !d_counts || !d_bgprob || !d_expected || !d_logp || !d_z)
    return fail(PENGK_ERR_ARG, "pengk_pattern_stats_order: NULL argument");
  if (!valid_w(W)) return fail(PENGK_ERR_ARG, "pattern length %d unsupported", W);
  if (k < 0 || max_k > 2 || k > max_k || max_k > W - 1) return fail(PENGK_ERR_ARG, "background orders k=%d max_k=%d unsupported", k, max_k);
  if (K < 0 || K > SO_MAX_K) return fail(PENGK_ERR_ARG, "pengk_pattern_stats_order: order %d out of range [0,%d]", K, SO_MAX_K);
  const bool control = d_ctrl_counts || d_ctrl_ltot;
  if (control && (!d_ctrl_counts || !d_ctrl_ltot))
    return fail(PENGK_ERR_ARG, "pengk_pattern_stats_order: a control needs both its counts and its window total");
  if (control ? (!(pseudocount >= 0.0) || pseudocount > 1.7976931348623157e308) : pseudocount != 0.0)
    return fail(PENGK_ERR_ARG, control ? "pengk_pattern_stats_order: pseudocount %g is not a finite number >= 0"
                                       : "pengk_pattern_stats_order: pseudocount %g without a control",
                pseudocount);
  int rc = enter(ctx);
  if (rc) return rc;
  if (control)
    return launch_with(ctx, W, both ? 1 : 0, k, max_k, d_V, K, d_VK, d_ltot, d_counts, d_bgprob, d_expected, d_logp, d_z,
                       Control{d_ctrl_counts, (const unsigned long long*)d_ctrl_ltot, pseudocount});
  return launch_with(ctx, W, both ? 1 : 0, k, max_k, d_V, K, d_VK, d_ltot, d_counts, d_bgprob, d_expected, d_logp, d_z);
}

}  // extern "C"
