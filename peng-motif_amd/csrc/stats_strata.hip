// stats_strata.hip -- the pattern-space sweep under a GC-stratified null (pengk_pattern_stats_strata,
// --stratified-background): one thread per pattern, as stats_kernel of stats.hip.
//
// The strata with a window (at most 16) bring a V table each: 84 floats a stratum in LDS, 5.4 KB at most.  A thread takes
// its pattern through every stratum in ascending order -- the Markov products of stats_common.h, the reverse complement
// added in float32 exactly as the plain sweep adds it -- and accumulates w_s * p_{s,o} in fp64, one multiplication and one
// addition (no fused multiply-add: -ffp-contract=off), then divides once by the sum of the weights and rounds once to
// float32.  The weights come by value with the launch (host integers turned into doubles on the host): the call does not
// wait for the stream.  Behind the mixture the control policy and pattern_statistics are the plain sweep's.
// S times the plain sweep's arithmetic at the same bytes: DESIGN.md 27 has the measured ratio.
#include "pengk_internal.h"
#include "stats_common.h"

namespace pengk {
namespace {

using namespace sweep;

struct Mixture {
  int n;           // strata with a window, 1 .. 16
  int row[16];     // their rows of V, ascending
  double w[16];    // (double)w_s
  double total;    // (double)(sum of all w_s)
};

template <int W, class... Ctrl>
__global__ __launch_bounds__(256) void stats_strata_kernel(int both, int k, int max_k, const float* __restrict__ V, const Mixture mix,
                                                           const unsigned long long* __restrict__ ltot_p,
                                                           const uint32_t* __restrict__ counts, float* __restrict__ bgprob,
                                                           float* __restrict__ expected, float* __restrict__ logp,
                                                           float* __restrict__ z, const Ctrl... ctrl_arg) {
  __shared__ float sV[16 * 84];
  for (int t = threadIdx.x; t < mix.n * 84; t += blockDim.x) sV[t] = V[mix.row[t / 84] * 84 + t % 84];
  __syncthreads();
  constexpr uint32_t NP = 1u << (2 * W);
  const float fl = (float)(*ltot_p);
  constexpr bool CTRL = sizeof...(Ctrl) != 0;
  [[maybe_unused]] double lc = 0.0;
  if constexpr (CTRL) lc = (double)(*the_control(ctrl_arg...).ltot_p);
  for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < NP; x += gridDim.x * blockDim.x) {
    const uint32_t r = revcomp32(x, W);
    const bool twin = both && r != x;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int j = 0; j < mix.n; ++j) {
      const float* v = sV + j * 84;
      float p[3];
      bg_products<W>(x, v, p[0], p[1], p[2], max_k);
      if (twin) {
        float q[3];
        bg_products<W>(r, v, q[0], q[1], q[2], max_k);
        p[0] += q[0];
        p[1] += q[1];
        p[2] += q[2];
      }
      const double w = mix.w[j];
      acc[0] += w * (double)p[0];
      acc[1] += w * (double)p[1];
      acc[2] += w * (double)p[2];
    }
    float m[3];
    m[0] = (float)(acc[0] / mix.total);
    m[1] = (float)(acc[1] / mix.total);
    m[2] = (float)(acc[2] / mix.total);
    if constexpr (CTRL) {
      const Control& ctrl = the_control(ctrl_arg...);
      const double share = control_share(ctrl.counts[x], ctrl.a, lc);
      m[0] = control_max(m[0], share);
      m[1] = control_max(m[1], share);
      m[2] = control_max(m[2], share);
    }
    bgprob[x] = m[0];
    if (max_k >= 1) bgprob[(size_t)NP + x] = m[1];
    if (max_k >= 2) bgprob[2 * (size_t)NP + x] = m[2];
    const float pk = k == 0 ? m[0] : (k == 1 ? m[1] : m[2]);
    float mu, lp, zz;
    pattern_statistics(pk, fl, counts[x], mu, lp, zz);
    expected[x] = mu;
    logp[x] = lp;
    z[x] = zz;
  }
}

template <int W, class... Ctrl>
int launch_w(pengk_ctx* ctx, int both, int k, int max_k, const float* d_V, const Mixture& mix, const uint64_t* d_ltot,
             const uint32_t* d_counts, float* d_bgprob, float* d_expected, float* d_logp, float* d_z, const Ctrl... ctrl) {
  const uint32_t np = 1u << (2 * W);
  const uint32_t need = (np + 255) / 256;
  const uint32_t cap = (uint32_t)ctx->num_cu * 16u;
  hipLaunchKernelGGL((stats_strata_kernel<W, Ctrl...>), dim3(need < cap ? need : cap), dim3(256), 0, ctx->stream, both, k, max_k, d_V,
                     mix, (const unsigned long long*)d_ltot, d_counts, d_bgprob, d_expected, d_logp, d_z, ctrl...);
  PENGK_HIP(hipGetLastError());
  return PENGK_OK;
}

template <class... Ctrl>
int launch_with(pengk_ctx* ctx, int W, int both, int k, int max_k, const float* d_V, const Mixture& mix, const uint64_t* d_ltot,
                const uint32_t* d_counts, float* d_bgprob, float* d_expected, float* d_logp, float* d_z, const Ctrl... ctrl) {
  switch (W) {
    case 2: return launch_w<2>(ctx, both, k, max_k, d_V, mix, d_ltot, d_counts, d_bgprob, d_expected, d_logp, d_z, ctrl...);
    case 4: return launch_w<4>(ctx, both, k, max_k, d_V, mix, d_ltot, d_counts, d_bgprob, d_expected, d_logp, d_z, ctrl...);
    case 6: return launch_w<6>(ctx, both, k, max_k, d_V, mix, d_ltot, d_counts, d_bgprob, d_expected, d_logp, d_z, ctrl...);
    case 8: return launch_w<8>(ctx, both, k, max_k, d_V, mix, d_ltot, d_counts, d_bgprob, d_expected, d_logp, d_z, ctrl...);
    case 10: return launch_w<10>(ctx, both, k, max_k, d_V, mix, d_ltot, d_counts, d_bgprob, d_expected, d_logp, d_z, ctrl...);
    case 12: return launch_w<12>(ctx, both, k, max_k, d_V, mix, d_ltot, d_counts, d_bgprob, d_expected, d_logp, d_z, ctrl...);
    case 14: return launch_w<14>(ctx, both, k, max_k, d_V, mix, d_ltot, d_counts, d_bgprob, d_expected, d_logp, d_z, ctrl...);
    default: return fail(PENGK_ERR_ARG, "pattern length %d unsupported", W);
  }
}

}  // namespace
}  // namespace pengk

using namespace pengk;

extern "C" {

int pengk_pattern_stats_strata(pengk_ctx* ctx, int W, int both, int k, int max_k, const float* d_V, int n_strata,
                               const uint64_t* h_windows, const uint64_t* d_ltot, const uint32_t* d_counts,
                               const uint32_t* d_ctrl_counts, const uint64_t* d_ctrl_ltot, double pseudocount, float* d_bgprob,
                               float* d_expected, float* d_logp, float* d_z) {
  if (!ctx || !d_V || !h_windows || !d_ltot || !d_counts || !d_bgprob || !d_expected || !d_logp || !d_z)
    return fail(PENGK_ERR_ARG, "pengk_pattern_stats_strata: NULL argument");
  if (!valid_w(W)) return fail(PENGK_ERR_ARG, "pattern length %d unsupported", W);
  if (k < 0 || max_k > 2 || k > max_k || max_k > W - 1) return fail(PENGK_ERR_ARG, "background orders k=%d max_k=%d unsupported", k, max_k);
  if (n_strata < 1 || n_strata > 16) return fail(PENGK_ERR_ARG, "pengk_pattern_stats_strata: n_strata %d out of range [1,16]", n_strata);
  const bool control = d_ctrl_counts || d_ctrl_ltot;
  if (control && (!d_ctrl_counts || !d_ctrl_ltot))
    return fail(PENGK_ERR_ARG, "pengk_pattern_stats_strata: a control needs both its counts and its window total");
  if (control ? (!(pseudocount >= 0.0) || pseudocount > 1.7976931348623157e308) : pseudocount != 0.0)
    return fail(PENGK_ERR_ARG, control ? "pengk_pattern_stats_strata: pseudocount %g is not a finite number >= 0"
                                       : "pengk_pattern_stats_strata: pseudocount %g without a control",
                pseudocount);
  Mixture mix = {};
  uint64_t total = 0;
  for (int s = 0; s < n_strata; ++s) {
    if (h_windows[s] > ~0ull - total) return fail(PENGK_ERR_ARG, "pengk_pattern_stats_strata: the weights sum beyond 2^64");
    total += h_windows[s];
    if (h_windows[s]) {
      mix.row[mix.n] = s;
      mix.w[mix.n++] = (double)h_windows[s];
    }
  }
  if (mix.n == 0) return fail(PENGK_ERR_ARG, "pengk_pattern_stats_strata: every weight is zero");
  mix.total = (double)total;
  int rc = enter(ctx);
  if (rc) return rc;
  if (control)
    return launch_with(ctx, W, both ? 1 : 0, k, max_k, d_V, mix, d_ltot, d_counts, d_bgprob, d_expected, d_logp, d_z,
                       Control{d_ctrl_counts, (const unsigned long long*)d_ctrl_ltot, pseudocount});
  return launch_with(ctx, W, both ? 1 : 0, k, max_k, d_V, mix, d_ltot, d_counts, d_bgprob, d_expected, d_logp, d_z);
}

}  // extern "C"
