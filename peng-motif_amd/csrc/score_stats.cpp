// score_stats.cpp -- the host side of the motif reports: what is computed from the histograms and counts that the
// kernels of score.hip, sites.hip and site_stats.hip leave.  No device code; double precision throughout.
//
//   scoring         AUC and occurrence from two best-score histograms, exact score tails under a background
//   q-values        Benjamini-Hochberg q-values from a site histogram and the score tail
//   enrichment      Fisher's exact tail over every threshold of two best-score histograms
//   centrality      the most enriched central window, by a binomial tail
//   spacing         co-occurrence and the preferred gap of a motif pair, by binomial tails
//   refinement      column frequencies and information content from the site profiles
//   first order     the interpolated first-order model from the single and pair profiles
#include <string.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "pengk_internal.h"

namespace pengk {
namespace {

// clamp(lround(100 log2(p / g)), -2000, 2000) in double: log_odds of host/motif_score.cpp
int32_t dinuc_log_odds(double p, double g) {
  const double v = 100.0 * std::log2(p / g);
  return (int32_t)std::lround(std::max(-2000.0, std::min(2000.0, v)));
}

// Lentz's continued fraction of the regularised incomplete beta: I_x(a, b) = x^a (1-x)^b / (a B(a, b)) * betacf(a, b, x),
// fast to converge for x < (a + 1) / (a + b + 2) (Numerical Recipes 6.4)
double betacf(double a, double b, double x) {
  const double FPMIN = 1e-300, EPS = 1e-16;
  const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
  auto tiny = [&](double v) { return std::fabs(v) < FPMIN ? FPMIN : v; };
  double c = 1.0, d = 1.0 / tiny(1.0 - qab * x / qap), h = d;
  for (int64_t i = 1; i <= (1 << 22); ++i) {
    const double m = (double)i, m2 = 2.0 * m;
    double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
    d = 1.0 / tiny(1.0 + aa * d);
    c = tiny(1.0 + aa / c);
    h *= d * c;
    aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
    d = 1.0 / tiny(1.0 + aa * d);
    c = tiny(1.0 + aa / c);
    const double del = d * c;
    h *= del;
    if (std::fabs(del - 1.0) < EPS) break;
  }
  return h;
}

// log10 P(X >= k) for X ~ Binomial(n, p) = log10 I_p(k, n - k + 1), in log space throughout: no underflow however small
// the tail (CentriMo's binomial test, which reports the same tail)
double log10_binomial_sf(uint64_t n, uint64_t k, double p) {
  if (k == 0 || p >= 1.0) return 0.0;
  if (p <= 0.0) return -INFINITY;
  const double a = (double)k, b = (double)(n - k) + 1.0;
  const double lbeta = std::lgamma(a) + std::lgamma(b) - std::lgamma(a + b);
  const double lfront = a * std::log(p) + b * std::log1p(-p) - lbeta;
  double ln;
  if (p < (a + 1.0) / (a + b + 2.0)) {
    ln = lfront - std::log(a) + std::log(betacf(a, b, p));
  } else {  // the upper tail is the larger part: 1 - I_{1-p}(b, a)
    const double q = std::exp(lfront - std::log(b)) * betacf(b, a, 1.0 - p);
    ln = q < 1.0 ? std::log1p(-q) : lfront - std::log(a) + std::log(betacf(a, b, p));  // (rounding: the direct form)
  }
  return ln / std::log(10.0);
}

// ---- the hypergeometric tail of --enrich (Loader 2000, "Fast and accurate computation of binomial probabilities") -----
// stirlerr(n) = log(n!) - log(sqrt(2 pi n) (n / e)^n), n >= 1: the series in 1 / n above 15, lgamma below
double stirlerr(double n) {
  const double S0 = 1.0 / 12.0, S1 = 1.0 / 360.0, S2 = 1.0 / 1260.0, S3 = 1.0 / 1680.0, S4 = 1.0 / 1188.0;
  const double HALF_LN_2PI = 0.918938533204672741780329736406;
  if (n <= 15.0) return std::lgamma(n + 1.0) - (n + 0.5) * std::log(n) + n - HALF_LN_2PI;
  const double nn = n * n;
  if (n > 500.0) return (S0 - S1 / nn) / n;
  if (n > 80.0) return (S0 - (S1 - S2 / nn) / nn) / n;
  if (n > 35.0) return (S0 - (S1 - (S2 - S3 / nn) / nn) / nn) / n;
  return (S0 - (S1 - (S2 - (S3 - S4 / nn) / nn) / nn) / nn) / n;
}

// bd0(x, np) = x log(x / np) + np - x, x > 0, np > 0: by its series in (x - np) / (x + np) where the direct form cancels
double bd0(double x, double np) {
  if (std::fabs(x - np) < 0.1 * (x + np)) {
    double v = (x - np) / (x + np);
    double s = (x - np) * v, ej = 2.0 * x * v;
    v = v * v;
    for (int j = 1; j < 1000; ++j) {
      ej *= v;
      const double s1 = s + ej / (double)(2 * j + 1);
      if (s1 == s) return s1;
      s = s1;
    }
    return s;
  }
  return x * std::log(x / np) + np - x;
}

// log of the Binomial(n, p) point mass at x (q = 1 - p, given apart so that neither is formed by a cancelling difference)
double log_dbinom(double x, double n, double p, double q) {
  if (p == 0.0) return x == 0.0 ? 0.0 : -INFINITY;
  if (q == 0.0) return x == n ? 0.0 : -INFINITY;
  if (x == 0.0) return n == 0.0 ? 0.0 : n * (p < 0.5 ? std::log1p(-p) : std::log(q));
  if (x == n) return n * (q < 0.5 ? std::log1p(-q) : std::log(p));
  const double lc = stirlerr(n) - stirlerr(x) - stirlerr(n - x) - bd0(x, n * p) - bd0(n - x, n * q);
  const double lf = 1.837877066409345483560659472811 + std::log(x) + std::log1p(-x / n);  // log(2 pi x (n - x) / n)
  return lc - 0.5 * lf;
}

// log P(X = x), X ~ Hypergeometric(N, K marked, n drawn), x inside the support: three binomial point masses at p = n / N
double log_dhyper(uint64_t N, uint64_t K, uint64_t n, uint64_t x) {
  const double p = (double)n / (double)N, q = (double)(N - n) / (double)N;
  return log_dbinom((double)x, (double)K, p, q) + log_dbinom((double)(n - x), (double)(N - K), p, q) -
         log_dbinom((double)n, (double)N, p, q);
}

// log10 P(X >= k) for the same X.  The point mass at the end of the shorter tail, then the ratio recurrence away from the
// mode, its terms relative to that point mass (they fall from 1.0: nothing under- or overflows): upwards from k when the
// terms fall from k on, else downwards from k - 1 and the complement.
double log10_hypergeom_sf(uint64_t N, uint64_t K, uint64_t n, uint64_t k) {
  const uint64_t lo = n + K > N ? n + K - N : 0, hi = std::min(K, n);
  if (k <= lo) return 0.0;
  if (k > hi) return -INFINITY;
  const double dN = (double)N, dK = (double)K, dn = (double)n;
  // P(x + 1) / P(x) = (K - x)(n - x) / ((x + 1)(N - K - n + x + 1))
  auto up = [&](double x) { return (dK - x) * (dn - x) / ((x + 1.0) * (dN - dK - dn + x + 1.0)); };
  const double LN10 = std::log(10.0);
  if (up((double)k) <= 1.0) {
    double term = 1.0, sum = 1.0;
    for (uint64_t x = k; x < hi; ++x) {
      term *= up((double)x);
      sum += term;
      if (term < sum * 1e-18) break;
    }
    return (log_dhyper(N, K, n, k) + std::log(sum)) / LN10;
  }
  // (k is at or below the mode: k - 1 >= lo is below it)
  double term = 1.0, sum = 1.0;
  for (uint64_t x = k - 1; x > lo; --x) {
    term /= up((double)(x - 1));
    sum += term;
    if (term < sum * 1e-18) break;
  }
  const double lower = std::exp(log_dhyper(N, K, n, k - 1) + std::log(sum));
  return lower < 1.0 ? std::log1p(-lower) / LN10 : -INFINITY;
}

}  // namespace
}  // namespace pengk

using namespace pengk;

extern "C" {

int pengk_score_summary(const uint64_t* h_pos, const uint64_t* h_neg, uint64_t nbins, double* zoops_out, double* occur_out) {
  if (!h_pos || !h_neg || !zoops_out || !occur_out || nbins == 0) return fail(PENGK_ERR_ARG, "pengk_score_summary: bad argument");
  const uint64_t LIMIT = 1ull << 62;
  uint64_t npos = 0, nneg = 0;
  for (uint64_t s = 0; s < nbins; ++s) {
    npos += h_pos[s];
    nneg += h_neg[s];
    if (npos > LIMIT || nneg > LIMIT) return fail(PENGK_ERR_RANGE, "pengk_score_summary: counts above 2^62");
  }
  if (npos == 0 || nneg == 0) {  // nothing to separate
    *zoops_out = 0.5;
    *occur_out = 0.0;
    return PENGK_OK;
  }
  // AUC numerator: sum_s P[s] * (2 * Nneg_below(s) + N[s]), every product and sum checked against 2^62
  unsigned __int128 num = 0;
  uint64_t below = 0;
  for (uint64_t s = 0; s < nbins; ++s) {
    num += (unsigned __int128)h_pos[s] * (2 * (unsigned __int128)below + h_neg[s]);
    if (num > (unsigned __int128)LIMIT) return fail(PENGK_ERR_RANGE, "pengk_score_summary: AUC numerator above 2^62");
    below += h_neg[s];
  }
  *zoops_out = (double)(uint64_t)num / (2.0 * (double)npos * (double)nneg);
  // occur: the smallest threshold t with 100 * Nneg_ge(t) <= Nneg (t = nbins: above every score)
  uint64_t neg_ge = nneg, pos_ge = npos, t = 0;
  for (; t < nbins; ++t) {
    if ((unsigned __int128)100 * neg_ge <= nneg) break;
    neg_ge -= h_neg[t];
    pos_ge -= h_pos[t];
  }
  const double fpr = (double)neg_ge / (double)nneg, tpr = (double)pos_ge / (double)npos;
  double occ = fpr == 1.0 ? 0.0 : (tpr - fpr) / (1.0 - fpr);
  *occur_out = occ < 0.0 ? 0.0 : occ > 1.0 ? 1.0 : occ;
  return PENGK_OK;
}

int pengk_score_tail_pvalues(const int32_t* h_S, int w, const float* h_bg, int32_t* lo_out, int32_t* hi_out, double* h_tail) {
  if (!h_S || !h_bg || !lo_out || !hi_out || w < 1 || w > PENGK_MAX_MOTIF_LEN)
    return fail(PENGK_ERR_ARG, "pengk_score_tail_pvalues: bad argument");
  int32_t lo = 0, hi = 0;
  for (int j = 0; j < w; ++j) {
    int32_t mn = 2000, mx = -2000;
    for (int a = 0; a < 4; ++a) {
      const int32_t v = h_S[j * 4 + a];
      if (v < -2000 || v > 2000) return fail(PENGK_ERR_ARG, "pengk_score_tail_pvalues: log-odds %d outside [-2000, 2000]", v);
      mn = std::min(mn, v);
      mx = std::max(mx, v);
    }
    lo += mn;
    hi += mx;
  }
  *lo_out = lo;
  *hi_out = hi;
  if (!h_tail) return PENGK_OK;
  double bg[4];
  for (int a = 0; a < 4; ++a) bg[a] = (double)h_bg[a];
  // q_j over the scores [clo, chi] of the first j columns; q_{j+1}[t] = sum over a = 0..3, in this order, of
  // q_j[t - S[j][a]] * bg[a], each from 0.0
  const size_t n = (size_t)(hi - lo) + 1;
  std::vector<double> q(n, 0.0), nq(n, 0.0);
  q[0] = 1.0;
  int32_t clo = 0, chi = 0;
  for (int j = 0; j < w; ++j) {
    int32_t mn = 2000, mx = -2000;
    for (int a = 0; a < 4; ++a) {
      mn = std::min(mn, h_S[j * 4 + a]);
      mx = std::max(mx, h_S[j * 4 + a]);
    }
    const int32_t nlo = clo + mn, nhi = chi + mx;
    for (int32_t t = nlo; t <= nhi; ++t) {
      double v = 0.0;
      for (int a = 0; a < 4; ++a) {
        const int32_t u = t - h_S[j * 4 + a];
        if (u >= clo && u <= chi) v += q[(size_t)(u - clo)] * bg[a];
      }
      nq[(size_t)(t - nlo)] = v;
    }
    q.swap(nq);
    clo = nlo;
    chi = nhi;
  }
  // the tail, summed from the highest score down
  double acc = 0.0;
  for (int64_t t = hi; t >= lo; --t) {
    acc += q[(size_t)(t - lo)];
    h_tail[t - lo] = acc;
  }
  return PENGK_OK;
}

int pengk_score_threshold(const double* h_tail, int32_t lo, int32_t hi, double p, int32_t* t_out) {
  if (!h_tail || !t_out || hi < lo || !(p > 0.0 && p <= 1.0)) return fail(PENGK_ERR_ARG, "pengk_score_threshold: bad argument");
  int32_t t = lo;
  while (t <= hi && !(h_tail[t - lo] <= p)) ++t;
  *t_out = t;
  return PENGK_OK;
}

int pengk_hypergeom_log10_sf(uint64_t N, uint64_t K, uint64_t n, uint64_t k, double* out) {
  if (!out || K > N || n > N) return fail(PENGK_ERR_ARG, "pengk_hypergeom_log10_sf: bad argument");
  *out = log10_hypergeom_sf(N, K, n, k);
  return PENGK_OK;
}

int pengk_enrich_summary(const uint64_t* h_pos, const uint64_t* h_neg, uint64_t nbins, int32_t thr, uint64_t n_pos,
                         uint64_t n_neg, pengk_enrichment* out) {
  if (!out || (nbins && (!h_pos || !h_neg)) || nbins > (1ull << 31) || (int64_t)thr + (int64_t)nbins > (int64_t)INT32_MAX ||
      n_pos + n_neg < n_pos)
    return fail(PENGK_ERR_ARG, "pengk_enrich_summary: bad argument");
  uint64_t a = 0, b = 0;
  for (uint64_t k = 0; k < nbins; ++k) {
    if (h_pos[k] > n_pos - a || h_neg[k] > n_neg - b)
      return fail(PENGK_ERR_ARG, "pengk_enrich_summary: more hits than scored sequences");
    a += h_pos[k];
    b += h_neg[k];
  }
  memset(out, 0, sizeof *out);
  out->threshold = (int32_t)((int64_t)thr + (int64_t)nbins);
  const uint64_t N = n_pos + n_neg;
  a = b = 0;
  for (uint64_t k = nbins; k-- > 0;) {
    a += h_pos[k];
    b += h_neg[k];
    if (h_pos[k] + h_neg[k] == 0) continue;  // (the tail of the threshold above: not a test of its own)
    const double lp = log10_hypergeom_sf(N, a + b, n_pos, a);
    if (out->n_thresholds == 0 || lp < out->log10_pvalue) {  // (from the top down: the higher threshold wins a tie)
      out->threshold = (int32_t)((int64_t)thr + (int64_t)k);
      out->pos_hits = a;
      out->neg_hits = b;
      out->log10_pvalue = lp;
    }
    ++out->n_thresholds;
  }
  out->enrichment = (((double)out->pos_hits + 1.0) / ((double)n_pos + 1.0)) / (((double)out->neg_hits + 1.0) / ((double)n_neg + 1.0));
  out->log10_adj_pvalue = out->n_thresholds ? std::min(0.0, out->log10_pvalue + std::log10((double)out->n_thresholds)) : 0.0;
  return PENGK_OK;
}

int pengk_sites_qvalues(const uint64_t* h_hist, uint64_t nbins, uint64_t n_tests, const double* h_tail_from_thr, double* h_q) {
  if (nbins && (!h_hist || !h_tail_from_thr || !h_q)) return fail(PENGK_ERR_ARG, "pengk_sites_qvalues: bad argument");
  // r(s) = N * tail / n(s), the ranks n(s) summed from the highest score down
  const double N = (double)n_tests;
  uint64_t n = 0;
  for (uint64_t k = nbins; k-- > 0;) {
    n += h_hist[k];
    if (n > 0) {
      const double x = N * h_tail_from_thr[k];
      h_q[k] = x / (double)n;
    } else {
      h_q[k] = INFINITY;
    }
  }
  // q(s) = min(1, min over s' <= s of r(s')), a running minimum from the threshold up
  double mn = INFINITY;
  for (uint64_t k = 0; k < nbins; ++k) {
    if (h_q[k] < mn) mn = h_q[k];
    h_q[k] = mn < 1.0 ? mn : 1.0;
  }
  return PENGK_OK;
}

int pengk_qvalue_threshold(const double* h_q, uint64_t nbins, int32_t t, double q_max, int32_t* t_out) {
  if (!t_out || (nbins && !h_q) || !(q_max >= 0.0) || (int64_t)t + (int64_t)nbins > (int64_t)INT32_MAX || nbins > (1ull << 32))
    return fail(PENGK_ERR_ARG, "pengk_qvalue_threshold: bad argument");
  uint64_t k = 0;
  while (k < nbins && !(h_q[k] <= q_max)) ++k;
  *t_out = (int32_t)((int64_t)t + (int64_t)k);
  return PENGK_OK;
}

int pengk_binomial_log10_sf(uint64_t n, uint64_t k, double p, double* out) {
  if (!out || k > n || !(p >= 0.0 && p <= 1.0)) return fail(PENGK_ERR_ARG, "pengk_binomial_log10_sf: bad argument");
  *out = log10_binomial_sf(n, k, p);
  return PENGK_OK;
}

int pengk_centrality_summary(const uint64_t* h_hist_offsets, const uint64_t* h_hist_lengths, uint32_t max_len, int w,
                             int n_motifs, pengk_centrality* out) {
  if (!h_hist_offsets || !h_hist_lengths || !out || max_len < 1 || max_len > PENGK_CENTRALITY_MAX_LEN || w < 1 ||
      w > PENGK_MAX_MOTIF_LEN || n_motifs < 1)
    return fail(PENGK_ERR_ARG, "pengk_centrality_summary: bad argument");
  memset(out, 0, sizeof *out);
  const int64_t C0 = max_len;  // bin of d = 0
  // N, Dm and the sites' offsets against the lengths they can come from
  uint64_t N = 0, Nd = 0;
  int64_t Dm = -1;
  for (uint32_t L = 0; L <= max_len; ++L) {
    const uint64_t n = h_hist_lengths[L];
    if (!n) continue;
    if ((int64_t)L < w) return fail(PENGK_ERR_ARG, "pengk_centrality_summary: sites on a sequence shorter than the motif");
    N += n;
    Dm = (int64_t)L - w;
  }
  for (int64_t b = 0; b <= 2 * C0; ++b) {
    const uint64_t n = h_hist_offsets[b];
    if (!n) continue;
    if (std::abs(b - C0) > Dm) return fail(PENGK_ERR_ARG, "pengk_centrality_summary: offset beyond the longest sequence");
    Nd += n;
  }
  if (N != Nd) return fail(PENGK_ERR_ARG, "pengk_centrality_summary: the histograms hold different totals");
  out->sites = N;
  if (N == 0) return PENGK_OK;
  out->max_offset = (uint32_t)Dm;
  // N p(r) = sum_L n_L #{p : |2p + w - L| <= r} / (D + 1), D = L - w: #{...} = D + 1 for r >= D, else r + [r = D mod 2].
  // By D: N p(r) = r (A_0(r) + A_1(r)) + A_{r mod 2}(r) + B(r) with A_par(r) = sum over D > r, D = par (mod 2) of
  // n_D / (D + 1) and B(r) = sum over D <= r of n_D -- suffix and prefix sums: O(Dm + lengths), not their product.
  const size_t nD = (size_t)Dm + 1;
  std::vector<double> A0(nD + 1, 0.0), A1(nD + 1, 0.0);  // A_par over D >= r (shifted by one below)
  std::vector<uint64_t> cnt(nD, 0), hit0(nD + 1, 0), hit1(nD + 1, 0);  // n_D; sites of D >= r by parity
  for (int64_t D = 0; D <= Dm; ++D) cnt[D] = h_hist_lengths[D + w];
  for (int64_t D = Dm; D >= 0; --D) {
    const double c = (double)cnt[D] / (double)(D + 1);
    A0[D] = A0[D + 1] + ((D & 1) ? 0.0 : c);
    A1[D] = A1[D + 1] + ((D & 1) ? c : 0.0);
    hit0[D] = hit0[D + 1] + ((D & 1) ? 0 : cnt[D]);
    hit1[D] = hit1[D + 1] + ((D & 1) ? cnt[D] : 0);
  }
  uint64_t below = 0, K = h_hist_offsets[C0];
  double best = 0.0;
  bool have = false;
  for (int64_t r = 0; r <= Dm; ++r) {
    below += cnt[r];  // B(r)
    if (r) K += h_hist_offsets[C0 - r] + h_hist_offsets[C0 + r];
    // r is a window of its own only if a sequence has an offset of its parity at distance r: otherwise p(r) and K(r)
    // equal those of r - 1 exactly (and p(0) = K(0) = 0), a tie that the smaller r wins
    if (((r & 1) ? hit1[r] : hit0[r]) == 0) continue;
    const double a0 = A0[r + 1], a1 = A1[r + 1];
    const double np = (double)r * (a0 + a1) + ((r & 1) ? a1 : a0) + (double)below;
    const double pbar = std::min(1.0, np / (double)N);
    const double lp = log10_binomial_sf(N, K, pbar);
    if (!have || lp < best) {
      have = true;
      best = lp;
      out->window = (uint32_t)r;
      out->in_window = K;
      out->expected = np;
      out->log10_pvalue = lp;
    }
  }
  out->log10_evalue = out->log10_pvalue + std::log10((double)(Dm + 1)) + std::log10((double)n_motifs);
  return PENGK_OK;
}

int pengk_spacing_summary(const uint64_t* h_gaps, const uint64_t* h_lengths, uint32_t max_gap, uint32_t max_len, int w_a,
                          int w_b, int n_classes, uint64_t n, uint64_t n_a, uint64_t n_b, int n_pairs, pengk_spacing* out) {
  if (!h_gaps || !h_lengths || !out || max_gap > PENGK_SPACING_MAX_GAP || max_len < 1 || max_len > PENGK_CENTRALITY_MAX_LEN ||
      w_a < 1 || w_a > PENGK_MAX_MOTIF_LEN || w_b < 1 || w_b > PENGK_MAX_MOTIF_LEN || (n_classes != 2 && n_classes != 4) ||
      n_a > n || n_b > n || n_pairs < 1)
    return fail(PENGK_ERR_ARG, "pengk_spacing_summary: bad argument");
  memset(out, 0, sizeof *out);
  const uint32_t G1 = max_gap + 1;
  uint64_t near = 0;
  for (uint32_t k = 0; k < 4 * G1; ++k) {
    if (h_gaps[k] && (int)(k / G1) >= n_classes)
      return fail(PENGK_ERR_ARG, "pengk_spacing_summary: a count in orientation %u of %d", k / G1, n_classes);
    near += h_gaps[k];
  }
  out->overlapping = h_gaps[4 * G1];
  out->far = h_gaps[4 * G1 + 1];
  out->apart = near + out->far;
  out->both = out->overlapping + out->apart;
  if (out->both > n_a || out->both > n_b) return fail(PENGK_ERR_ARG, "pengk_spacing_summary: more pairs than sites of a motif");
  // the apart sequences' lengths, ascending
  const int64_t ws = (int64_t)w_a + w_b;
  std::vector<uint32_t> Ls;
  uint64_t nl = 0;
  for (uint32_t L = 0; L <= max_len; ++L) {
    if (!h_lengths[L]) continue;
    if ((int64_t)L < ws) return fail(PENGK_ERR_ARG, "pengk_spacing_summary: two sites apart on a sequence shorter than both motifs");
    nl += h_lengths[L];
    Ls.push_back(L);
  }
  if (nl != out->apart) return fail(PENGK_ERR_ARG, "pengk_spacing_summary: the histograms hold different totals");
  if (n) {
    const double p_co = ((double)n_a / (double)n) * ((double)n_b / (double)n);
    out->expected_both = (double)n * p_co;
    out->log10_pvalue_both = log10_binomial_sf(n, out->both, p_co);
  }
  const uint64_t Na = out->apart;
  if (Na == 0) return PENGK_OK;
  std::vector<double> pg(G1, 0.0);
  for (uint32_t g = 0; g <= max_gap; ++g) {
    double s = 0.0;
    for (const uint32_t L : Ls) {
      const int64_t T = (int64_t)L - ws + 1, k = T - (int64_t)g;
      if (k > 0) s += (double)h_lengths[L] * (double)k / ((double)n_classes * (double)(T * (T + 1) / 2));
    }
    pg[g] = s / (double)Na;
    if (pg[g] > 0.0) {
      ++out->tested_gaps;
      continue;
    }
    for (int c = 0; c < n_classes; ++c)
      if (h_gaps[(uint32_t)c * G1 + g]) return fail(PENGK_ERR_ARG, "pengk_spacing_summary: gap %u on sequences too short for it", g);
  }
  bool have = false;
  for (int c = 0; c < n_classes; ++c)
    for (uint32_t g = 0; g <= max_gap; ++g) {
      if (!(pg[g] > 0.0)) continue;
      const uint64_t H = h_gaps[(uint32_t)c * G1 + g];
      const double lp = log10_binomial_sf(Na, H, std::min(1.0, pg[g]));
      if (!have || lp < out->log10_pvalue) {
        have = true;
        out->orientation = (uint32_t)c;
        out->gap = g;
        out->count = H;
        out->expected = (double)Na * pg[g];
        out->log10_pvalue = lp;
      }
    }
  out->log10_evalue =
      out->log10_pvalue + std::log10((double)n_classes * (double)out->tested_gaps) + std::log10((double)n_pairs);
  return PENGK_OK;
}

int pengk_profile_refine(const uint64_t* h_counts, int w, int flank, const float* h_bg, double min_ic, double* h_q,
                         double* h_ic, float* h_pwm, int32_t* first_out, int32_t* last_out, uint64_t* sites_out) {
  if (!h_counts || !h_bg || !first_out || !last_out || w < 1 || w > PENGK_MAX_MOTIF_LEN || flank < 0 || !(min_ic == min_ic))
    return fail(PENGK_ERR_ARG, "pengk_profile_refine: bad argument");
  for (int b = 0; b < 4; ++b)
    if (!(h_bg[b] > 0.0f)) return fail(PENGK_ERR_ARG, "pengk_profile_refine: background frequency %d is not positive", b);
  const int F = std::min(flank, (PENGK_MAX_MOTIF_LEN - w) / 2), C = w + 2 * F;
  int first = C, last = 0;  // [first, last): empty
  for (int c = 0; c < C; ++c) {
    const uint64_t* k = h_counts + (size_t)c * 5;
    const uint64_t n = ((k[0] + k[1]) + k[2]) + k[3];
    double ic = 0.0;
    for (int b = 0; b < 4; ++b) {
      const double g = (double)h_bg[b];
      const double q = ((double)k[b] + g) / ((double)n + 1.0);
      ic += q * std::log2(q / g);
      if (h_q) h_q[(size_t)c * 4 + b] = q;
    }
    if (h_ic) h_ic[c] = ic;
    if (ic >= min_ic) {
      if (first == C) first = c;
      last = c + 1;
    }
  }
  if (first == C) first = 0;
  if (h_pwm)
    for (int c = first; c < last; ++c) {
      const uint64_t* k = h_counts + (size_t)c * 5;
      const uint64_t n = ((k[0] + k[1]) + k[2]) + k[3];
      for (int b = 0; b < 4; ++b)
        h_pwm[(size_t)(c - first) * 4 + b] = (float)(((double)k[b] + (double)h_bg[b]) / ((double)n + 1.0));
    }
  *first_out = first;
  *last_out = last;
  if (sites_out) {  // every site adds 1 to one bin of every column: the first motif column's total
    const uint64_t* k = h_counts + (size_t)F * 5;
    *sites_out = k[0] + k[1] + k[2] + k[3] + k[4];
  }
  return PENGK_OK;
}

int pengk_dinuc_model(const uint64_t* h_counts1, const uint64_t* h_counts2, int w, int flank, const float* h_bg0,
                      const float* h_bg1, double alpha, double* h_q0, double* h_q1, double* h_mi, int32_t* h_S0, int32_t* h_D1,
                      int32_t* h_D0, uint64_t* sites_out) {
  if (!h_counts1 || !h_counts2 || !h_bg0 || !h_bg1 || w < 1 || w > PENGK_MAX_MOTIF_LEN || flank < 0 || !(alpha > 0.0) ||
      !(alpha <= 1.7976931348623157e308))
    return fail(PENGK_ERR_ARG, "pengk_dinuc_model: bad argument");
  for (int b = 0; b < 4; ++b)
    if (!(h_bg0[b] > 0.0f)) return fail(PENGK_ERR_ARG, "pengk_dinuc_model: background frequency %d is not positive", b);
  for (int b = 0; b < 16; ++b)
    if (!(h_bg1[b] > 0.0f)) return fail(PENGK_ERR_ARG, "pengk_dinuc_model: background conditional %d is not positive", b);
  const int F = std::min(flank, (PENGK_MAX_MOTIF_LEN - w) / 2), C = w + 2 * F;
  double g0[4], g1[16];
  for (int b = 0; b < 4; ++b) g0[b] = (double)h_bg0[b];
  for (int b = 0; b < 16; ++b) g1[b] = (double)h_bg1[b];
  for (int c = 0; c < C; ++c) {
    const uint64_t* k1 = h_counts1 + (size_t)c * 5;
    const uint64_t* k2 = h_counts2 + (size_t)c * 17;
    const uint64_t n1 = ((k1[0] + k1[1]) + k1[2]) + k1[3];
    double q0[4];
    for (int b = 0; b < 4; ++b) q0[b] = ((double)k1[b] + g0[b]) / ((double)n1 + 1.0);
    if (h_q0)
      for (int b = 0; b < 4; ++b) h_q0[(size_t)c * 4 + b] = q0[b];
    if (c == 0 && h_S0)
      for (int b = 0; b < 4; ++b) h_S0[b] = dinuc_log_odds(q0[b], g0[b]);
    uint64_t row[4], col[4];
    for (int a = 0; a < 4; ++a) row[a] = ((k2[4 * a] + k2[4 * a + 1]) + k2[4 * a + 2]) + k2[4 * a + 3];
    for (int b = 0; b < 4; ++b) col[b] = ((k2[b] + k2[4 + b]) + k2[8 + b]) + k2[12 + b];
    for (int a = 0; a < 4; ++a)
      for (int b = 0; b < 4; ++b) {
        const int x = 4 * a + b;
        const double q1 = c == 0 ? q0[b] : ((double)k2[x] + alpha * q0[b]) / ((double)row[a] + alpha);
        if (h_q1) h_q1[(size_t)c * 16 + x] = q1;
        if (h_D1) h_D1[(size_t)c * 16 + x] = c == 0 ? 0 : dinuc_log_odds(q1, g1[x]);
        if (h_D0) h_D0[(size_t)c * 16 + x] = c == 0 ? 0 : dinuc_log_odds(q0[b], g1[x]);
      }
    if (h_mi) {
      double mi = 0.0;
      const uint64_t N = ((row[0] + row[1]) + row[2]) + row[3];
      if (c > 0 && N > 0)
        for (int a = 0; a < 4; ++a)
          for (int b = 0; b < 4; ++b) {
            const uint64_t k = k2[4 * a + b];
            if (k == 0) continue;
            const double num = (double)k * (double)N, den = (double)row[a] * (double)col[b];
            mi += ((double)k / (double)N) * std::log2(num / den);
          }
      h_mi[c] = mi;
    }
  }
  if (sites_out) {
    const uint64_t* k = h_counts1 + (size_t)F * 5;
    *sites_out = k[0] + k[1] + k[2] + k[3] + k[4];
  }
  return PENGK_OK;
}

// BackgroundModel::calculateV (host/shared/BackgroundModel.cpp) continued to order K <= 5: float32, the same operations in
// the same order (this file is compiled without fused multiply-adds).  DESIGN.md 29.
int pengk_bg_model_order(const uint64_t* h_counts, int K, const float* h_alpha, int interpolate, float* h_V) {
  if (!h_counts || !h_alpha || !h_V) return fail(PENGK_ERR_ARG, "pengk_bg_model_order: NULL argument");
  if (K < 0 || K > 5) return fail(PENGK_ERR_ARG, "pengk_bg_model_order: order %d out of range [0,5]", K);
  auto at = [](int k) { return (size_t)(((1u << (2 * (k + 1))) - 4u) / 3u); };
  uint64_t base_counts = 0;
  for (int y = 0; y < 4; ++y) base_counts += h_counts[y];
  for (int y = 0; y < 4; ++y) h_V[y] = ((float)h_counts[y] + h_alpha[0] * 0.25f) / ((float)base_counts + h_alpha[0]);
  for (int k = 1; k <= K; ++k) {
    const int ny = 1 << (2 * (k + 1)), yk = 1 << (2 * k);
    const uint64_t* n = h_counts + at(k);
    const uint64_t* below = h_counts + at(k - 1);
    float* v = h_V + at(k);
    const float* prior_of = h_V + at(k - 1);
    const float a = h_alpha[k];
    for (int y = 0; y < ny; ++y) {
      const float prior = interpolate ? prior_of[y % yk] : 0.25f;
      v[y] = ((float)n[y] + a * prior) / ((float)below[y / 4] + a);
    }
    for (int g = 0; g < ny; g += 4) {
      float factor = 0.0f;
      for (int b = 0; b < 4; ++b) factor += v[g + b];
      for (int b = 0; b < 4; ++b) v[g + b] /= factor;
    }
  }
  return PENGK_OK;
}

}  // extern "C"
