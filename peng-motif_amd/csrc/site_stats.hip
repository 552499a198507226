// site_stats.hip -- what the reports on a motif's best sites need from the device (scan_walk.h; the motifs staged by
// score.hip).
//
//   best sites     (--centrality) the scan's walk keeping the best window strand of every motif on every
//                  sequence, ties broken by a counter-based key; the offset and length histograms of those sites
//   spacing        (--spacing) the gap, orientation and length histograms of motif pairs' best sites
//   profiles       (--refine) the base counts of every column of the best sites and their flanks
//   first order    (--dinuc) the adjacent-pair counts of the best sites, and the scan again with a 16-entry
//                  boundary table behind every chunk table (scan::Order1)
// The tests and models computed from these counts are host code: score_stats.cpp.
#include <string.h>

#include <algorithm>
#include <vector>

#include "pengk_internal.h"
#include "scan_walk.h"

namespace pengk {
using namespace scan;  // the shared walk and its records (scan_walk.h)
namespace {

// ---- central enrichment (pengk_motif_best_sites, pengk_centrality_histograms) --------------------------
constexpr uint64_t GOLDEN = 0x9E3779B97F4A7C15ull;
constexpr int CENT_LDS_BINS = 16384;  // offset and length bins of one motif in LDS (64 KiB) when they all fit, else global

// the best window strand of every motif on every sequence: the largest (score, key), key = mix64(h ^ (2p + s)),
// h = mix64(GOLDEN * (g + 1) ^ m); an equal key keeps the earlier window strand, which the scan order (p, then + before
// -) makes the smaller (p, s).  Keys are computed on ties only: the best's own key once, then the challenger's.
template <bool BOTH>
struct BestSiteVisit {
  const MotifRec* mrec;
  int32_t* best_out;
  unsigned long long* site_out;
  uint64_t n_seq, i, g;
  int32_t b[SCAN_PASS];
  uint64_t c[SCAN_PASS];   // 2p + s of the best
  uint64_t h[SCAN_PASS];
  uint64_t kb[SCAN_PASS];  // its key, once kv
  bool kv[SCAN_PASS];
  __device__ __forceinline__ void begin(int q, int r) {
    b[q] = PENGK_SCORE_SENTINEL;
    c[q] = 0;
    kv[q] = false;
    h[q] = mix64((GOLDEN * (g + 1)) ^ (uint64_t)mrec[r].m);
  }
  __device__ __forceinline__ void offer(int q, uint64_t cand, int32_t sc) {
    if (sc > b[q]) {
      b[q] = sc;
      c[q] = cand;
      kv[q] = false;
      return;
    }
    if (!kv[q]) {
      kb[q] = mix64(h[q] ^ c[q]);
      kv[q] = true;
    }
    const uint64_t k = mix64(h[q] ^ cand);
    if (k > kb[q]) {
      c[q] = cand;
      kb[q] = k;
    }
  }
  __device__ __forceinline__ void window(int q, uint32_t pos, int32_t sf, int32_t sr) {
    if (sf >= b[q]) offer(q, 2ull * pos, sf);
    if (BOTH && sr >= b[q]) offer(q, 2ull * pos + 1ull, sr);
  }
  __device__ __forceinline__ void end(int q, int r) {
    const uint64_t o = (uint64_t)mrec[r].m * n_seq + i;
    best_out[o] = b[q];
    site_out[o] = c[q];
  }
};

// a kernel of its own: the visitor's state (key, site) stays out of the scoring and sites kernels
template <bool BOTH>
__global__ __launch_bounds__(SCAN_THREADS) void motif_best_site_kernel(const uint64_t* __restrict__ words,
                                                                       const uint32_t* __restrict__ valid,
                                                                       const int64_t* __restrict__ offs,
                                                                       const uint32_t* __restrict__ lens, uint64_t n_seq,
                                                                       uint64_t seq0, const int32_t* __restrict__ tables,
                                                                       const MotifRec* __restrict__ recs,
                                                                       const GroupRec* __restrict__ groups,
                                                                       int32_t* __restrict__ best_out,
                                                                       unsigned long long* __restrict__ site_out) {
  __shared__ int32_t tab[SCAN_TABLES * 256];
  __shared__ MotifRec mrec[SCAN_MAX_MOTIFS];
  const GroupRec g = groups[blockIdx.y];
  load_group(g, tables, recs, tab, mrec);
  __syncthreads();
  for (uint64_t i = blockIdx.x * (uint64_t)SCAN_THREADS + threadIdx.x; i < n_seq; i += (uint64_t)gridDim.x * SCAN_THREADS) {
    const uint32_t L = lens[i];
    const uint64_t w0 = (uint64_t)offs[i] >> 5;
    BestSiteVisit<BOTH> v{mrec, best_out, site_out, n_seq, i, seq0 + i, {}, {}, {}, {}, {}};
    walk_sequence<BOTH>(words + w0, valid ? valid + w0 : nullptr, L, tab, mrec, g.m1 - g.m0, v);
  }
}

// per motif (blockIdx.y): the best sites at or above its threshold of the sequences with w <= L <= max_len, ADDED to
// the offset bins hd[m * (2 max_len + 1) + max_len + d], d = 2p + w - L, and the length bins hl[m * (max_len + 1) + L].
// LDS: every bin of the motif in LDS (equal lengths send all counts to a few bins), flushed once per block.
template <bool LDS>
__global__ __launch_bounds__(HIST_THREADS) void centrality_hist_kernel(const int32_t* __restrict__ best,
                                                                       const unsigned long long* __restrict__ site,
                                                                       const uint32_t* __restrict__ lens, uint64_t n_seq,
                                                                       const int32_t* __restrict__ wt, uint32_t max_len,
                                                                       unsigned long long* __restrict__ hd,
                                                                       unsigned long long* __restrict__ hl) {
  __shared__ uint32_t h[LDS ? CENT_LDS_BINS : 1];
  const int m = blockIdx.y;
  const uint32_t w = (uint32_t)wt[2 * m];
  const int32_t t = wt[2 * m + 1];
  const uint32_t nd = 2 * max_len + 1, nl = max_len + 1;
  unsigned long long* HD = hd + (uint64_t)m * nd;
  unsigned long long* HL = hl + (uint64_t)m * nl;
  if (LDS) {
    for (uint32_t k = threadIdx.x; k < nd + nl; k += HIST_THREADS) h[k] = 0;
    __syncthreads();
  }
  const int32_t* B = best + (uint64_t)m * n_seq;
  const unsigned long long* C = site + (uint64_t)m * n_seq;
  for (uint64_t i = blockIdx.x * (uint64_t)HIST_THREADS + threadIdx.x; i < n_seq; i += (uint64_t)gridDim.x * HIST_THREADS) {
    const uint32_t L = lens[i];
    if (B[i] < t || L > max_len || L < w) continue;
    const uint64_t p = C[i] >> 1;
    if (p > L - w) continue;  // (not a window of this sequence: no bin)
    const uint32_t bd = 2 * (uint32_t)p + w + max_len - L;  // max_len + d, in [max_len - (L - w), max_len + (L - w)]
    if (LDS) {
      atomicAdd(&h[bd], 1u);
      atomicAdd(&h[nd + L], 1u);
    } else {
      atomicAdd(&HD[bd], 1ull);
      atomicAdd(&HL[L], 1ull);
    }
  }
  if (LDS) {
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < nd + nl; k += HIST_THREADS)
      if (h[k]) atomicAdd(k < nd ? &HD[k] : &HL[k - nd], (unsigned long long)h[k]);
  }
}

// ---- motif pair spacing (pengk_spacing_histograms) ---------------------------------------------------
constexpr int SPACE_THREADS = 1024;
constexpr int SPACE_LDS_BINS = 16000;  // the bins of one row's pairs in LDS (62.5 KiB, two workgroups per CU)

// a grid row: motif b against the motifs [a0, a1) before it; the row with a0 = 0 also counts b's own sites
struct SpaceRow {
  int32_t b, a0, a1, pad;
};

// One more in bin `bin` of h for every lane with `on`; every lane of the wave calls.  The lanes that share the first
// counting lane's bin add once, together: a composite element sends nearly every lane to one gap bin and equal-length
// input sends every lane to one length bin, where 64 adds to one LDS address would queue.  The others add on their own.
__device__ __forceinline__ void wave_count(uint32_t* h, bool on, uint32_t bin) {
  const unsigned long long act = __ballot(on);
  if (!act) return;
  const int lead = __ffsll(act) - 1;
  const uint32_t first = (uint32_t)__shfl((int)bin, lead);
  const unsigned long long same = __ballot(on && bin == first);
  if (!on) return;
  if (bin != first) atomicAdd(&h[bin], 1u);
  else if ((int)(threadIdx.x & 63u) == lead) atomicAdd(&h[first], (uint32_t)__popcll(same));
}

// per row (blockIdx.y): motif b's site read once per sequence and, only where b has one, the motifs a of the row: best[a]
// first, site[a] on a hit.  wt: (width, threshold) per motif.  Considered: min_len <= L <= max_len.  Pair q = b (b - 1) / 2
// + a owns nb = 4 (G + 1) + 2 gap bins in hg and max_len + 1 length bins in hl (include/pengk.h, "motif pair spacing").
// LDS: the row's (a1 - a0) (nb + max_len + 1) bins in LDS as uint32, flushed once per block, one add per non-zero bin.
template <bool LDS>
__global__ __launch_bounds__(SPACE_THREADS) void spacing_hist_kernel(const int32_t* __restrict__ best,
                                                                     const unsigned long long* __restrict__ site,
                                                                     const uint32_t* __restrict__ lens, uint64_t n_seq,
                                                                     const int32_t* __restrict__ wt,
                                                                     const SpaceRow* __restrict__ rows, uint32_t G,
                                                                     uint32_t min_len, uint32_t max_len,
                                                                     unsigned long long* __restrict__ hg,
                                                                     unsigned long long* __restrict__ hl,
                                                                     unsigned long long* __restrict__ hm) {
  __shared__ uint32_t h[LDS ? SPACE_LDS_BINS : 1];
  __shared__ int32_t sw[PENGK_SPACING_MAX_MOTIFS], st[PENGK_SPACING_MAX_MOTIFS];
  __shared__ unsigned long long s_sites;
  const SpaceRow row = rows[blockIdx.y];
  const uint32_t nb = 4 * (G + 1) + 2, nl = max_len + 1, per = nb + nl;
  const uint32_t n_lds = (uint32_t)(row.a1 - row.a0) * per;  // (LDS only: the host made it fit)
  if (threadIdx.x < (unsigned)row.a1 || (int)threadIdx.x == row.b) {
    sw[threadIdx.x] = wt[2 * threadIdx.x];
    st[threadIdx.x] = wt[2 * threadIdx.x + 1];
  }
  if (threadIdx.x == 0) s_sites = 0;
  if (LDS)
    for (uint32_t k = threadIdx.x; k < n_lds; k += SPACE_THREADS) h[k] = 0;
  __syncthreads();
  const uint32_t wb = (uint32_t)sw[row.b];
  const int32_t tb = st[row.b];
  const int32_t* Bb = best + (uint64_t)row.b * n_seq;
  const unsigned long long* Cb = site + (uint64_t)row.b * n_seq;
  const uint64_t q0 = (uint64_t)row.b * (uint64_t)(row.b - 1) / 2;  // (b = 0: no pair, never used)
  uint32_t mine = 0;  // b's sites seen by this thread (a block walks fewer than 2^32 sequences: the host sees to it)
  // (the loop's trip count is the same for every lane of a wave: wave_count needs them all)
  for (uint64_t i0 = blockIdx.x * (uint64_t)SPACE_THREADS; i0 < n_seq; i0 += (uint64_t)gridDim.x * SPACE_THREADS) {
    const uint64_t i = i0 + threadIdx.x;
    bool has = false;
    uint32_t L = 0, pb = 0, sb = 0;
    if (i < n_seq) {
      L = lens[i];
      if (L >= min_len && L <= max_len) {
        const int32_t s = Bb[i];
        if (s != PENGK_SCORE_SENTINEL && s >= tb) {
          const unsigned long long c = Cb[i];
          has = (c >> 1) <= (unsigned long long)(L - wb);
          pb = (uint32_t)(c >> 1);
          sb = (uint32_t)(c & 1u);
        }
      }
    }
    mine += has;
    if (!__any(has)) continue;
    for (int a = row.a0; a < row.a1; ++a) {
      bool apart = false, hit = false;
      uint32_t bin = 0;
      if (has) {
        const int32_t s = best[(uint64_t)a * n_seq + i];
        if (s != PENGK_SCORE_SENTINEL && s >= st[a]) {
          const unsigned long long c = site[(uint64_t)a * n_seq + i];
          const uint32_t wa = (uint32_t)sw[a], sa = (uint32_t)(c & 1u);
          if ((c >> 1) <= (unsigned long long)(L - wa)) {
            const uint32_t pa = (uint32_t)(c >> 1);
            hit = true;
            if (pb >= pa + wa || pa >= pb + wb) {
              apart = true;
              const uint32_t side = pb >= pa + wa ? 0u : 1u;
              const uint32_t g = side ? pa - pb - wb : pb - pa - wa;
              bin = g <= G ? (2 * (sa ^ sb) + (side ^ sa)) * (G + 1) + g : nb - 1;
            } else {
              bin = nb - 2;
            }
          }
        }
      }
      if (LDS) {
        uint32_t* hp = h + (uint32_t)(a - row.a0) * per;
        wave_count(hp, hit, bin);
        wave_count(hp + nb, apart, L);
      } else if (hit) {
        const uint64_t q = q0 + (uint64_t)a;
        atomicAdd(&hg[q * nb + bin], 1ull);
        if (apart) atomicAdd(&hl[q * nl + L], 1ull);
      }
    }
  }
  if (row.a0 == 0 && mine) atomicAdd(&s_sites, (unsigned long long)mine);
  __syncthreads();
  if (row.a0 == 0 && threadIdx.x == 0 && s_sites) atomicAdd(&hm[row.b], s_sites);
  if (LDS)
    for (uint32_t k = threadIdx.x; k < n_lds; k += SPACE_THREADS)
      if (h[k]) {
        const uint32_t slot = k / per, r = k - slot * per;
        const uint64_t q = q0 + (uint64_t)row.a0 + slot;
        atomicAdd(r < nb ? &hg[q * nb + r] : &hl[q * nl + (r - nb)], (unsigned long long)h[k]);
      }
}

// ---- site profiles (pengk_site_profiles) -------------------------------------------------------------
constexpr int PROF_THREADS = 256;
constexpr int PROF_BINS = PENGK_MAX_MOTIF_LEN * 5;

// per motif (blockIdx.y): the base of every column c in [-F, w + F) of the best sites at or above the motif's threshold,
// read on the site's strand, ADDED to counts[(m * PENGK_MAX_MOTIF_LEN + c + F) * 5 + b] (b = 4: outside the sequence or
// not A/C/G/T).  A wave takes 64 consecutive sequences.  For a strong motif nearly every lane of it adds to the same
// (column, base) bin, so the lanes do not add at all: per column the wave ballots the two bits of the base, "is a base"
// and "has a site", counts the five bins from the masks, and lanes 0..4 add them once to the block's LDS bins, which
// are flushed once per block.  A site with its flanks spans at most 64 bases: three words per lane, loaded once.
// A wave without a site (the usual wave of a weak motif) reads best, site and length and goes on.
__global__ __launch_bounds__(PROF_THREADS) void site_profile_kernel(const uint64_t* __restrict__ words,
                                                                    const uint32_t* __restrict__ valid,
                                                                    const int64_t* __restrict__ offs,
                                                                    const uint32_t* __restrict__ lens, uint64_t n_seq,
                                                                    const int32_t* __restrict__ best,
                                                                    const unsigned long long* __restrict__ site,
                                                                    const int32_t* __restrict__ wtf,
                                                                    unsigned long long* __restrict__ counts) {
  __shared__ uint32_t bins[PROF_BINS];
  const int m = blockIdx.y;
  const int32_t w = wtf[3 * m], t = wtf[3 * m + 1], F = wtf[3 * m + 2];
  const int32_t C = w + 2 * F;  // <= PENGK_MAX_MOTIF_LEN (the host clamps F)
  for (int k = threadIdx.x; k < PROF_BINS; k += PROF_THREADS) bins[k] = 0;
  __syncthreads();
  const int32_t* B = best + (uint64_t)m * n_seq;
  const unsigned long long* S = site + (uint64_t)m * n_seq;
  const int lane = threadIdx.x & 63;
  // (every lane of a wave makes the same trips: the ballots below see the whole wave)
  for (uint64_t i0 = blockIdx.x * (uint64_t)PROF_THREADS + (threadIdx.x & ~63); i0 < n_seq;
       i0 += (uint64_t)gridDim.x * PROF_THREADS) {
    const uint64_t i = i0 + lane;
    bool sel = false;
    int64_t L = 0, p = 0;
    int32_t strand = 0;
    if (i < n_seq) {
      const int32_t b = B[i];
      L = lens[i];
      if (b != PENGK_SCORE_SENTINEL && b >= t && L >= w) {
        const uint64_t c = S[i];
        p = (int64_t)(c >> 1);
        strand = (int32_t)(c & 1);
        sel = p <= L - w;  // (not a window of this sequence: no site)
      }
    }
    const unsigned long long has = __ballot(sel);
    if (has == 0) continue;
    // the bases [g0, g0 + C) of the sequence that lie inside it: [a, e), in the words j0 .. j0 + 2 of the sequence
    const int64_t g0 = p - F;
    int64_t a = 0, e = 0, j0 = 0;
    uint64_t W0 = 0, W1 = 0, W2 = 0;
    uint32_t V0 = 0, V1 = 0, V2 = 0;
    if (sel) {
      a = g0 > 0 ? g0 : 0;
      e = g0 + C < L ? g0 + C : L;  // a <= p < p + w <= e
      j0 = a >> 5;
      const int64_t j1 = (e - 1) >> 5;  // <= j0 + 2: e - a <= 64
      const uint64_t w0 = ((uint64_t)offs[i] >> 5) + (uint64_t)j0;
      W0 = words[w0];
      V0 = valid ? valid[w0] : 0xFFFFFFFFu;
      if (j0 + 1 <= j1) {
        W1 = words[w0 + 1];
        V1 = valid ? valid[w0 + 1] : 0xFFFFFFFFu;
      }
      if (j0 + 2 <= j1) {
        W2 = words[w0 + 2];
        V2 = valid ? valid[w0 + 2] : 0xFFFFFFFFu;
      }
    }
    for (int32_t c = 0; c < C; ++c) {
      // column c of the site: base g0 + c on +, g0 + C - 1 - c complemented on -
      const int64_t q = g0 + (strand ? C - 1 - c : c);
      bool ok = false;
      uint32_t b = 0;
      if (sel && q >= a && q < e) {
        const int64_t j = (q >> 5) - j0;
        const uint64_t W = j == 0 ? W0 : (j == 1 ? W1 : W2);
        const uint32_t V = j == 0 ? V0 : (j == 1 ? V1 : V2);
        const uint32_t r = (uint32_t)q & 31u;
        ok = (V >> r) & 1u;
        b = ((uint32_t)(W >> (2 * r)) & 3u) ^ (strand ? 3u : 0u);
      }
      const unsigned long long mo = __ballot(ok), m0 = __ballot(b & 1u), m1 = __ballot(b & 2u);
      if (lane < 5) {
        const unsigned long long mask =
            lane == 4 ? has & ~mo : mo & (lane & 1 ? m0 : ~m0) & (lane & 2 ? m1 : ~m1);
        const uint32_t n = (uint32_t)__popcll(mask);
        if (n) atomicAdd(&bins[c * 5 + lane], n);
      }
    }
  }
  __syncthreads();
  unsigned long long* out = counts + (uint64_t)m * PROF_BINS;
  for (int k = threadIdx.x; k < C * 5; k += PROF_THREADS)
    if (bins[k]) atomicAdd(&out[k], (unsigned long long)bins[k]);
}

// ---- first-order models (--dinuc) --------------------------------------------------------------------
constexpr int PAIR_BINS = PENGK_MAX_MOTIF_LEN * 17;

// site_profile_kernel for adjacent pairs: per motif (blockIdx.y) and column c in (-F, w + F) of its best sites, the
// letters a at c - 1 and b at c, read on the site's strand, ADDED to counts[(m * PENGK_MAX_MOTIF_LEN + c + F) * 17 + 4a + b]
// (bin 16: either position outside the sequence or not A/C/G/T; row 0 stays untouched).  The same wave per 64
// sequences and the same three words per lane; the column's (is a base, base) is kept for the next column.  Per column
// the wave ballots the two bits of a, the two bits of b, "both are bases" and "has a site"; lane l < 16 builds the mask
// of its own bin from them, lane 16 takes the rest, and each of the 17 adds its count once to the block's LDS bins.
__global__ __launch_bounds__(PROF_THREADS) void site_pair_profile_kernel(const uint64_t* __restrict__ words,
                                                                         const uint32_t* __restrict__ valid,
                                                                         const int64_t* __restrict__ offs,
                                                                         const uint32_t* __restrict__ lens, uint64_t n_seq,
                                                                         const int32_t* __restrict__ best,
                                                                         const unsigned long long* __restrict__ site,
                                                                         const int32_t* __restrict__ wtf,
                                                                         unsigned long long* __restrict__ counts) {
  __shared__ uint32_t bins[PAIR_BINS];
  const int m = blockIdx.y;
  const int32_t w = wtf[3 * m], t = wtf[3 * m + 1], F = wtf[3 * m + 2];
  const int32_t C = w + 2 * F;  // <= PENGK_MAX_MOTIF_LEN (the host clamps F)
  for (int k = threadIdx.x; k < PAIR_BINS; k += PROF_THREADS) bins[k] = 0;
  __syncthreads();
  const int32_t* B = best + (uint64_t)m * n_seq;
  const unsigned long long* S = site + (uint64_t)m * n_seq;
  const int lane = threadIdx.x & 63;
  // (every lane of a wave makes the same trips: the ballots below see the whole wave)
  for (uint64_t i0 = blockIdx.x * (uint64_t)PROF_THREADS + (threadIdx.x & ~63); i0 < n_seq;
       i0 += (uint64_t)gridDim.x * PROF_THREADS) {
    const uint64_t i = i0 + lane;
    bool sel = false;
    int64_t L = 0, p = 0;
    int32_t strand = 0;
    if (i < n_seq) {
      const int32_t b = B[i];
      L = lens[i];
      if (b != PENGK_SCORE_SENTINEL && b >= t && L >= w) {
        const uint64_t c = S[i];
        p = (int64_t)(c >> 1);
        strand = (int32_t)(c & 1);
        sel = p <= L - w;  // (not a window of this sequence: no site)
      }
    }
    const unsigned long long has = __ballot(sel);
    if (has == 0) continue;
    // the bases [g0, g0 + C) of the sequence that lie inside it: [a, e), in the words j0 .. j0 + 2 of the sequence
    const int64_t g0 = p - F;
    int64_t a = 0, e = 0, j0 = 0;
    uint64_t W0 = 0, W1 = 0, W2 = 0;
    uint32_t V0 = 0, V1 = 0, V2 = 0;
    if (sel) {
      a = g0 > 0 ? g0 : 0;
      e = g0 + C < L ? g0 + C : L;  // a <= p < p + w <= e
      j0 = a >> 5;
      const int64_t j1 = (e - 1) >> 5;  // <= j0 + 2: e - a <= 64
      const uint64_t w0 = ((uint64_t)offs[i] >> 5) + (uint64_t)j0;
      W0 = words[w0];
      V0 = valid ? valid[w0] : 0xFFFFFFFFu;
      if (j0 + 1 <= j1) {
        W1 = words[w0 + 1];
        V1 = valid ? valid[w0 + 1] : 0xFFFFFFFFu;
      }
      if (j0 + 2 <= j1) {
        W2 = words[w0 + 2];
        V2 = valid ? valid[w0 + 2] : 0xFFFFFFFFu;
      }
    }
    bool pok = false;
    uint32_t pb = 0;
    for (int32_t c = 0; c < C; ++c) {
      // column c of the site: base g0 + c on +, g0 + C - 1 - c complemented on -
      const int64_t q = g0 + (strand ? C - 1 - c : c);
      bool ok = false;
      uint32_t b = 0;
      if (sel && q >= a && q < e) {
        const int64_t j = (q >> 5) - j0;
        const uint64_t W = j == 0 ? W0 : (j == 1 ? W1 : W2);
        const uint32_t V = j == 0 ? V0 : (j == 1 ? V1 : V2);
        const uint32_t r = (uint32_t)q & 31u;
        ok = (V >> r) & 1u;
        b = ((uint32_t)(W >> (2 * r)) & 3u) ^ (strand ? 3u : 0u);
      }
      if (c > 0) {
        const unsigned long long mo = __ballot(ok && pok), a0 = __ballot(pb & 1u), a1 = __ballot(pb & 2u),
                                 b0 = __ballot(b & 1u), b1 = __ballot(b & 2u);
        if (lane < 17) {
          const unsigned long long mask = lane == 16 ? has & ~mo
                                                     : mo & (lane & 4 ? a0 : ~a0) & (lane & 8 ? a1 : ~a1) &
                                                           (lane & 1 ? b0 : ~b0) & (lane & 2 ? b1 : ~b1);
          const uint32_t n = (uint32_t)__popcll(mask);
          if (n) atomicAdd(&bins[c * 17 + lane], n);
        }
      }
      pok = ok;
      pb = b;
    }
  }
  __syncthreads();
  unsigned long long* out = counts + (uint64_t)m * PAIR_BINS;
  for (int k = 17 + threadIdx.x; k < C * 17; k += PROF_THREADS)
    if (bins[k]) atomicAdd(&out[k], (unsigned long long)bins[k]);
}

// The first-order scan: motif_scan_kernel's walk (score.hip) under scan::Order1 tables
template <bool BOTH>
__global__ __launch_bounds__(SCAN_THREADS) void motif_scan_dinuc_kernel(const uint64_t* __restrict__ words,
                                                                        const uint32_t* __restrict__ valid,
                                                                        const int64_t* __restrict__ offs,
                                                                        const uint32_t* __restrict__ lens, uint64_t n_seq,
                                                                        const int32_t* __restrict__ tables,
                                                                        const MotifRec* __restrict__ recs,
                                                                        const GroupRec* __restrict__ groups,
                                                                        int32_t* __restrict__ best_out) {
  __shared__ int32_t tab[SCAN_TABLES * 256];
  __shared__ MotifRec mrec[SCAN_MAX_MOTIFS];
  const GroupRec g = groups[blockIdx.y];
  load_group(g, tables, recs, tab, mrec);
  __syncthreads();
  for (uint64_t i = blockIdx.x * (uint64_t)SCAN_THREADS + threadIdx.x; i < n_seq; i += (uint64_t)gridDim.x * SCAN_THREADS) {
    const uint32_t L = lens[i];
    const uint64_t w0 = (uint64_t)offs[i] >> 5;
    BestVisit<BOTH> v{mrec, best_out, n_seq, i, {}};
    walk_sequence<BOTH, Order1>(words + w0, valid ? valid + w0 : nullptr, L, tab, mrec, g.m1 - g.m0, v);
  }
}

// pengk_site_profiles and (pairs) pengk_site_pair_profiles: the same arguments, checks, clamp and grid
int site_profiles(const char* who, bool pairs, pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid,
                  const int64_t* d_offs, const uint32_t* d_lens, uint64_t n_seq, int n_motifs, const int32_t* d_best,
                  const uint64_t* d_site, const int32_t* h_len, const int32_t* h_thr, int flank, uint64_t* d_counts) {
  if (!ctx || n_motifs < 0 || flank < 0 || (n_motifs && (!h_len || !h_thr || !d_counts)) ||
      (n_seq && n_motifs && (!d_words || !d_offs || !d_lens || !d_best || !d_site)))
    return fail(PENGK_ERR_ARG, "%s: bad argument", who);
  for (int m = 0; m < n_motifs; ++m)
    if (h_len[m] < 1 || h_len[m] > PENGK_MAX_MOTIF_LEN)
      return fail(PENGK_ERR_ARG, "%s: motif %d has width %d (1..%d)", who, m, h_len[m], PENGK_MAX_MOTIF_LEN);
  SCORE_ENTER(ctx);
  if (n_seq == 0 || n_motifs == 0) return PENGK_OK;
  std::vector<int32_t> wtf(3 * (size_t)n_motifs);
  for (int m = 0; m < n_motifs; ++m) {
    wtf[3 * m] = h_len[m];
    wtf[3 * m + 1] = h_thr[m];
    wtf[3 * m + 2] = std::min(flank, (PENGK_MAX_MOTIF_LEN - h_len[m]) / 2);
  }
  int rc = ensure_scratch(ctx, &ctx->d_misc, &ctx->misc_bytes, wtf.size() * sizeof(int32_t));
  if (rc) return rc;
  PENGK_HIP(hipStreamSynchronize(ctx->stream));
  PENGK_HIP(hipMemcpy(ctx->d_misc, wtf.data(), wtf.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  // blocks per motif: enough to fill the device, and so many that a block's 32-bit LDS bins cannot wrap (< 2^31 each)
  const uint64_t need = (n_seq + PROF_THREADS - 1) / PROF_THREADS;
  const uint64_t fill = (uint64_t)ctx->num_cu * 8 / (uint64_t)n_motifs + 1;
  const uint64_t per_motif = std::max<uint64_t>(std::min(need, fill), (n_seq >> 31) + 1);
  const dim3 grid((unsigned)per_motif, (unsigned)n_motifs);
  hipLaunchKernelGGL(pairs ? site_pair_profile_kernel : site_profile_kernel, grid, dim3(PROF_THREADS), 0, ctx->stream, d_words,
                     d_valid, d_offs, d_lens, n_seq, d_best, (const unsigned long long*)d_site, (const int32_t*)ctx->d_misc,
                     (unsigned long long*)d_counts);
  PENGK_HIP(hipGetLastError());
  return PENGK_OK;
}

}  // namespace
}  // namespace pengk

using namespace pengk;

extern "C" {

int pengk_motif_best_sites(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                           const uint32_t* d_lens, uint64_t n_seq, uint64_t seq0, int n_motifs, const int32_t* h_S,
                           const int32_t* h_len, int both_strands, int32_t* d_best, uint64_t* d_site) {
  if (!ctx || n_motifs < 0 || (n_motifs && (!h_S || !h_len)) ||
      (n_seq && n_motifs && (!d_words || !d_offs || !d_lens || !d_best || !d_site)))
    return fail(PENGK_ERR_ARG, "pengk_motif_best_sites: bad argument");
  int rc = check_motifs("pengk_motif_best_sites", n_motifs, h_S, h_len);
  if (rc) return rc;
  SCORE_ENTER(ctx);
  if (n_seq == 0 || n_motifs == 0) return PENGK_OK;
  StagedMotifs st;
  rc = stage_motifs(ctx, n_motifs, h_S, h_len, both_strands ? 2 : 1, nullptr, &st);
  if (rc) return rc;
  const dim3 grid(grid_for(ctx, n_seq, SCAN_THREADS, 8), (unsigned)st.n_groups);
  unsigned long long* site = (unsigned long long*)d_site;
  by_strands(both_strands, [&](auto B) {
    hipLaunchKernelGGL(motif_best_site_kernel<decltype(B)::value>, grid, dim3(SCAN_THREADS), 0, ctx->stream, d_words, d_valid,
                       d_offs, d_lens, n_seq, seq0, st.tables, st.recs, st.groups, d_best, site);
  });
  PENGK_HIP(hipGetLastError());
  return PENGK_OK;
}

int pengk_centrality_histograms(pengk_ctx* ctx, int n_motifs, const int32_t* d_best, const uint64_t* d_site,
                                const uint32_t* d_lens, uint64_t n_seq, const int32_t* h_len, const int32_t* h_thr,
                                uint32_t max_len, uint64_t* d_hist_offsets, uint64_t* d_hist_lengths) {
  if (!ctx || n_motifs < 0 || max_len < 1 || max_len > PENGK_CENTRALITY_MAX_LEN ||
      (n_motifs && (!h_len || !h_thr || !d_hist_offsets || !d_hist_lengths)) || (n_seq && n_motifs && (!d_best || !d_site || !d_lens)))
    return fail(PENGK_ERR_ARG, "pengk_centrality_histograms: bad argument");
  for (int m = 0; m < n_motifs; ++m)
    if (h_len[m] < 1 || h_len[m] > PENGK_MAX_MOTIF_LEN)
      return fail(PENGK_ERR_ARG, "pengk_centrality_histograms: motif %d has width %d (1..%d)", m, h_len[m], PENGK_MAX_MOTIF_LEN);
  SCORE_ENTER(ctx);
  if (n_seq == 0 || n_motifs == 0) return PENGK_OK;
  std::vector<int32_t> wt(2 * (size_t)n_motifs);
  for (int m = 0; m < n_motifs; ++m) {
    wt[2 * m] = h_len[m];
    wt[2 * m + 1] = h_thr[m];
  }
  int rc = ensure_scratch(ctx, &ctx->d_misc, &ctx->misc_bytes, wt.size() * sizeof(int32_t));
  if (rc) return rc;
  PENGK_HIP(hipStreamSynchronize(ctx->stream));
  PENGK_HIP(hipMemcpy(ctx->d_misc, wt.data(), wt.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  const uint64_t per_motif = std::max<uint64_t>(1, std::min<uint64_t>((n_seq + HIST_THREADS - 1) / HIST_THREADS,
                                                                      (uint64_t)ctx->num_cu * 2 / (uint64_t)n_motifs + 1));
  const dim3 grid((unsigned)per_motif, (unsigned)n_motifs);
  const bool lds = 3ull * max_len + 2 <= (uint64_t)CENT_LDS_BINS && n_seq >= (uint64_t)HIST_THREADS * 16;
  const unsigned long long* site = (const unsigned long long*)d_site;
  unsigned long long* hd = (unsigned long long*)d_hist_offsets;
  unsigned long long* hl = (unsigned long long*)d_hist_lengths;
  if (lds)
    hipLaunchKernelGGL(centrality_hist_kernel<true>, grid, dim3(HIST_THREADS), 0, ctx->stream, d_best, site, d_lens, n_seq,
                       (const int32_t*)ctx->d_misc, max_len, hd, hl);
  else
    hipLaunchKernelGGL(centrality_hist_kernel<false>, grid, dim3(HIST_THREADS), 0, ctx->stream, d_best, site, d_lens, n_seq,
                       (const int32_t*)ctx->d_misc, max_len, hd, hl);
  PENGK_HIP(hipGetLastError());
  return PENGK_OK;
}

int pengk_spacing_histograms(pengk_ctx* ctx, int n_motifs, const int32_t* d_best, const uint64_t* d_site,
                             const uint32_t* d_lens, uint64_t n_seq, const int32_t* h_len, const int32_t* h_thr,
                             uint32_t max_gap, uint32_t min_len, uint32_t max_len, uint64_t* d_hist_gaps,
                             uint64_t* d_hist_lengths, uint64_t* d_hist_motifs) {
  if (!ctx || n_motifs < 0 || (n_motifs && (!h_len || !h_thr || !d_hist_motifs)) ||
      (n_motifs > 1 && (!d_hist_gaps || !d_hist_lengths)) || (n_seq && n_motifs && (!d_best || !d_site || !d_lens)))
    return fail(PENGK_ERR_ARG, "pengk_spacing_histograms: bad argument");
  if (n_motifs > PENGK_SPACING_MAX_MOTIFS)
    return fail(PENGK_ERR_ARG, "pengk_spacing_histograms: %d motifs (at most %d)", n_motifs, PENGK_SPACING_MAX_MOTIFS);
  if (max_gap > PENGK_SPACING_MAX_GAP)
    return fail(PENGK_ERR_ARG, "pengk_spacing_histograms: max_gap %u (at most %d)", max_gap, PENGK_SPACING_MAX_GAP);
  if (max_len < 1 || max_len > PENGK_CENTRALITY_MAX_LEN)
    return fail(PENGK_ERR_ARG, "pengk_spacing_histograms: max_len %u (1..%d)", max_len, PENGK_CENTRALITY_MAX_LEN);
  for (int m = 0; m < n_motifs; ++m) {
    if (h_len[m] < 1 || h_len[m] > PENGK_MAX_MOTIF_LEN)
      return fail(PENGK_ERR_ARG, "pengk_spacing_histograms: motif %d has width %d (1..%d)", m, h_len[m], PENGK_MAX_MOTIF_LEN);
    if (min_len < (uint32_t)h_len[m])
      return fail(PENGK_ERR_ARG, "pengk_spacing_histograms: min_len %u below the width %d of motif %d", min_len, h_len[m], m);
  }
  SCORE_ENTER(ctx);
  if (n_seq == 0 || n_motifs == 0) return PENGK_OK;
  // LDS bins when a pair's bins fit and the input is large enough for a block to add to a bin more than once; a motif
  // with more earlier motifs than fit gets several rows.  Else one row per motif, global bins.
  const uint64_t per = 4ull * (max_gap + 1) + 2 + (uint64_t)max_len + 1;
  const bool lds = per <= (uint64_t)SPACE_LDS_BINS && n_seq >= (uint64_t)SPACE_THREADS * 16;
  const int fit = lds ? (int)((uint64_t)SPACE_LDS_BINS / per) : PENGK_SPACING_MAX_MOTIFS;
  std::vector<SpaceRow> rows;
  for (int b = 0; b < n_motifs; ++b)
    for (int a0 = 0; a0 == 0 || a0 < b; a0 += fit) rows.push_back(SpaceRow{b, a0, std::min(b, a0 + fit), 0});
  const size_t wb = 2 * (size_t)n_motifs * sizeof(int32_t);  // (a multiple of 8: the rows are 16 bytes each)
  std::vector<char> staged(wb + rows.size() * sizeof(SpaceRow));
  int32_t* wt = (int32_t*)staged.data();
  for (int m = 0; m < n_motifs; ++m) {
    wt[2 * m] = h_len[m];
    wt[2 * m + 1] = h_thr[m];
  }
  memcpy(staged.data() + wb, rows.data(), rows.size() * sizeof(SpaceRow));
  int rc = ensure_scratch(ctx, &ctx->d_misc, &ctx->misc_bytes, staged.size());
  if (rc) return rc;
  PENGK_HIP(hipStreamSynchronize(ctx->stream));
  PENGK_HIP(hipMemcpy(ctx->d_misc, staged.data(), staged.size(), hipMemcpyHostToDevice));
  // blocks per row: four per CU over all rows, and enough that no block's uint32 bin can wrap
  const uint64_t blocks = (n_seq + SPACE_THREADS - 1) / SPACE_THREADS;
  const uint64_t per_row = std::max<uint64_t>(std::min<uint64_t>(blocks, (uint64_t)ctx->num_cu * 4 / rows.size() + 1), (n_seq >> 31) + 1);
  const dim3 grid((unsigned)per_row, (unsigned)rows.size());
  const int32_t* d_wt = (const int32_t*)ctx->d_misc;
  const SpaceRow* d_rows = (const SpaceRow*)((const char*)ctx->d_misc + wb);
  const unsigned long long* site = (const unsigned long long*)d_site;
  unsigned long long* hg = (unsigned long long*)d_hist_gaps;
  unsigned long long* hl = (unsigned long long*)d_hist_lengths;
  unsigned long long* hm = (unsigned long long*)d_hist_motifs;
  if (lds)
    hipLaunchKernelGGL(spacing_hist_kernel<true>, grid, dim3(SPACE_THREADS), 0, ctx->stream, d_best, site, d_lens, n_seq, d_wt,
                       d_rows, max_gap, min_len, max_len, hg, hl, hm);
  else
    hipLaunchKernelGGL(spacing_hist_kernel<false>, grid, dim3(SPACE_THREADS), 0, ctx->stream, d_best, site, d_lens, n_seq, d_wt,
                       d_rows, max_gap, min_len, max_len, hg, hl, hm);
  PENGK_HIP(hipGetLastError());
  return PENGK_OK;
}

int pengk_site_profiles(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                        const uint32_t* d_lens, uint64_t n_seq, int n_motifs, const int32_t* d_best, const uint64_t* d_site,
                        const int32_t* h_len, const int32_t* h_thr, int flank, uint64_t* d_counts) {
  return site_profiles("pengk_site_profiles", false, ctx, d_words, d_valid, d_offs, d_lens, n_seq, n_motifs, d_best, d_site, h_len,
                       h_thr, flank, d_counts);
}

int pengk_site_pair_profiles(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                             const uint32_t* d_lens, uint64_t n_seq, int n_motifs, const int32_t* d_best, const uint64_t* d_site,
                             const int32_t* h_len, const int32_t* h_thr, int flank, uint64_t* d_counts) {
  return site_profiles("pengk_site_pair_profiles", true, ctx, d_words, d_valid, d_offs, d_lens, n_seq, n_motifs, d_best, d_site,
                       h_len, h_thr, flank, d_counts);
}

int pengk_motif_scan_dinuc(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                           const uint32_t* d_lens, uint64_t n_seq, int n_motifs, const int32_t* h_S0, const int32_t* h_D,
                           const int32_t* h_len, int both_strands, int32_t* d_best) {
  if (!ctx || n_motifs < 0 || (n_motifs && (!h_S0 || !h_D || !h_len)) ||
      (n_seq && n_motifs && (!d_words || !d_offs || !d_lens || !d_best)))
    return fail(PENGK_ERR_ARG, "pengk_motif_scan_dinuc: bad argument");
  for (int m = 0; m < n_motifs; ++m) {
    if (h_len[m] < 1 || h_len[m] > PENGK_MAX_MOTIF_LEN)
      return fail(PENGK_ERR_ARG, "pengk_motif_scan_dinuc: motif %d has width %d (1..%d)", m, h_len[m], PENGK_MAX_MOTIF_LEN);
    for (int j = 0; j < 4; ++j) {
      const int32_t v = h_S0[(size_t)m * 4 + j];
      if (v < -2000 || v > 2000) return fail(PENGK_ERR_ARG, "pengk_motif_scan_dinuc: motif %d: log-odds %d outside [-2000, 2000]", m, v);
    }
    for (int j = 16; j < h_len[m] * 16; ++j) {
      const int32_t v = h_D[(size_t)m * PENGK_MAX_MOTIF_LEN * 16 + j];
      if (v < -2000 || v > 2000) return fail(PENGK_ERR_ARG, "pengk_motif_scan_dinuc: motif %d: log-odds %d outside [-2000, 2000]", m, v);
    }
  }
  SCORE_ENTER(ctx);
  if (n_seq == 0 || n_motifs == 0) return PENGK_OK;
  StagedMotifs st;
  int rc = stage_motifs_dinuc(ctx, n_motifs, h_S0, h_D, h_len, both_strands ? 2 : 1, &st);
  if (rc) return rc;
  const dim3 grid(grid_for(ctx, n_seq, SCAN_THREADS, 8), (unsigned)st.n_groups);
  by_strands(both_strands, [&](auto B) {
    hipLaunchKernelGGL(motif_scan_dinuc_kernel<decltype(B)::value>, grid, dim3(SCAN_THREADS), 0, ctx->stream, d_words, d_valid,
                       d_offs, d_lens, n_seq, st.tables, st.recs, st.groups, d_best);
  });
  PENGK_HIP(hipGetLastError());
  return PENGK_OK;
}

}  // extern "C"
