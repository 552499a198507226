// sites.hip -- the walks of the scan layout that count, emit and bin motif sites (scan_walk.h; the motifs staged by score.hip).
//
//   sites          (--sites) the scan's walk with per-motif thresholds: a count pass, block totals that cut
//                  the sequences into slices of bounded records, an exclusive scan of a slice's counts and an emit pass
//                  that writes every site at its place
//   q-values       (--sites-qvalue) the count pass with every site binned by its score
//   enrichment     (--enrich) the scan with a sequence's best score kept in a register and binned where it
//                  stands, for a whole motif database: nothing of size motifs x sequences; Fisher's exact tail on the host
// The summaries of these histograms are host code: score_stats.cpp.
#include <string.h>

#include <algorithm>
#include <vector>

#include "pengk_internal.h"
#include "scan_walk.h"

namespace pengk {
using namespace scan;  // the shared walk and its records (scan_walk.h)
namespace {

// ---- motif sites (pengk_sites_*): every window strand at or above a motif's threshold, in a fixed order --------------
constexpr int SITES_THREADS = 256;
constexpr uint32_t SITES_BLOCK = PENGK_SITES_BLOCK;  // sequences per block total of pengk_sites_slices
constexpr int XS_PER = 8;                            // offsets scan: elements per thread ...
constexpr int XS_TILE = SITES_THREADS * XS_PER;      // ... and per workgroup

// sites of every motif on every sequence: counts[m * n_seq + i] (uint64: 2 per window of a 2^32-base sequence)
template <bool BOTH>
struct CountVisit {
  const MotifRec* mrec;
  const int32_t* thr;  // by group record
  unsigned long long* counts;
  uint64_t n_seq, i;
  int32_t t[SCAN_PASS];
  unsigned long long c[SCAN_PASS];
  __device__ __forceinline__ void begin(int q, int r) {
    t[q] = thr[r];
    c[q] = 0;
  }
  __device__ __forceinline__ void window(int q, uint32_t, int32_t sf, int32_t sr) {
    c[q] += (unsigned)(sf >= t[q]) + (unsigned)(BOTH && sr >= t[q]);
  }
  __device__ __forceinline__ void end(int q, int r) { counts[(uint64_t)mrec[r].m * n_seq + i] = c[q]; }
};

// the records of sequences [i0, i1): sequence i's sites of motif m from d_so[m * (i1 - i0) + i - i0] on, in window order,
// + before -; a record at or beyond cap is not written (the caller sized cap from the counts: none is)
template <bool BOTH>
struct EmitVisit {
  const MotifRec* mrec;
  const int32_t* thr;
  const unsigned long long* so;
  pengk_site* out;
  uint64_t cap, ns, i, il;
  int32_t t[SCAN_PASS];
  uint64_t o[SCAN_PASS];
  uint32_t ms[SCAN_PASS];
  __device__ __forceinline__ void begin(int q, int r) {
    t[q] = thr[r];
    o[q] = so[(uint64_t)mrec[r].m * ns + il];
    ms[q] = (uint32_t)mrec[r].m << 1;
  }
  __device__ __forceinline__ void put(int q, uint32_t pos, int32_t sc, uint32_t strand) {
    if (o[q] < cap) {
      pengk_site rec;
      rec.seq = (uint32_t)il;
      rec.pos = pos;
      rec.score = sc;
      rec.motif_strand = ms[q] | strand;
      out[o[q]] = rec;
    }
    ++o[q];
  }
  __device__ __forceinline__ void window(int q, uint32_t pos, int32_t sf, int32_t sr) {
    if (sf >= t[q]) put(q, pos, sf, 0u);
    if (BOTH && sr >= t[q]) put(q, pos, sr, 1u);
  }
  __device__ __forceinline__ void end(int, int) {}
};

// one kernel for both passes: the shared walk, the visitor's state per sequence
template <bool BOTH, bool EMIT>
__global__ __launch_bounds__(SCAN_THREADS) void motif_sites_kernel(const uint64_t* __restrict__ words,
                                                                   const uint32_t* __restrict__ valid,
                                                                   const int64_t* __restrict__ offs,
                                                                   const uint32_t* __restrict__ lens, uint64_t i0, uint64_t i1,
                                                                   uint64_t n_seq, const int32_t* __restrict__ tables,
                                                                   const MotifRec* __restrict__ recs,
                                                                   const GroupRec* __restrict__ groups,
                                                                   const int32_t* __restrict__ thr,
                                                                   unsigned long long* __restrict__ counts,
                                                                   const unsigned long long* __restrict__ so,
                                                                   pengk_site* __restrict__ out, uint64_t cap) {
  __shared__ int32_t tab[SCAN_TABLES * 256];
  __shared__ MotifRec mrec[SCAN_MAX_MOTIFS];
  __shared__ int32_t mthr[SCAN_MAX_MOTIFS];
  const GroupRec g = groups[blockIdx.y];
  load_group(g, tables, recs, tab, mrec, [&](int t, const MotifRec& mr) { mthr[t] = thr[mr.m]; });
  __syncthreads();
  for (uint64_t i = i0 + blockIdx.x * (uint64_t)SCAN_THREADS + threadIdx.x; i < i1; i += (uint64_t)gridDim.x * SCAN_THREADS) {
    const uint32_t L = lens[i];
    const uint64_t w0 = (uint64_t)offs[i] >> 5;
    if (EMIT) {
      EmitVisit<BOTH> v{mrec, mthr, so, out, cap, i1 - i0, i, i - i0, {}, {}, {}};
      walk_sequence<BOTH>(words + w0, valid ? valid + w0 : nullptr, L, tab, mrec, g.m1 - g.m0, v);
    } else {
      CountVisit<BOTH> v{mrec, mthr, counts, n_seq, i, {}, {}};
      walk_sequence<BOTH>(words + w0, valid ? valid + w0 : nullptr, L, tab, mrec, g.m1 - g.m0, v);
    }
  }
}

// inclusive sum over the workgroup (sh: SITES_THREADS entries; every thread calls it)
__device__ __forceinline__ unsigned long long block_inclusive_sum(unsigned long long v, unsigned long long* sh,
                                                                  unsigned long long* total = nullptr) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int d = 1; d < SITES_THREADS; d <<= 1) {
    const unsigned long long x = t >= d ? sh[t - d] : 0ull;
    __syncthreads();
    sh[t] += x;
    __syncthreads();
  }
  const unsigned long long r = sh[t];
  if (total) *total = sh[SITES_THREADS - 1];
  __syncthreads();
  return r;
}

// per-sequence totals over the motifs, per-block totals (SITES_BLOCK sequences) and per-motif totals (added to mtot)
__global__ __launch_bounds__(SITES_THREADS) void site_totals_kernel(const unsigned long long* __restrict__ counts, uint64_t n_seq,
                                                                   int n_motifs, unsigned long long* __restrict__ seq_tot,
                                                                   unsigned long long* __restrict__ block_tot,
                                                                   unsigned long long* __restrict__ mtot) {
  __shared__ unsigned long long sh[SITES_THREADS];
  constexpr int PER = SITES_BLOCK / SITES_THREADS;
  const uint64_t base = (uint64_t)blockIdx.x * SITES_BLOCK;
  unsigned long long st[PER];
#pragma unroll
  for (int r = 0; r < PER; ++r) st[r] = 0;
  for (int m = 0; m < n_motifs; ++m) {
    unsigned long long ms = 0;
#pragma unroll
    for (int r = 0; r < PER; ++r) {
      const uint64_t i = base + (uint64_t)r * SITES_THREADS + threadIdx.x;
      if (i < n_seq) {
        const unsigned long long c = counts[(uint64_t)m * n_seq + i];
        st[r] += c;
        ms += c;
      }
    }
    ms = block_inclusive_sum(ms, sh);
    if (threadIdx.x == SITES_THREADS - 1 && ms) atomicAdd(&mtot[m], ms);
  }
  unsigned long long bs = 0;
#pragma unroll
  for (int r = 0; r < PER; ++r) {
    const uint64_t i = base + (uint64_t)r * SITES_THREADS + threadIdx.x;
    if (i < n_seq) seq_tot[i] = st[r];
    bs += st[r];
  }
  bs = block_inclusive_sum(bs, sh);
  if (threadIdx.x == SITES_THREADS - 1) block_tot[blockIdx.x] = bs;
}

// exclusive scan of the counts of sequences [i0, i0 + ns), motif-major: element k = counts[(k / ns) * n_seq + i0 + k % ns]
__device__ __forceinline__ unsigned long long xs_elem(const unsigned long long* counts, uint64_t n_seq, uint64_t i0, uint64_t ns,
                                                      uint64_t k) {
  return counts[(k / ns) * n_seq + i0 + k % ns];
}

__global__ __launch_bounds__(SITES_THREADS) void xscan_tiles_kernel(const unsigned long long* __restrict__ counts, uint64_t n_seq,
                                                                    uint64_t i0, uint64_t ns, uint64_t n,
                                                                    unsigned long long* __restrict__ part) {
  __shared__ unsigned long long sh[SITES_THREADS];
  const uint64_t k0 = (uint64_t)blockIdx.x * XS_TILE + (uint64_t)threadIdx.x * XS_PER;
  unsigned long long s = 0;
  for (int r = 0; r < XS_PER; ++r)
    if (k0 + r < n) s += xs_elem(counts, n_seq, i0, ns, k0 + r);
  s = block_inclusive_sum(s, sh);
  if (threadIdx.x == SITES_THREADS - 1) part[blockIdx.x] = s;
}

// (one workgroup) the tiles' sums -> their exclusive prefix sums, in place
__global__ __launch_bounds__(SITES_THREADS) void xscan_parts_kernel(unsigned long long* __restrict__ part, uint64_t n_tiles) {
  __shared__ unsigned long long sh[SITES_THREADS];
  unsigned long long carry = 0;
  for (uint64_t b = 0; b < n_tiles; b += XS_TILE) {
    unsigned long long v[XS_PER], s = 0;
    const uint64_t k0 = b + (uint64_t)threadIdx.x * XS_PER;
    for (int r = 0; r < XS_PER; ++r) {
      v[r] = k0 + r < n_tiles ? part[k0 + r] : 0ull;
      s += v[r];
    }
    unsigned long long tot = 0;
    unsigned long long e = carry + block_inclusive_sum(s, sh, &tot) - s;
    for (int r = 0; r < XS_PER; ++r) {
      if (k0 + r < n_tiles) part[k0 + r] = e;
      e += v[r];
    }
    carry += tot;
  }
}

__global__ __launch_bounds__(SITES_THREADS) void xscan_apply_kernel(const unsigned long long* __restrict__ counts, uint64_t n_seq,
                                                                    uint64_t i0, uint64_t ns, uint64_t n,
                                                                    const unsigned long long* __restrict__ part,
                                                                    unsigned long long* __restrict__ out) {
  __shared__ unsigned long long sh[SITES_THREADS];
  const uint64_t k0 = (uint64_t)blockIdx.x * XS_TILE + (uint64_t)threadIdx.x * XS_PER;
  unsigned long long v[XS_PER], s = 0;
  for (int r = 0; r < XS_PER; ++r) {
    v[r] = k0 + r < n ? xs_elem(counts, n_seq, i0, ns, k0 + r) : 0ull;
    s += v[r];
  }
  unsigned long long e = part[blockIdx.x] + block_inclusive_sum(s, sh) - s;
  for (int r = 0; r < XS_PER; ++r) {
    if (k0 + r < n) out[k0 + r] = e;
    e += v[r];
  }
}

// ---- private bins: what the q-value and the enrichment kernel share ----------------------------------------------------
constexpr int QH_PRIV_BINS = 2560;          // workgroup-private 32-bit bins (10 KiB), shared evenly by the group's motifs
constexpr uint32_t QH_LONG_SEQ = 1u << 16;  // a longer sequence adds to the global bins only
constexpr int QH_FLUSH_TRIPS = 64;          // trips of the workgroup's sequence loop between two flushes of the private bins

// The record of motif mr.m (HistRec, EnrichRec): its global bins (bin 0 = the threshold), its threshold and the lowest
// score with a private bin.  The private bins: scores (hi - per, hi], none below the threshold (hi >= every score: the
// host checked it).
template <class Rec>
__device__ __forceinline__ Rec private_rec(const MotifRec& mr, int per, const int32_t* __restrict__ thr,
                                           const int32_t* __restrict__ hi, const uint64_t* __restrict__ hoffs,
                                           unsigned long long* __restrict__ hist) {
  const int64_t tp = (int64_t)hi[mr.m] - per + 1;
  Rec r{};
  r.H = hist + hoffs[mr.m];
  r.thr = thr[mr.m];
  r.top = tp > (int64_t)r.thr ? (int32_t)tp : r.thr;
  return r;
}

// The private bins added to the global ones (every thread of the workgroup, behind a barrier).  Private bin k of record
// k / per holds score top + k % per: bin top - thr + k % per of the motif (a bin above hi - thr is never added to and
// stays 0).  CLEAR: the bins are used again.
template <bool CLEAR, class Rec>
__device__ __forceinline__ void flush_private(uint32_t* priv, const Rec* rec, int nrec, int per) {
  for (int k = threadIdx.x; k < nrec * per; k += SCAN_THREADS) {
    const uint32_t n = priv[k];
    if (n) {
      const int rr = k / per;
      atomicAdd(&rec[rr].H[(int64_t)rec[rr].top - rec[rr].thr + (k - rr * per)], (unsigned long long)n);
      if (CLEAR) priv[k] = 0;
    }
  }
}

// ---- site histograms (pengk_sites_histograms: the ranks behind --sites-qvalue) -------------------------
// Per motif of the group: the global bins (bin 0 = the threshold), the lowest score with a private bin, the scored
// window strands of the workgroup.
struct HistRec {
  unsigned long long* H;
  unsigned long long tests;
  int32_t thr, top;
};

// A fourth visitor: every site adds 1 to its motif's bin score - t, every valid window counts as one or two scored
// strands, and the per-(motif, sequence) site count is CountVisit's.  The top `per` scores of each motif of the group
// (where a motif that sits in every sequence sends its sites) have a workgroup-private 32-bit bin in LDS; a lower score
// adds to the global uint64 bin directly.
// No private bin can wrap: a thread adds to it only for a sequence of at most QH_LONG_SEQ = 2^16 bases, so at most 2^17
// times per trip of the workgroup's loop (one sequence per thread and trip, two strands per window); 256 threads and
// QH_FLUSH_TRIPS = 64 trips between two flushes bound a bin by 2^8 * 2^17 * 2^6 = 2^31 < 2^32.  A longer sequence (up to
// 2^33 window strands) gets top = INT32_MAX, which no score reaches: all its sites go to the global bins.
template <bool BOTH>
struct HistVisit {
  const MotifRec* mrec;
  HistRec* hrec;
  uint32_t* priv;
  unsigned long long* counts;  // NULL: not stored
  uint64_t n_seq, i;
  int per;
  bool short_seq;
  int32_t t[SCAN_PASS], top[SCAN_PASS], pb[SCAN_PASS], r[SCAN_PASS];
  uint32_t nw[SCAN_PASS];
  unsigned long long c[SCAN_PASS];
  __device__ __forceinline__ void begin(int q, int rr) {
    r[q] = rr;
    t[q] = hrec[rr].thr;
    top[q] = short_seq ? hrec[rr].top : INT32_MAX;
    pb[q] = rr * per - hrec[rr].top;  // private bin of score s: priv[pb + s], in [rr * per, (rr + 1) * per) for top <= s <= hi
    nw[q] = 0;
    c[q] = 0;
  }
  __device__ __forceinline__ void bump(int q, int32_t sc) {
    if (sc >= top[q]) atomicAdd(&priv[pb[q] + sc], 1u);
    else atomicAdd(&hrec[r[q]].H[(int64_t)sc - t[q]], 1ull);
    ++c[q];
  }
  __device__ __forceinline__ void window(int q, uint32_t, int32_t sf, int32_t sr) {
    ++nw[q];
    if (sf >= t[q]) bump(q, sf);
    if (BOTH && sr >= t[q]) bump(q, sr);
  }
  __device__ __forceinline__ void end(int q, int rr) {
    if (nw[q]) atomicAdd(&hrec[rr].tests, (unsigned long long)nw[q] * (BOTH ? 2u : 1u));
    if (counts) counts[(uint64_t)mrec[rr].m * n_seq + i] = c[q];
  }
};

// a kernel of its own: the count pass of --sites keeps its code when q-values are not asked for
template <bool BOTH>
__global__ __launch_bounds__(SCAN_THREADS) void motif_sites_hist_kernel(const uint64_t* __restrict__ words,
                                                                        const uint32_t* __restrict__ valid,
                                                                        const int64_t* __restrict__ offs,
                                                                        const uint32_t* __restrict__ lens, uint64_t n_seq,
                                                                        const int32_t* __restrict__ tables,
                                                                        const MotifRec* __restrict__ recs,
                                                                        const GroupRec* __restrict__ groups,
                                                                        const int32_t* __restrict__ thr,
                                                                        const int32_t* __restrict__ hi,
                                                                        const uint64_t* __restrict__ hoffs,
                                                                        unsigned long long* __restrict__ hist,
                                                                        unsigned long long* __restrict__ tests,
                                                                        unsigned long long* __restrict__ counts) {
  __shared__ int32_t tab[SCAN_TABLES * 256];
  __shared__ MotifRec mrec[SCAN_MAX_MOTIFS];
  __shared__ HistRec hrec[SCAN_MAX_MOTIFS];
  __shared__ uint32_t priv[QH_PRIV_BINS];
  const GroupRec g = groups[blockIdx.y];
  const int nrec = g.m1 - g.m0;
  const int per = QH_PRIV_BINS / nrec;  // (1 <= nrec <= SCAN_MAX_MOTIFS: at least 64 bins each)
  load_group(g, tables, recs, tab, mrec,
             [&](int t, const MotifRec& mr) { hrec[t] = private_rec<HistRec>(mr, per, thr, hi, hoffs, hist); });
  for (int t = threadIdx.x; t < QH_PRIV_BINS; t += SCAN_THREADS) priv[t] = 0;
  __syncthreads();
  // (every thread of the workgroup makes the same trips: the flush inside the loop is reached by all of them)
  int trips = 0;
  for (uint64_t ib = blockIdx.x * (uint64_t)SCAN_THREADS; ib < n_seq; ib += (uint64_t)gridDim.x * SCAN_THREADS) {
    const uint64_t i = ib + threadIdx.x;
    if (i < n_seq) {
      const uint32_t L = lens[i];
      const uint64_t w0 = (uint64_t)offs[i] >> 5;
      HistVisit<BOTH> v{mrec, hrec, priv, counts, n_seq, i, per, L <= QH_LONG_SEQ, {}, {}, {}, {}, {}, {}};
      walk_sequence<BOTH>(words + w0, valid ? valid + w0 : nullptr, L, tab, mrec, nrec, v);
    }
    if (++trips == QH_FLUSH_TRIPS) {
      __syncthreads();
      flush_private<true>(priv, hrec, nrec, per);
      __syncthreads();
      trips = 0;
    }
  }
  __syncthreads();
  flush_private<true>(priv, hrec, nrec, per);
  // the scored window strands: one global atomic per motif and workgroup
  for (int t = threadIdx.x; t < nrec; t += SCAN_THREADS)
    if (hrec[t].tests) atomicAdd(&tests[mrec[t].m], hrec[t].tests);
}

// ---- database enrichment (pengk_motif_enrich: the histograms behind --enrich) ----------------------------
// Per motif of the group: the global bins (bin 0 = the threshold) and the lowest score with a private bin.
struct EnrichRec {
  unsigned long long* H;
  int32_t thr, top;
};

// A fifth visitor: BestVisit's register maximum, binned where it stands instead of stored.  The window loop is
// BestVisit's (a score is above PENGK_SCORE_SENTINEL, so the maximum itself says whether there was a window); per
// (motif, sequence) the end adds the sequence to the motif's scored counter -- one 32-bit LDS add per wave: the lanes
// that are here together are counted by a ballot, and a lane that is not counts itself the same way -- and, at or above
// the threshold, 1 to the bin of the best score: a private 32-bit LDS bin for the top `per` scores (HistVisit's
// arrangement), the global uint64 bin below them.
// No private bin or counter can wrap and none is flushed inside the loop: a sequence adds at most once per motif and
// the host refuses n_seq >= 2^32.
template <bool BOTH>
struct EnrichVisit {
  const EnrichRec* erec;
  uint32_t* priv;
  uint32_t* scored;
  int per;
  int best[SCAN_PASS];
  __device__ __forceinline__ void begin(int q, int) { best[q] = PENGK_SCORE_SENTINEL; }
  __device__ __forceinline__ void window(int q, uint32_t, int32_t sf, int32_t sr) { best[q] = max(best[q], BOTH ? max(sf, sr) : sf); }
  __device__ __forceinline__ void end(int q, int rr) {
    const int32_t b = best[q];
    const bool had = b != PENGK_SCORE_SENTINEL;
    const unsigned long long here = __ballot(1), hm = __ballot(had);
    if (hm && (int)__lane_id() == __ffsll((long long)here) - 1) atomicAdd(&scored[rr], (uint32_t)__popcll(hm));
    if (!had) return;
    const EnrichRec e = erec[rr];
    if (b < e.thr) return;
    if (b >= e.top) atomicAdd(&priv[rr * per + (b - e.top)], 1u);
    else atomicAdd(&e.H[(int64_t)b - e.thr], 1ull);
  }
};

template <bool BOTH>
__global__ __launch_bounds__(SCAN_THREADS) void motif_enrich_kernel(const uint64_t* __restrict__ words,
                                                                    const uint32_t* __restrict__ valid,
                                                                    const int64_t* __restrict__ offs,
                                                                    const uint32_t* __restrict__ lens, uint64_t n_seq,
                                                                    const int32_t* __restrict__ tables,
                                                                    const MotifRec* __restrict__ recs,
                                                                    const GroupRec* __restrict__ groups,
                                                                    const int32_t* __restrict__ thr,
                                                                    const int32_t* __restrict__ hi,
                                                                    const uint64_t* __restrict__ hoffs,
                                                                    unsigned long long* __restrict__ hist,
                                                                    unsigned long long* __restrict__ scored_out) {
  __shared__ int32_t tab[SCAN_TABLES * 256];
  __shared__ MotifRec mrec[SCAN_MAX_MOTIFS];
  __shared__ EnrichRec erec[SCAN_MAX_MOTIFS];
  __shared__ uint32_t scored[SCAN_MAX_MOTIFS];
  __shared__ uint32_t priv[QH_PRIV_BINS];
  const GroupRec g = groups[blockIdx.y];
  const int nrec = g.m1 - g.m0;
  const int per = QH_PRIV_BINS / nrec;  // (1 <= nrec <= SCAN_MAX_MOTIFS: at least 64 bins each)
  load_group(g, tables, recs, tab, mrec, [&](int t, const MotifRec& mr) {
    erec[t] = private_rec<EnrichRec>(mr, per, thr, hi, hoffs, hist);
    scored[t] = 0;
  });
  for (int t = threadIdx.x; t < QH_PRIV_BINS; t += SCAN_THREADS) priv[t] = 0;
  __syncthreads();
  for (uint64_t i = blockIdx.x * (uint64_t)SCAN_THREADS + threadIdx.x; i < n_seq; i += (uint64_t)gridDim.x * SCAN_THREADS) {
    const uint32_t L = lens[i];
    const uint64_t w0 = (uint64_t)offs[i] >> 5;
    EnrichVisit<BOTH> v{erec, priv, scored, per, {}};
    walk_sequence<BOTH>(words + w0, valid ? valid + w0 : nullptr, L, tab, mrec, nrec, v);
  }
  __syncthreads();
  flush_private<false>(priv, erec, nrec, per);
  // the scored sequences: one global atomic per motif and workgroup
  for (int t = threadIdx.x; t < nrec; t += SCAN_THREADS)
    if (scored[t]) atomicAdd(&scored_out[mrec[t].m], (unsigned long long)scored[t]);
}

// every score must have its bin: h_hi[m] at or above the sum of the column maxima, and bins to add to
int check_hist_range(const char* who, int n_motifs, const int32_t* h_S, const int32_t* h_len, const int32_t* h_thr,
                     const int32_t* h_hi, const uint64_t* d_hist) {
  for (int m = 0; m < n_motifs; ++m) {
    int32_t mx = 0;
    for (int j = 0; j < h_len[m]; ++j) {
      const int32_t* c = h_S + ((size_t)m * PENGK_MAX_MOTIF_LEN + j) * 4;
      mx += std::max(std::max(c[0], c[1]), std::max(c[2], c[3]));
    }
    if (h_hi[m] < mx) return fail(PENGK_ERR_ARG, "%s: motif %d: hi %d below its best score %d", who, m, h_hi[m], mx);
    if (h_hi[m] >= h_thr[m] && !d_hist) return fail(PENGK_ERR_ARG, "%s: bad argument", who);
  }
  return PENGK_OK;
}

// The motifs of a histogram launch staged: stage_motifs, and h_hi | h_hist_offs (the offsets from an 8-byte boundary) in
// ctx->d_misc.  The scratch is sized before stage_motifs synchronises with the stream and filled behind it.
int stage_hist_motifs(pengk_ctx* ctx, int n_motifs, const int32_t* h_S, const int32_t* h_len, int strands, const int32_t* h_thr,
                      const int32_t* h_hi, const uint64_t* h_hist_offs, StagedMotifs* st, const int32_t** d_hi,
                      const uint64_t** d_ho) {
  const size_t hb = ((size_t)n_motifs * sizeof(int32_t) + 7) & ~(size_t)7;
  std::vector<char> staged(hb + (size_t)n_motifs * sizeof(uint64_t));
  memcpy(staged.data(), h_hi, (size_t)n_motifs * sizeof(int32_t));
  memcpy(staged.data() + hb, h_hist_offs, (size_t)n_motifs * sizeof(uint64_t));
  int rc = ensure_scratch(ctx, &ctx->d_misc, &ctx->misc_bytes, staged.size());
  if (rc) return rc;
  rc = stage_motifs(ctx, n_motifs, h_S, h_len, strands, h_thr, st);
  if (rc) return rc;
  PENGK_HIP(hipMemcpy(ctx->d_misc, staged.data(), staged.size(), hipMemcpyHostToDevice));
  *d_hi = (const int32_t*)ctx->d_misc;
  *d_ho = (const uint64_t*)((char*)ctx->d_misc + hb);
  return PENGK_OK;
}

}  // namespace
}  // namespace pengk

using namespace pengk;

extern "C" {

int pengk_sites_count(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                      const uint32_t* d_lens, uint64_t n_seq, int n_motifs, const int32_t* h_S, const int32_t* h_len,
                      int both_strands, const int32_t* h_thr, uint64_t* d_counts) {
  if (!ctx || n_motifs < 0 || (n_motifs && (!h_S || !h_len || !h_thr)) ||
      (n_seq && n_motifs && (!d_words || !d_offs || !d_lens || !d_counts)))
    return fail(PENGK_ERR_ARG, "pengk_sites_count: bad argument");
  int rc = check_motifs("pengk_sites_count", n_motifs, h_S, h_len);
  if (rc) return rc;
  SCORE_ENTER(ctx);
  if (n_seq == 0 || n_motifs == 0) return PENGK_OK;
  StagedMotifs st;
  rc = stage_motifs(ctx, n_motifs, h_S, h_len, both_strands ? 2 : 1, h_thr, &st);
  if (rc) return rc;
  const dim3 grid(grid_for(ctx, n_seq, SCAN_THREADS, 8), (unsigned)st.n_groups);
  unsigned long long* c = (unsigned long long*)d_counts;
  by_strands(both_strands, [&](auto B) {
    hipLaunchKernelGGL((motif_sites_kernel<decltype(B)::value, false>), grid, dim3(SCAN_THREADS), 0, ctx->stream, d_words, d_valid,
                       d_offs, d_lens, (uint64_t)0, n_seq, n_seq, st.tables, st.recs, st.groups, st.thr, c, nullptr, nullptr,
                       (uint64_t)0);
  });
  PENGK_HIP(hipGetLastError());
  return PENGK_OK;
}

int pengk_sites_histograms(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                           const uint32_t* d_lens, uint64_t n_seq, int n_motifs, const int32_t* h_S, const int32_t* h_len,
                           int both_strands, const int32_t* h_thr, const int32_t* h_hi, const uint64_t* h_hist_offs,
                           uint64_t* d_hist, uint64_t* d_tests, uint64_t* d_counts) {
  if (!ctx || n_motifs < 0 || (n_motifs && (!h_S || !h_len || !h_thr || !h_hi || !h_hist_offs || !d_tests)) ||
      (n_seq && n_motifs && (!d_words || !d_offs || !d_lens)))
    return fail(PENGK_ERR_ARG, "pengk_sites_histograms: bad argument");
  int rc = check_motifs("pengk_sites_histograms", n_motifs, h_S, h_len);
  if (rc) return rc;
  rc = check_hist_range("pengk_sites_histograms", n_motifs, h_S, h_len, h_thr, h_hi, d_hist);
  if (rc) return rc;
  SCORE_ENTER(ctx);
  if (n_seq == 0 || n_motifs == 0) return PENGK_OK;
  StagedMotifs st;
  const int32_t* d_hi;
  const uint64_t* d_ho;
  rc = stage_hist_motifs(ctx, n_motifs, h_S, h_len, both_strands ? 2 : 1, h_thr, h_hi, h_hist_offs, &st, &d_hi, &d_ho);
  if (rc) return rc;
  const dim3 grid(grid_for(ctx, n_seq, SCAN_THREADS, 8), (unsigned)st.n_groups);
  unsigned long long* h = (unsigned long long*)d_hist;
  unsigned long long* t = (unsigned long long*)d_tests;
  unsigned long long* c = (unsigned long long*)d_counts;
  by_strands(both_strands, [&](auto B) {
    hipLaunchKernelGGL(motif_sites_hist_kernel<decltype(B)::value>, grid, dim3(SCAN_THREADS), 0, ctx->stream, d_words, d_valid,
                       d_offs, d_lens, n_seq, st.tables, st.recs, st.groups, st.thr, d_hi, d_ho, h, t, c);
  });
  PENGK_HIP(hipGetLastError());
  return PENGK_OK;
}

int pengk_motif_enrich(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                       const uint32_t* d_lens, uint64_t n_seq, int n_motifs, const int32_t* h_S, const int32_t* h_len,
                       int both_strands, const int32_t* h_thr, const int32_t* h_hi, const uint64_t* h_hist_offs,
                       uint64_t* d_hist, uint64_t* d_scored) {
  if (!ctx || n_motifs < 0 || (n_motifs && (!h_S || !h_len || !h_thr || !h_hi || !h_hist_offs || !d_scored)) ||
      (n_seq && n_motifs && (!d_words || !d_offs || !d_lens)))
    return fail(PENGK_ERR_ARG, "pengk_motif_enrich: bad argument");
  // (what keeps a 32-bit private bin from wrapping without a flush inside the loop: a sequence adds once per motif)
  if (n_seq >= (1ull << 32)) return fail(PENGK_ERR_ARG, "pengk_motif_enrich: n_seq %llu (below 2^32)", (unsigned long long)n_seq);
  int rc = check_motifs("pengk_motif_enrich", n_motifs, h_S, h_len);
  if (rc) return rc;
  rc = check_hist_range("pengk_motif_enrich", n_motifs, h_S, h_len, h_thr, h_hi, d_hist);
  if (rc) return rc;
  SCORE_ENTER(ctx);
  if (n_seq == 0 || n_motifs == 0) return PENGK_OK;
  const int strands = both_strands ? 2 : 1;
  const int64_t per_launch = ctx->enrich_groups_per_launch;
  unsigned long long* h = (unsigned long long*)d_hist;
  unsigned long long* sc = (unsigned long long*)d_scored;
  // batches of whole motif groups: the groups are stage_motifs' (the same rule, in motif order), so a batch that starts
  // where a group starts is cut into the groups the whole set would be cut into
  for (int m0 = 0; m0 < n_motifs;) {
    int m1 = m0, ints = 0;
    int64_t n_groups = 1;
    for (; m1 < n_motifs; ++m1) {
      const MotifFit fit = fit_motif(ints, h_len[m1], strands, Order0::STRIDE);
      if (fit.opens) {
        if (n_groups == per_launch) break;
        ++n_groups;
        ints = 0;
      }
      ints += fit.need;
    }
    const int nb = m1 - m0;
    StagedMotifs st;
    const int32_t* d_hi;
    const uint64_t* d_ho;
    rc = stage_hist_motifs(ctx, nb, h_S + (size_t)m0 * PENGK_MAX_MOTIF_LEN * 4, h_len + m0, strands, h_thr + m0, h_hi + m0,
                           h_hist_offs + m0, &st, &d_hi, &d_ho);
    if (rc) return rc;
    if (st.n_groups != (int)n_groups) return fail(PENGK_ERR_RANGE, "pengk_motif_enrich: %d groups staged, %d planned", st.n_groups, (int)n_groups);
    const dim3 grid(grid_for(ctx, n_seq, SCAN_THREADS, 8), (unsigned)st.n_groups);
    // (the records carry motif indices within the batch: the scored counters are passed from the batch's first motif on;
    // the histogram offsets are the caller's, from d_hist)
    by_strands(both_strands, [&](auto B) {
      hipLaunchKernelGGL(motif_enrich_kernel<decltype(B)::value>, grid, dim3(SCAN_THREADS), 0, ctx->stream, d_words, d_valid,
                         d_offs, d_lens, n_seq, st.tables, st.recs, st.groups, st.thr, d_hi, d_ho, h, sc + m0);
    });
    PENGK_HIP(hipGetLastError());
    m0 = m1;
  }
  return PENGK_OK;
}

int pengk_sites_slices(pengk_ctx* ctx, const uint64_t* d_counts, uint64_t n_seq, int n_motifs, uint64_t* h_motif_totals,
                       uint64_t max_slices, uint64_t* h_bounds, uint64_t* h_records, uint64_t* n_slices) {
  if (!ctx || n_motifs < 0 || !n_slices || (n_motifs && !h_motif_totals) || (max_slices && (!h_bounds || !h_records)) ||
      (n_seq && n_motifs && !d_counts))
    return fail(PENGK_ERR_ARG, "pengk_sites_slices: bad argument");
  SCORE_ENTER(ctx);
  *n_slices = 0;
  for (int m = 0; m < n_motifs; ++m) h_motif_totals[m] = 0;
  if (n_seq == 0) return PENGK_OK;
  const uint64_t nb = (n_seq + SITES_BLOCK - 1) / SITES_BLOCK;
  std::vector<uint64_t> bt(nb, 0);
  unsigned long long *seq_tot = nullptr, *block_tot = nullptr;
  if (n_motifs) {
    const size_t bytes = (n_seq + nb + (size_t)n_motifs) * sizeof(uint64_t);
    int rc = ensure_scratch(ctx, &ctx->d_sites, &ctx->sites_bytes, bytes);
    if (rc) return rc;
    seq_tot = (unsigned long long*)ctx->d_sites;
    block_tot = seq_tot + n_seq;
    unsigned long long* mtot = block_tot + nb;
    PENGK_HIP(hipMemsetAsync(mtot, 0, (size_t)n_motifs * sizeof(uint64_t), ctx->stream));
    hipLaunchKernelGGL(site_totals_kernel, dim3((unsigned)nb), dim3(SITES_THREADS), 0, ctx->stream,
                       (const unsigned long long*)d_counts, n_seq, n_motifs, seq_tot, block_tot, mtot);
    PENGK_HIP(hipGetLastError());
    PENGK_HIP(hipMemcpyAsync(bt.data(), block_tot, nb * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    PENGK_HIP(hipMemcpyAsync(h_motif_totals, mtot, (size_t)n_motifs * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    PENGK_HIP(hipStreamSynchronize(ctx->stream));
  }
  // slices of whole blocks while their records fit the budget; a block above it alone is cut between its sequences, and a
  // sequence above it is a slice of its own
  const uint64_t B = ctx->sites_record_budget;
  const uint64_t MAX_SEQ = 1ull << 31;  // (a record's sequence is an index into its slice: uint32)
  uint64_t ns = 0, i0 = 0, acc = 0;
  auto close = [&](uint64_t i1) {
    if (ns < max_slices) {
      h_bounds[ns] = i0;
      h_bounds[ns + 1] = i1;
      h_records[ns] = acc;
    }
    ++ns;
    i0 = i1;
    acc = 0;
  };
  std::vector<uint64_t> st;
  for (uint64_t b = 0; b < nb; ++b) {
    const uint64_t bb = b * SITES_BLOCK, be = std::min<uint64_t>(n_seq, bb + SITES_BLOCK);
    if (be - i0 > MAX_SEQ) close(bb);
    if (acc + bt[b] <= B) {
      acc += bt[b];
      continue;
    }
    if (bt[b] <= B) {
      close(bb);
      acc = bt[b];
      continue;
    }
    st.resize(be - bb);
    PENGK_HIP(hipMemcpy(st.data(), seq_tot + bb, (be - bb) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    for (uint64_t i = bb; i < be; ++i) {
      const uint64_t t = st[i - bb];
      if (acc + t > B && i > i0) close(i);
      acc += t;
    }
  }
  close(n_seq);
  *n_slices = ns;
  return PENGK_OK;
}

int pengk_sites_emit(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                     const uint32_t* d_lens, uint64_t n_seq, int n_motifs, const int32_t* h_S, const int32_t* h_len,
                     int both_strands, const int32_t* h_thr, const uint64_t* d_counts, uint64_t i0, uint64_t i1,
                     pengk_site* d_sites, uint64_t cap) {
  if (!ctx || n_motifs < 0 || i0 > i1 || i1 > n_seq || i1 - i0 > (1ull << 31) || (n_motifs && (!h_S || !h_len || !h_thr)) ||
      (i1 > i0 && n_motifs && (!d_words || !d_offs || !d_lens || !d_counts || (cap && !d_sites))))
    return fail(PENGK_ERR_ARG, "pengk_sites_emit: bad argument");
  int rc = check_motifs("pengk_sites_emit", n_motifs, h_S, h_len);
  if (rc) return rc;
  SCORE_ENTER(ctx);
  if (i1 == i0 || n_motifs == 0) return PENGK_OK;
  const uint64_t ns = i1 - i0, n = ns * (uint64_t)n_motifs, n_tiles = (n + XS_TILE - 1) / XS_TILE;
  StagedMotifs st;
  rc = stage_motifs(ctx, n_motifs, h_S, h_len, both_strands ? 2 : 1, h_thr, &st);
  if (rc) return rc;
  rc = ensure_scratch(ctx, &ctx->d_sites, &ctx->sites_bytes, (n + n_tiles) * sizeof(uint64_t));
  if (rc) return rc;
  unsigned long long* so = (unsigned long long*)ctx->d_sites;
  unsigned long long* part = so + n;
  const unsigned long long* c = (const unsigned long long*)d_counts;
  // where each (motif, sequence) writes: the exclusive scan of the counts, motif-major
  hipLaunchKernelGGL(xscan_tiles_kernel, dim3((unsigned)n_tiles), dim3(SITES_THREADS), 0, ctx->stream, c, n_seq, i0, ns, n, part);
  hipLaunchKernelGGL(xscan_parts_kernel, dim3(1), dim3(SITES_THREADS), 0, ctx->stream, part, n_tiles);
  hipLaunchKernelGGL(xscan_apply_kernel, dim3((unsigned)n_tiles), dim3(SITES_THREADS), 0, ctx->stream, c, n_seq, i0, ns, n, part, so);
  PENGK_HIP(hipGetLastError());
  const dim3 grid(grid_for(ctx, ns, SCAN_THREADS, 8), (unsigned)st.n_groups);
  by_strands(both_strands, [&](auto B) {
    hipLaunchKernelGGL((motif_sites_kernel<decltype(B)::value, true>), grid, dim3(SCAN_THREADS), 0, ctx->stream, d_words, d_valid,
                       d_offs, d_lens, i0, i1, n_seq, st.tables, st.recs, st.groups, st.thr, nullptr, so, d_sites, cap);
  });
  PENGK_HIP(hipGetLastError());
  return PENGK_OK;
}

}  // extern "C"
