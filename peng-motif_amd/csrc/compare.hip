// compare.hip -- --compare: found motifs against a database of known motifs (include/pengk.h, "motif comparison").  The
// same shape of work as similarity.hip with a database on one side, plus a p-value per match from a null built over the
// whole database.  The definitions are this project's own, in the spirit of Tomtom (Gupta et al. 2007) with the
// Sandelin-Wasserman column score; tests/motif_compare_model.py restates them in numpy.
//
// A column is four int16 in [0, 4096] (8 bytes; quantised on the host, pengk_compare_quantize): the device sees integers
// only, and the score of two columns is s = max(0, 256 - (d >> 17)), d their squared distance.
//
// Three kernels:
//   compare_null_kernel   h[q][i][v]: the database columns, in both orientations, that score v against column i of
//                         query q.  Reversing a motif moves no column out of the database, so the other orientation is
//                         met by reversing the QUERY column's letters: one pass over the packed columns serves both.
//                         A workgroup owns 16 query columns and 8192 database columns, bins in LDS (16 x 257 uint32),
//                         flushed with one 64-bit atomic per non-empty bin.
//   compare_tail_kernel   per (query, i0): the chain pmf_i0, pmf_i0 * pmf_i0+1, ... in fp64 (pmf_i = h_i / N), resident
//                         in LDS (64 x 256 + 1 doubles = 128 KiB, between zeros so that no index is tested), each
//                         thread holding up to 17 of the new values in registers; after every step the suffix sums
//                         P(sum >= S) -- at most 1, 1 up to the smallest sum the null can give, never rising with S --
//                         go to the tail table.  All terms are non-negative: any summation order stays within a relative
//                         n_terms * 2^-53 of the exact sum.
//   compare_align_kernel  per (query, tile of 64 targets), a wave per target: a lane owns an (orientation, offset), sums
//                         the column scores of the overlap, looks its tail up and keeps the best by (smaller p, larger
//                         overlap, + before -, smaller offset); a butterfly over the wave selects the pair's alignment.
//
// Device memory is bounded: a query of width w needs sum over i0, n of (256 n + 1) doubles of tails (w = 64: 11.72 M
// doubles, 94 MB), so queries are processed in batches of at most TAIL_BUDGET bytes of tails (256 MiB) and at most
// PAIR_BUDGET (query, target) records (2^22, 28 bytes each); a single query is a batch of its own when it exceeds either.
#include <math.h>

#include <algorithm>
#include <vector>

#include "pengk_internal.h"

namespace pengk {
namespace {

constexpr int MAXL = PENGK_MAX_MOTIF_LEN;
constexpr int BINS = 257;
constexpr int QSCALE = 4096;

constexpr int NULL_COLS = 16;      // query columns of a workgroup of compare_null_kernel
constexpr int NULL_CHUNK = 8192;   // ... and its database columns (a bin stays below 2^15)
constexpr int TAIL_THREADS = 1024;
constexpr int TAIL_PER = 17;       // ceil((MAXL * 256 + 1) / TAIL_THREADS)
constexpr int TAIL_PAD = 256;
constexpr int ALIGN_TILE = 64;
constexpr size_t TAIL_BUDGET = (size_t)256 << 20;
constexpr size_t PAIR_BUDGET = (size_t)1 << 22;
constexpr int MAX_BATCH_QUERIES = 4096;

static_assert(TAIL_PER * TAIL_THREADS >= MAXL * 256 + 1, "a thread holds its share of the longest pmf");

__host__ __device__ inline uint64_t tails_before(int n) {  // sum over n' < n of (256 n' + 1): where tail(i0, n) starts in row i0
  const uint64_t l = (uint64_t)(n - 1);
  return 128 * l * (l + 1) + l;
}

__device__ __forceinline__ int col_score(short4 x, short4 y) {
  const int a = x.x - y.x, b = x.y - y.y, c = x.z - y.z, e = x.w - y.w;
  const uint32_t d = (uint32_t)(a * a) + (uint32_t)(b * b) + (uint32_t)(c * c) + (uint32_t)(e * e);  // <= 2^26
  const int s = 256 - (int)(d >> 17);
  return s < 0 ? 0 : s;
}

__device__ __forceinline__ short4 flip(short4 x) { return make_short4(x.w, x.z, x.y, x.x); }

// grid: (queries x MAXL / NULL_COLS, chunks of the database)
__global__ __launch_bounds__(256) void compare_null_kernel(const short4* __restrict__ Q, const int32_t* __restrict__ qlen,
                                                           const short4* __restrict__ T, uint32_t n_cols, int both,
                                                           unsigned long long* __restrict__ hist) {
  constexpr int GROUPS = MAXL / NULL_COLS;
  const int q = blockIdx.x / GROUPS, c0 = (blockIdx.x % GROUPS) * NULL_COLS;
  const int w = qlen[q];
  if (c0 >= w) return;
  const int nc = min(NULL_COLS, w - c0);
  __shared__ uint32_t h[NULL_COLS * BINS];
  __shared__ short4 qc[NULL_COLS];
  for (int e = threadIdx.x; e < NULL_COLS * BINS; e += 256) h[e] = 0;
  if (threadIdx.x < nc) qc[threadIdx.x] = Q[(size_t)q * MAXL + c0 + threadIdx.x];
  __syncthreads();
  const uint32_t begin = blockIdx.y * (uint32_t)NULL_CHUNK;
  const uint32_t end = min(begin + (uint32_t)NULL_CHUNK, n_cols);
  for (uint32_t j = begin + threadIdx.x; j < end; j += 256) {
    const short4 t = T[j];
    for (int c = 0; c < nc; ++c) {
      const short4 x = qc[c];
      atomicAdd(&h[c * BINS + col_score(x, t)], 1u);
      if (both) atomicAdd(&h[c * BINS + col_score(flip(x), t)], 1u);
    }
  }
  __syncthreads();
  unsigned long long* out = hist + ((size_t)q * MAXL + c0) * BINS;
  for (int e = threadIdx.x; e < nc * BINS; e += 256)
    if (h[e]) atomicAdd(&out[e], (unsigned long long)h[e]);
}

// grid: queries of the batch x MAXL (i0).  hist, qlen: of the batch's first query on.  row[q * MAXL + i0]: where the tails
// of (q, i0) start in `tails`.
__global__ __launch_bounds__(TAIL_THREADS) void compare_tail_kernel(const unsigned long long* __restrict__ hist,
                                                                    const int32_t* __restrict__ qlen, double N,
                                                                    const unsigned long long* __restrict__ row,
                                                                    double* __restrict__ tails) {
  const int q = blockIdx.x / MAXL, i0 = blockIdx.x % MAXL;
  const int w = qlen[q];
  if (i0 >= w) return;
  const int tid = threadIdx.x;
  // TAIL_PAD zeros, then the pmf of the columns so far, zero above its range up to every thread's last slot (138 KiB)
  __shared__ double cur[TAIL_PAD + TAIL_PER * TAIL_THREADS];
  __shared__ double col[BINS];
  __shared__ double part[TAIL_THREADS];
  __shared__ double wmax[TAIL_THREADS / 64];
  __shared__ int smin;
  int vmin = 0;
  for (int e = tid; e < TAIL_PAD + TAIL_PER * TAIL_THREADS; e += TAIL_THREADS) cur[e] = 0.0;
  __syncthreads();
  double* const out = tails + row[(size_t)q * MAXL + i0];
  const int L = w - i0;
  for (int n = 1; n <= L; ++n) {
    const unsigned long long* h = hist + ((size_t)q * MAXL + i0 + n - 1) * BINS;
    if (tid == 0) smin = BINS;
    __syncthreads();
    if (tid < BINS) {
      const unsigned long long hv = h[tid];
      col[tid] = (double)hv / N;
      if (hv) atomicMin(&smin, tid);
    }
    __syncthreads();
    vmin += smin;  // the smallest sum the null can give: at and below it the tail is 1, whatever the rounding
    const int len = n * 256 + 1;
    if (n == 1) {
      if (tid < BINS) cur[TAIL_PAD + tid] = col[tid];
    } else {
      double acc[TAIL_PER];
#pragma unroll
      for (int j = 0; j < TAIL_PER; ++j) acc[j] = 0.0;
      const int jmax = (len + TAIL_THREADS - 1) / TAIL_THREADS;  // (block-uniform)
      for (int u = 0; u < BINS; ++u) {
        const double pu = col[u];
        if (pu == 0.0) continue;  // (block-uniform; an empty bin adds nothing)
        const double* src = cur + TAIL_PAD + tid - u;  // >= cur (u <= TAIL_PAD); + j * TAIL_THREADS stays inside cur
#pragma unroll
        for (int j = 0; j < TAIL_PER; ++j)
          if (j < jmax) acc[j] += src[j * TAIL_THREADS] * pu;
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < TAIL_PER; ++j) {
        const int v = tid + j * TAIL_THREADS;
        if (v < len) cur[TAIL_PAD + v] = acc[j];
      }
    }
    __syncthreads();
    // suffix sums: a thread sums its chunk, the chunks' sums are scanned from the top, the thread writes its tails
    const int C = (len + TAIL_THREADS - 1) / TAIL_THREADS;
    const int lo = min(tid * C, len), hi = min(lo + C, len);
    double s = 0.0;
    for (int v = hi - 1; v >= lo; --v) s += cur[TAIL_PAD + v];
    part[tid] = s;
    __syncthreads();
    for (int off = 1; off < TAIL_THREADS; off <<= 1) {
      const double add = tid + off < TAIL_THREADS ? part[tid + off] : 0.0;
      __syncthreads();
      part[tid] += add;
      __syncthreads();
    }
    const double above = tid + 1 < TAIL_THREADS ? part[tid + 1] : 0.0;
    // A tail must not rise with S.  Within a thread's chunk it cannot; across chunks the scanned sum `above` and the
    // next thread's own additions round differently, and the tail at the top of a chunk could lie an ulp or two below
    // the one above it.  So no tail is smaller than the largest tail of the threads above: `low` is this thread's tail at
    // its lowest v (the additions of the loop below, in their order), `floor_` the largest `low` of the threads above --
    // a suffix maximum over the wave, then over the waves.
    double low = above;
    for (int v = hi - 1; v >= lo; --v) low += cur[TAIL_PAD + v];
    const int lane = tid & 63, wave = tid >> 6;
    double m = low;
    for (int off = 1; off < 64; off <<= 1) {
      const double other = __shfl_down(m, off, 64);
      if (lane + off < 64) m = fmax(m, other);
    }
    double floor_ = __shfl_down(m, 1, 64);
    if (lane == 63) floor_ = 0.0;
    if (lane == 0) wmax[wave] = m;
    __syncthreads();
    for (int x = wave + 1; x < TAIL_THREADS / 64; ++x) floor_ = fmax(floor_, wmax[x]);
    double run = above;
    double* o = out + tails_before(n);
    for (int v = hi - 1; v >= lo; --v) {
      run += cur[TAIL_PAD + v];
      o[v] = v <= vmin ? 1.0 : fmin(fmax(run, floor_), 1.0);
    }
    // (the next step writes col, then cur, part and wmax only behind a barrier that every thread reaches after these reads)
  }
}

struct Cand {
  double p;
  int n, o, k, S;
};

__device__ __forceinline__ bool better(const Cand& a, const Cand& b) {
  if (a.p != b.p) return a.p < b.p;
  if (a.n != b.n) return a.n > b.n;
  if (a.o != b.o) return a.o < b.o;
  return a.k < b.k;
}

// grid: (tiles of ALIGN_TILE targets, queries of the batch).  Q, qlen, row: of the batch's first query on; align, p_out:
// the batch's records, query-major.
__global__ __launch_bounds__(256) void compare_align_kernel(const short4* __restrict__ Q, const int32_t* __restrict__ qlen,
                                                            const short4* __restrict__ T, const uint32_t* __restrict__ toff,
                                                            uint32_t n_t, int both, int M,
                                                            const unsigned long long* __restrict__ row,
                                                            const double* __restrict__ tails, int32_t* __restrict__ align,
                                                            double* __restrict__ p_out) {
  const int q = blockIdx.y;
  const int wq = qlen[q];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ short4 qc[MAXL];
  __shared__ short4 tc[4][MAXL];
  if (threadIdx.x < MAXL) qc[threadIdx.x] = threadIdx.x < wq ? Q[(size_t)q * MAXL + threadIdx.x] : make_short4(0, 0, 0, 0);
  const int n_or = both ? 2 : 1;
  for (int r = 0; r < ALIGN_TILE / 4; ++r) {  // (every thread makes every round: the barriers are uniform)
    const uint32_t t = blockIdx.x * (uint32_t)ALIGN_TILE + (uint32_t)(r * 4 + wave);
    const bool live = t < n_t;
    const uint32_t t0 = live ? toff[t] : 0;
    const int wt = live ? (int)(toff[t + 1] - t0) : 0;
    __syncthreads();  // (the last round's reads of tc; qc in round 0)
    tc[wave][lane] = lane < wt ? T[t0 + lane] : make_short4(0, 0, 0, 0);
    __syncthreads();
    if (!live) continue;
    const int m = min(M, min(wq, wt));
    const int nk = wq + wt - 2 * m + 1, kmin = -(wt - m);
    Cand best = {INFINITY, -1, 2, 0, 0};
    for (int idx = lane; idx < n_or * nk; idx += 64) {
      const int o = idx / nk, k = kmin + idx % nk;
      const int i0 = max(k, 0), j0 = max(-k, 0);
      const int n = min(wq - i0, wt - j0);  // m <= n <= 64
      int S = 0;
      for (int c = 0; c < n; ++c) {
        const short4 y = o ? flip(tc[wave][wt - 1 - (j0 + c)]) : tc[wave][j0 + c];
        S += col_score(qc[i0 + c], y);
      }
      const Cand cand = {tails[row[(size_t)q * MAXL + i0] + tails_before(n) + (uint64_t)S], n, o, k, S};  // S <= 256 n
      if (better(cand, best)) best = cand;
    }
    for (int off = 32; off > 0; off >>= 1) {
      Cand other;
      other.p = __shfl_xor(best.p, off, 64);
      other.n = __shfl_xor(best.n, off, 64);
      other.o = __shfl_xor(best.o, off, 64);
      other.k = __shfl_xor(best.k, off, 64);
      other.S = __shfl_xor(best.S, off, 64);
      if (better(other, best)) best = other;
    }
    if (lane == 0) {
      const size_t rec = (size_t)q * n_t + t;
      int32_t* a = align + rec * 5;
      a[0] = best.k;
      a[1] = best.o;
      a[2] = best.n;
      a[3] = best.S;
      a[4] = n_or * nk;
      p_out[rec] = best.p;
    }
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
int check_motifs(const char* who, const char* what, int n, const int16_t* X, const int32_t* len) {
  for (int i = 0; i < n; ++i) {
    if (len[i] < 1 || len[i] > MAXL) return fail(PENGK_ERR_ARG, "%s: %s motif %d has width %d (1..%d)", who, what, i, len[i], MAXL);
    const int16_t* x = X + (size_t)i * MAXL * 4;
    for (int e = 0; e < len[i] * 4; ++e)
      if (x[e] < 0 || x[e] > QSCALE)
        return fail(PENGK_ERR_ARG, "%s: %s motif %d, column %d, letter %d is %d (0..%d)", who, what, i, e / 4, e % 4, (int)x[e], QSCALE);
  }
  return PENGK_OK;
}

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

struct Plan {
  // device layout of one call (offsets into ctx->d_cmp)
  size_t o_Q = 0, o_qlen = 0, o_T = 0, o_toff = 0, o_hist = 0, o_row = 0, o_tails = 0, o_align = 0, o_p = 0, bytes = 0;
  uint32_t n_cols = 0;
  std::vector<uint32_t> toff;
  std::vector<int16_t> cols;                 // the database's columns, back to back
  std::vector<int> batch_begin;              // queries [batch_begin[b], batch_begin[b + 1])
  std::vector<unsigned long long> row;       // [q * MAXL + i0]: offset of (q, i0)'s tails within its batch's table
};

// validates, packs the database and lays the scratch out; with_tails = false: what pengk_compare_nulls needs
int make_plan(const char* who, int n_q, const int16_t* h_QX, const int32_t* h_qlen, int n_t, const int16_t* h_TX,
              const int32_t* h_tlen, bool with_tails, Plan* pl) {
  if (n_q < 1) return fail(PENGK_ERR_ARG, "%s: n_q = %d (at least 1 query)", who, n_q);
  if (n_t < 1) return fail(PENGK_ERR_ARG, "%s: n_t = %d (at least 1 target)", who, n_t);
  if (!h_QX || !h_qlen || !h_TX || !h_tlen) return fail(PENGK_ERR_ARG, "%s: NULL argument", who);
  int rc = check_motifs(who, "h_QX / h_qlen: query", n_q, h_QX, h_qlen);
  if (!rc) rc = check_motifs(who, "h_TX / h_tlen: target", n_t, h_TX, h_tlen);
  if (rc) return rc;
  if ((uint64_t)n_t * MAXL > 0xFFFFFFFFull / 2 || (uint64_t)n_q * (MAXL / NULL_COLS) > 0x7FFFFFFFull)
    return fail(PENGK_ERR_RANGE, "%s: %d queries against %d targets in one call", who, n_q, n_t);
  pl->toff.assign((size_t)n_t + 1, 0);
  for (int t = 0; t < n_t; ++t) pl->toff[t + 1] = pl->toff[t] + (uint32_t)h_tlen[t];
  pl->n_cols = pl->toff[n_t];
  pl->cols.resize((size_t)pl->n_cols * 4);
  for (int t = 0; t < n_t; ++t)
    std::copy(h_TX + (size_t)t * MAXL * 4, h_TX + (size_t)t * MAXL * 4 + (size_t)h_tlen[t] * 4, pl->cols.begin() + (size_t)pl->toff[t] * 4);
  if ((pl->n_cols + (uint32_t)NULL_CHUNK - 1) / NULL_CHUNK > 65535u)
    return fail(PENGK_ERR_RANGE, "%s: %u database columns in one call", who, pl->n_cols);

  size_t tails_max = 0, pairs_max = 0;
  if (with_tails) {
    pl->row.assign((size_t)n_q * MAXL, 0);
    size_t cur = 0;
    int in_batch = 0;
    pl->batch_begin.push_back(0);
    for (int q = 0; q < n_q; ++q) {
      size_t need = 0;
      for (int i0 = 0; i0 < h_qlen[q]; ++i0) need += (size_t)tails_before(h_qlen[q] - i0 + 1);
      if (in_batch && ((cur + need) * sizeof(double) > TAIL_BUDGET || (size_t)(in_batch + 1) * (size_t)n_t > PAIR_BUDGET ||
                       in_batch == MAX_BATCH_QUERIES)) {
        pl->batch_begin.push_back(q);
        cur = 0;
        in_batch = 0;
      }
      for (int i0 = 0; i0 < h_qlen[q]; ++i0) {
        pl->row[(size_t)q * MAXL + i0] = cur;
        cur += (size_t)tails_before(h_qlen[q] - i0 + 1);
      }
      ++in_batch;
      tails_max = std::max(tails_max, cur);
      pairs_max = std::max(pairs_max, (size_t)in_batch * (size_t)n_t);
    }
    pl->batch_begin.push_back(n_q);
  }
  size_t o = 0;
  pl->o_Q = o;
  o = up256(o + (size_t)n_q * MAXL * 8);
  pl->o_qlen = o;
  o = up256(o + (size_t)n_q * 4);
  pl->o_T = o;
  o = up256(o + (size_t)pl->n_cols * 8);
  pl->o_toff = o;
  o = up256(o + ((size_t)n_t + 1) * 4);
  pl->o_hist = o;
  o = up256(o + (size_t)n_q * MAXL * BINS * 8);
  pl->o_row = o;
  o = up256(o + (size_t)n_q * MAXL * 8);
  pl->o_tails = o;
  o = up256(o + tails_max * sizeof(double));
  pl->o_align = o;
  o = up256(o + pairs_max * 5 * sizeof(int32_t));
  pl->o_p = o;
  o = up256(o + pairs_max * sizeof(double));
  pl->bytes = o;
  return PENGK_OK;
}

// uploads the motifs and fills the null histograms of every query on the device
int run_nulls(pengk_ctx* ctx, const Plan& pl, int n_q, const int16_t* h_QX, const int32_t* h_qlen, int n_t, int both) {
  int rc = ensure_scratch(ctx, &ctx->d_cmp, &ctx->cmp_bytes, pl.bytes);
  if (rc) return rc;
  char* base = (char*)ctx->d_cmp;
  PENGK_HIP(hipMemcpyAsync(base + pl.o_Q, h_QX, (size_t)n_q * MAXL * 8, hipMemcpyHostToDevice, ctx->stream));
  PENGK_HIP(hipMemcpyAsync(base + pl.o_qlen, h_qlen, (size_t)n_q * 4, hipMemcpyHostToDevice, ctx->stream));
  PENGK_HIP(hipMemcpyAsync(base + pl.o_T, pl.cols.data(), (size_t)pl.n_cols * 8, hipMemcpyHostToDevice, ctx->stream));
  PENGK_HIP(hipMemcpyAsync(base + pl.o_toff, pl.toff.data(), ((size_t)n_t + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
  if (!pl.row.empty())
    PENGK_HIP(hipMemcpyAsync(base + pl.o_row, pl.row.data(), pl.row.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  PENGK_HIP(hipMemsetAsync(base + pl.o_hist, 0, (size_t)n_q * MAXL * BINS * 8, ctx->stream));
  const dim3 grid((unsigned)n_q * (MAXL / NULL_COLS), (pl.n_cols + NULL_CHUNK - 1) / NULL_CHUNK);
  hipLaunchKernelGGL(compare_null_kernel, grid, dim3(256), 0, ctx->stream, (const short4*)(base + pl.o_Q),
                     (const int32_t*)(base + pl.o_qlen), (const short4*)(base + pl.o_T), pl.n_cols, both,
                     (unsigned long long*)(base + pl.o_hist));
  PENGK_HIP(hipGetLastError());
  PENGK_HIP(hipStreamSynchronize(ctx->stream));  // (the plan's host vectors may go once this returns)
  return PENGK_OK;
}

}  // namespace

// (pengk_warmup: loads this translation unit's code object ahead of its first launch)
int warm_compare() {
  hipFuncAttributes a;
  PENGK_HIP(hipFuncGetAttributes(&a, (const void*)compare_align_kernel));
  return PENGK_OK;
}

}  // namespace pengk

using namespace pengk;

extern "C" {

int pengk_compare_quantize(const double* h_rows, int w, int16_t* h_X) {
  if (!h_rows || !h_X) return fail(PENGK_ERR_ARG, "pengk_compare_quantize: NULL argument");
  if (w < 1 || w > MAXL) return fail(PENGK_ERR_ARG, "pengk_compare_quantize: w = %d (1..%d)", w, MAXL);
  for (int j = 0; j < w; ++j) {
    const double* p = h_rows + (size_t)j * 4;
    for (int a = 0; a < 4; ++a)
      if (!(p[a] >= 0.0)) return fail(PENGK_ERR_ARG, "pengk_compare_quantize: h_rows: row %d, letter %d is %g (>= 0)", j, a, p[a]);
    const double s = ((p[0] + p[1]) + p[2]) + p[3];
    if (!(s > 0.0) || !(s <= 1.79769313486231570815e+308))
      return fail(PENGK_ERR_ARG, "pengk_compare_quantize: h_rows: row %d sums to %g (a positive, finite number)", j, s);
    for (int a = 0; a < 4; ++a) h_X[(size_t)j * 4 + a] = (int16_t)floor(4096.0 * (p[a] / s) + 0.5);
  }
  return PENGK_OK;
}

int pengk_compare_nulls(pengk_ctx* ctx, int n_q, const int16_t* h_QX, const int32_t* h_qlen, int n_t, const int16_t* h_TX,
                        const int32_t* h_tlen, int both, uint64_t* h_hist) {
  if (!ctx || !h_hist) return fail(PENGK_ERR_ARG, "pengk_compare_nulls: NULL argument");
  Plan pl;
  int rc = make_plan("pengk_compare_nulls", n_q, h_QX, h_qlen, n_t, h_TX, h_tlen, false, &pl);
  if (rc) return rc;
  rc = enter(ctx);
  if (!rc) rc = run_nulls(ctx, pl, n_q, h_QX, h_qlen, n_t, both ? 1 : 0);
  if (rc) return rc;
  PENGK_HIP(hipMemcpyAsync(h_hist, (char*)ctx->d_cmp + pl.o_hist, (size_t)n_q * MAXL * BINS * 8, hipMemcpyDeviceToHost, ctx->stream));
  PENGK_HIP(hipStreamSynchronize(ctx->stream));
  return PENGK_OK;
}

int pengk_compare_motifs(pengk_ctx* ctx, int n_q, const int16_t* h_QX, const int32_t* h_qlen, int n_t, const int16_t* h_TX,
                         const int32_t* h_tlen, int both, int min_overlap, int32_t* h_align, double* h_p) {
  if (!ctx || !h_align || !h_p) return fail(PENGK_ERR_ARG, "pengk_compare_motifs: NULL argument");
  if (min_overlap < 1) return fail(PENGK_ERR_ARG, "pengk_compare_motifs: min_overlap = %d (at least 1 column)", min_overlap);
  Plan pl;
  int rc = make_plan("pengk_compare_motifs", n_q, h_QX, h_qlen, n_t, h_TX, h_tlen, true, &pl);
  if (rc) return rc;
  rc = enter(ctx);
  if (!rc) rc = run_nulls(ctx, pl, n_q, h_QX, h_qlen, n_t, both ? 1 : 0);
  if (rc) return rc;
  char* base = (char*)ctx->d_cmp;
  const double N = (double)pl.n_cols * (both ? 2.0 : 1.0);
  const int M = std::min(min_overlap, MAXL);
  for (size_t b = 0; b + 1 < pl.batch_begin.size(); ++b) {
    const int qa = pl.batch_begin[b], nq = pl.batch_begin[b + 1] - qa;
    const int32_t* d_qlen = (const int32_t*)(base + pl.o_qlen) + qa;
    const unsigned long long* d_row = (const unsigned long long*)(base + pl.o_row) + (size_t)qa * MAXL;
    hipLaunchKernelGGL(compare_tail_kernel, dim3((unsigned)nq * MAXL), dim3(TAIL_THREADS), 0, ctx->stream,
                       (const unsigned long long*)(base + pl.o_hist) + (size_t)qa * MAXL * BINS, d_qlen, N, d_row,
                       (double*)(base + pl.o_tails));
    PENGK_HIP(hipGetLastError());
    hipLaunchKernelGGL(compare_align_kernel, dim3(((unsigned)n_t + ALIGN_TILE - 1) / ALIGN_TILE, (unsigned)nq), dim3(256), 0,
                       ctx->stream, (const short4*)(base + pl.o_Q) + (size_t)qa * MAXL, d_qlen, (const short4*)(base + pl.o_T),
                       (const uint32_t*)(base + pl.o_toff), (uint32_t)n_t, both ? 1 : 0, M, d_row,
                       (const double*)(base + pl.o_tails), (int32_t*)(base + pl.o_align), (double*)(base + pl.o_p));
    PENGK_HIP(hipGetLastError());
    const size_t pairs = (size_t)nq * (size_t)n_t;
    PENGK_HIP(hipMemcpyAsync(h_align + (size_t)qa * n_t * 5, base + pl.o_align, pairs * 5 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    PENGK_HIP(hipMemcpyAsync(h_p + (size_t)qa * n_t, base + pl.o_p, pairs * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    PENGK_HIP(hipStreamSynchronize(ctx->stream));
  }
  return PENGK_OK;
}

int pengk_test_compare_tails(pengk_ctx* ctx, int w, const uint64_t* h_hist, double* h_tails) {
  if (!ctx || !h_hist || !h_tails) return fail(PENGK_ERR_ARG, "pengk_test_compare_tails: NULL argument");
  if (w < 1 || w > MAXL) return fail(PENGK_ERR_ARG, "pengk_test_compare_tails: w = %d (1..%d)", w, MAXL);
  uint64_t N = 0;
  for (int i = 0; i < w; ++i) {
    uint64_t s = 0;
    bool over = false;
    for (int v = 0; v < BINS; ++v) {
      over = over || h_hist[(size_t)i * BINS + v] > ((uint64_t)1 << 32);  // (so that the sum cannot wrap)
      s += h_hist[(size_t)i * BINS + v];
    }
    if (over || s > ((uint64_t)1 << 32))
      return fail(PENGK_ERR_ARG, "pengk_test_compare_tails: h_hist: row %d sums to more than 2^32", i);
    if (i == 0) N = s;
    if (s != N)
      return fail(PENGK_ERR_ARG, "pengk_test_compare_tails: h_hist: row %d sums to %llu, row 0 to %llu", i, (unsigned long long)s,
                  (unsigned long long)N);
  }
  if (N == 0) return fail(PENGK_ERR_ARG, "pengk_test_compare_tails: h_hist: the rows sum to 0");
  // one query, a batch of its own: the layout of make_plan's row for it
  std::vector<unsigned long long> row(MAXL, 0);
  size_t total = 0;
  for (int i0 = 0; i0 < w; ++i0) {
    row[i0] = total;
    total += (size_t)tails_before(w - i0 + 1);
  }
  const int32_t qlen = w;
  const size_t o_hist = 0, o_qlen = up256((size_t)MAXL * BINS * 8), o_row = up256(o_qlen + 4), o_tails = up256(o_row + (size_t)MAXL * 8);
  int rc = enter(ctx);
  if (!rc) rc = ensure_scratch(ctx, &ctx->d_cmp, &ctx->cmp_bytes, up256(o_tails + total * sizeof(double)));
  if (rc) return rc;
  char* base = (char*)ctx->d_cmp;
  PENGK_HIP(hipMemsetAsync(base + o_hist, 0, (size_t)MAXL * BINS * 8, ctx->stream));
  PENGK_HIP(hipMemcpyAsync(base + o_hist, h_hist, (size_t)w * BINS * 8, hipMemcpyHostToDevice, ctx->stream));
  PENGK_HIP(hipMemcpyAsync(base + o_qlen, &qlen, 4, hipMemcpyHostToDevice, ctx->stream));
  PENGK_HIP(hipMemcpyAsync(base + o_row, row.data(), (size_t)MAXL * 8, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(compare_tail_kernel, dim3((unsigned)MAXL), dim3(TAIL_THREADS), 0, ctx->stream,
                     (const unsigned long long*)(base + o_hist), (const int32_t*)(base + o_qlen), (double)N,
                     (const unsigned long long*)(base + o_row), (double*)(base + o_tails));
  PENGK_HIP(hipGetLastError());
  PENGK_HIP(hipMemcpyAsync(h_tails, base + o_tails, total * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PENGK_HIP(hipStreamSynchronize(ctx->stream));  // (qlen and row are read until here)
  return PENGK_OK;
}

int pengk_compare_summary(const double* h_p, const int32_t* h_noff, int n_t, double* h_p_match, double* h_evalue, double* h_qvalue) {
  if (!h_p || !h_noff || !h_p_match || !h_evalue || !h_qvalue) return fail(PENGK_ERR_ARG, "pengk_compare_summary: NULL argument");
  if (n_t < 1) return fail(PENGK_ERR_ARG, "pengk_compare_summary: n_t = %d (at least 1 target)", n_t);
  const double T = (double)n_t;
  for (int t = 0; t < n_t; ++t) {
    if (!(h_p[t] >= 0.0 && h_p[t] <= 1.0) || h_noff[t] < 1)
      return fail(PENGK_ERR_ARG, "pengk_compare_summary: target %d has p_offset %g, n_offsets %d", t, h_p[t], h_noff[t]);
    h_p_match[t] = h_p[t] < 1.0 ? -expm1((double)h_noff[t] * log1p(-h_p[t])) : 1.0;
    h_evalue[t] = h_p_match[t] * T;
  }
  std::vector<int> order(n_t);
  for (int t = 0; t < n_t; ++t) order[t] = t;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return h_p_match[a] < h_p_match[b]; });
  double run = INFINITY;
  for (int r = n_t - 1; r >= 0; --r) {
    run = std::min(run, h_p_match[order[r]] * T / (double)(r + 1));
    h_qvalue[order[r]] = std::min(run, 1.0);
  }
  return PENGK_OK;
}

}  // extern "C"
