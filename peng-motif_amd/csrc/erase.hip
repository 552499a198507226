// erase.hip -- masking the sites of found motifs and packing what is left, on the device (--erase).
//
//   mask     the sites walk of sites.hip once more (scan_walk.h), with a visitor that turns every site into cover bits:
//            d_out_valid = d_valid & ~cover.  Windows arrive in ascending position, so a "covered until" index and one
//            pending word per thread are all the state; a word's cover is ANDed out with one integer atomic, whose
//            returned old value says which bits this call cleared first (the erased count).  Integer AND commutes:
//            motif groups on gridDim.y may arrive in any order.
//   pack     the host packer's rule (pack.cpp, for_each_run) over validity bits instead of byte codes: a measure pass
//            (stored bases, windows, items and bin bound per sequence), exclusive prefix sums in three launches, and a
//            write pass that copies every run's bases to its place in the 2-bit stream and stores its items.
//            The result is what pengk_pack writes for the same sequences, bit for bit.
// One thread per sequence throughout, like every scan kernel.  No float, no waiting between workgroups.
#include <string.h>

#include <algorithm>

#include "pengk_internal.h"
#include "scan_walk.h"
#include "tile_walk.h"

namespace pengk {
namespace {

using namespace scan;

// ---- pengk_mask_sites -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mask_init_kernel(const uint32_t* __restrict__ valid, const int64_t* __restrict__ offs,
                                                        const uint32_t* __restrict__ lens, uint64_t n_seq,
                                                        uint32_t* __restrict__ out) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n_seq; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t L = lens[i];
    const uint64_t w0 = (uint64_t)offs[i] >> 5;
    for (uint32_t j = 0; 32ull * j < L; ++j) out[w0 + j] = tile::valid_word_in(valid ? valid + w0 : nullptr, L, j);
  }
}

// The sites of a pass's motif, turned into cover bits of the sequence's words `out`.  until: the bases below it are
// covered by the sites seen so far; (cw, cb): the word being gathered and its cover bits, ANDed out when the cover
// moves on to a later word and in end() -- at most one atomic per touched word and motif.
template <bool BOTH>
struct MaskVisit {
  const MotifRec* mrec;
  const int32_t* thr;            // by group record
  unsigned long long* sites;     // LDS, by group record
  uint32_t* out;
  uint32_t erased;               // bits this thread's atomics found set and cleared
  int32_t t[SCAN_PASS];
  uint32_t w[SCAN_PASS], until[SCAN_PASS], cw[SCAN_PASS], cb[SCAN_PASS];
  unsigned long long c[SCAN_PASS];
  __device__ __forceinline__ void flush(int q) {
    if (cb[q]) {
      const uint32_t old = atomicAnd(&out[cw[q]], ~cb[q]);
      erased += (uint32_t)__popc(old & cb[q]);
      cb[q] = 0;
    }
  }
  __device__ __forceinline__ void begin(int q, int r) {
    t[q] = thr[r];
    w[q] = (uint32_t)mrec[r].w;
    until[q] = cw[q] = cb[q] = 0;
    c[q] = 0;
  }
  __device__ __forceinline__ void window(int q, uint32_t pos, int32_t sf, int32_t sr) {
    const unsigned hit = (unsigned)(sf >= t[q]) + (unsigned)(BOTH && sr >= t[q]);
    if (!hit) return;
    c[q] += hit;
    uint32_t a = pos > until[q] ? pos : until[q];
    const uint32_t b = pos + w[q];  // (<= L: a window of valid bases lies inside the sequence)
    until[q] = b;
    while (a < b) {
      const uint32_t j = a >> 5, lo = a & 31u;
      const uint32_t n = b - a < 32u - lo ? b - a : 32u - lo;
      if (j != cw[q]) {
        flush(q);
        cw[q] = j;
      }
      cb[q] |= (n == 32u ? 0xFFFFFFFFu : ((1u << n) - 1u)) << lo;
      a += n;
    }
  }
  __device__ __forceinline__ void end(int q, int r) {
    flush(q);
    if (c[q]) atomicAdd(&sites[r], c[q]);
  }
};

template <bool BOTH>
__global__ __launch_bounds__(SCAN_THREADS) void mask_sites_kernel(const uint64_t* __restrict__ words,
                                                                  const uint32_t* __restrict__ valid,
                                                                  const int64_t* __restrict__ offs,
                                                                  const uint32_t* __restrict__ lens, uint64_t n_seq,
                                                                  const int32_t* __restrict__ tables,
                                                                  const MotifRec* __restrict__ recs,
                                                                  const GroupRec* __restrict__ groups,
                                                                  const int32_t* __restrict__ thr, uint32_t* __restrict__ out,
                                                                  unsigned long long* __restrict__ sites,
                                                                  unsigned long long* __restrict__ erased) {
  __shared__ int32_t tab[SCAN_TABLES * 256];
  __shared__ MotifRec mrec[SCAN_MAX_MOTIFS];
  __shared__ int32_t mthr[SCAN_MAX_MOTIFS];
  __shared__ unsigned long long msites[SCAN_MAX_MOTIFS];
  __shared__ unsigned long long berased;
  const GroupRec g = groups[blockIdx.y];
  load_group(g, tables, recs, tab, mrec, [&](int t, const MotifRec& mr) {
    mthr[t] = thr[mr.m];
    msites[t] = 0;
  });
  if (threadIdx.x == 0) berased = 0;
  __syncthreads();
  unsigned long long mine = 0;
  for (uint64_t i = blockIdx.x * (uint64_t)SCAN_THREADS + threadIdx.x; i < n_seq; i += (uint64_t)gridDim.x * SCAN_THREADS) {
    const uint32_t L = lens[i];
    const uint64_t w0 = (uint64_t)offs[i] >> 5;
    MaskVisit<BOTH> v{mrec, mthr, msites, out + w0, 0u, {}, {}, {}, {}, {}, {}};
    walk_sequence<BOTH>(words + w0, valid ? valid + w0 : nullptr, L, tab, mrec, g.m1 - g.m0, v);
    mine += v.erased;
  }
  if (mine) atomicAdd(&berased, mine);
  __syncthreads();
  for (int t = threadIdx.x; t < g.m1 - g.m0; t += SCAN_THREADS)
    if (msites[t]) atomicAdd(&sites[mrec[t].m], msites[t]);
  if (threadIdx.x == 0 && berased) atomicAdd(erased, berased);
}

// ---- pengk_pack_scan_sizes / pengk_pack_scan --------------------------------------------------------------------------
constexpr int PACK_THREADS = 256;
constexpr int PS_PER = 8;                        // prefix sums: elements per thread ...
constexpr int PS_TILE = PACK_THREADS * PS_PER;   // ... and per workgroup
enum { TOT_WINDOWS = 0, TOT_BOUND, TOT_MAX_LEN, TOT_NOT_WHOLE, TOT_BASES, TOT_ITEMS, TOT_N };

// the first position >= i of a sequence of L bases that holds no valid base (L: none); vp NULL: every base valid
__device__ __forceinline__ uint64_t first_invalid(const uint32_t* vp, uint32_t L, uint64_t i) {
  if (!vp) return L;
  uint32_t k = (uint32_t)(i >> 5);  // (i < L: word k exists, here and below)
  uint32_t inv = ~tile::valid_word_in(vp, L, k) >> (i & 31u);
  if (inv) return i + (uint32_t)__builtin_ctz(inv);  // (a bit at or beyond L reads as invalid: never past L)
  for (++k; 32ull * k < L; ++k) {
    inv = ~tile::valid_word_in(vp, L, k);
    if (inv) return 32ull * k + (uint32_t)__builtin_ctz(inv);
  }
  return L;
}

// f(run_start, run_len) for every visited run: pack.cpp's for_each_run over validity bits
template <class F>
__device__ __forceinline__ void for_each_run_bits(const uint32_t* vp, uint32_t L, uint32_t W, F&& f) {
  uint64_t i = 0;
  while (i < L) {
    const uint64_t j = first_invalid(vp, L, i);
    if (j - i >= W) {
      f(i, j - i);
      i = j + 2;
    } else {
      i = j + 1;
    }
  }
}

__global__ __launch_bounds__(PACK_THREADS) void pack_measure_kernel(const uint32_t* __restrict__ valid,
                                                                    const int64_t* __restrict__ offs,
                                                                    const uint32_t* __restrict__ lens, uint64_t n_seq, uint32_t W,
                                                                    uint64_t M, unsigned long long* __restrict__ seq_base,
                                                                    unsigned long long* __restrict__ seq_item,
                                                                    unsigned long long* __restrict__ tot) {
  __shared__ unsigned long long sh[4];
  if (threadIdx.x < 4) sh[threadIdx.x] = 0;
  __syncthreads();
  unsigned long long windows = 0, bound = 0, max_len = 0, not_whole = 0;
  for (uint64_t i = blockIdx.x * (uint64_t)PACK_THREADS + threadIdx.x; i < n_seq; i += (uint64_t)gridDim.x * PACK_THREADS) {
    const uint32_t L = lens[i];
    const uint32_t* vp = valid ? valid + ((uint64_t)offs[i] >> 5) : nullptr;
    unsigned long long bases = 0, items = 0;
    uint32_t runs = 0;
    bool whole = false;
    for_each_run_bits(vp, L, W, [&](uint64_t start, uint64_t len) {
      ++runs;
      whole = start == 0 && len == L;
      const uint64_t nwin = len - W + 1;
      bases += len;
      windows += nwin;
      bound += (nwin + W - 1) / W;
      items += (nwin + M - 1) / M;
    });
    seq_base[i] = bases;
    seq_item[i] = items;
    max_len = L > max_len ? L : max_len;
    if (!(runs == 1 && whole)) not_whole = 1;
  }
  if (windows) atomicAdd(&sh[0], windows);
  if (bound) atomicAdd(&sh[1], bound);
  if (max_len) atomicMax(&sh[2], max_len);
  if (not_whole) atomicOr(&sh[3], 1ull);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (sh[0]) atomicAdd(&tot[TOT_WINDOWS], sh[0]);
    if (sh[1]) atomicAdd(&tot[TOT_BOUND], sh[1]);
    if (sh[2]) atomicMax(&tot[TOT_MAX_LEN], sh[2]);
    if (sh[3]) atomicOr(&tot[TOT_NOT_WHOLE], 1ull);
  }
}

// inclusive sum over the workgroup (sh: PACK_THREADS entries; every thread calls it)
__device__ __forceinline__ unsigned long long group_inclusive_sum(unsigned long long v, unsigned long long* sh,
                                                                  unsigned long long* total = nullptr) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int d = 1; d < PACK_THREADS; d <<= 1) {
    const unsigned long long x = t >= d ? sh[t - d] : 0ull;
    __syncthreads();
    sh[t] += x;
    __syncthreads();
  }
  const unsigned long long r = sh[t];
  if (total) *total = sh[PACK_THREADS - 1];
  __syncthreads();
  return r;
}

// Exclusive prefix sums of two arrays of n elements in place (blockIdx.y picks the array), in three launches: the tiles'
// sums, their own exclusive sums (one workgroup per array, which also leaves the grand total), the tiles again.
__global__ __launch_bounds__(PACK_THREADS) void pscan_tiles_kernel(const unsigned long long* __restrict__ a0,
                                                                   const unsigned long long* __restrict__ a1, uint64_t n,
                                                                   uint64_t n_tiles, unsigned long long* __restrict__ part) {
  __shared__ unsigned long long sh[PACK_THREADS];
  const unsigned long long* a = blockIdx.y ? a1 : a0;
  const uint64_t k0 = (uint64_t)blockIdx.x * PS_TILE + (uint64_t)threadIdx.x * PS_PER;
  unsigned long long s = 0;
  for (int r = 0; r < PS_PER; ++r)
    if (k0 + r < n) s += a[k0 + r];
  s = group_inclusive_sum(s, sh);
  if (threadIdx.x == PACK_THREADS - 1) part[blockIdx.y * n_tiles + blockIdx.x] = s;
}

__global__ __launch_bounds__(PACK_THREADS) void pscan_parts_kernel(unsigned long long* __restrict__ part, uint64_t n_tiles,
                                                                   unsigned long long* __restrict__ tot) {
  __shared__ unsigned long long sh[PACK_THREADS];
  unsigned long long* p = part + blockIdx.x * n_tiles;
  unsigned long long carry = 0;
  for (uint64_t b = 0; b < n_tiles; b += PS_TILE) {
    unsigned long long v[PS_PER], s = 0;
    const uint64_t k0 = b + (uint64_t)threadIdx.x * PS_PER;
    for (int r = 0; r < PS_PER; ++r) {
      v[r] = k0 + r < n_tiles ? p[k0 + r] : 0ull;
      s += v[r];
    }
    unsigned long long t = 0;
    unsigned long long e = carry + group_inclusive_sum(s, sh, &t) - s;
    for (int r = 0; r < PS_PER; ++r) {
      if (k0 + r < n_tiles) p[k0 + r] = e;
      e += v[r];
    }
    carry += t;
  }
  if (threadIdx.x == 0) tot[blockIdx.x ? TOT_ITEMS : TOT_BASES] = carry;
}

__global__ __launch_bounds__(PACK_THREADS) void pscan_apply_kernel(unsigned long long* __restrict__ a0,
                                                                   unsigned long long* __restrict__ a1, uint64_t n,
                                                                   uint64_t n_tiles, const unsigned long long* __restrict__ part) {
  __shared__ unsigned long long sh[PACK_THREADS];
  unsigned long long* a = blockIdx.y ? a1 : a0;
  const uint64_t k0 = (uint64_t)blockIdx.x * PS_TILE + (uint64_t)threadIdx.x * PS_PER;
  unsigned long long v[PS_PER], s = 0;
  for (int r = 0; r < PS_PER; ++r) {
    v[r] = k0 + r < n ? a[k0 + r] : 0ull;
    s += v[r];
  }
  unsigned long long e = part[blockIdx.y * n_tiles + blockIdx.x] + group_inclusive_sum(s, sh) - s;
  for (int r = 0; r < PS_PER; ++r) {
    if (k0 + r < n) a[k0 + r] = e;
    e += v[r];
  }
}

// 32 bases of a sequence's words from base t on (those beyond the sequence's words: zero)
__device__ __forceinline__ uint64_t bases_at(const uint64_t* wp, uint32_t nw, uint64_t t) {
  const uint32_t k = (uint32_t)(t >> 5), s = 2u * (uint32_t)(t & 31u);
  uint64_t v = wp[k] >> s;
  if (s && k + 1u < nw) v |= wp[k + 1u] << (64u - s);
  return v;
}

// The write pass: sequence i's runs go to stream positions PENGK_FRONT_PAD_BASES + seq_base[i] on, its items to
// seq_item[i] on.  A stream word that this thread fills from its first base to its last is stored; every other word may
// be shared with a neighbour sequence and is merged with an atomic OR (the buffer is zeroed).  Nothing is written at or
// beyond n_words / n_items: offsets that do not come from pengk_pack_scan_sizes of the same input cannot leave the buffers.
__global__ __launch_bounds__(PACK_THREADS) void pack_write_kernel(const uint64_t* __restrict__ words,
                                                                  const uint32_t* __restrict__ valid,
                                                                  const int64_t* __restrict__ offs,
                                                                  const uint32_t* __restrict__ lens, uint64_t n_seq, uint32_t W,
                                                                  uint64_t M, const unsigned long long* __restrict__ seq_base,
                                                                  const unsigned long long* __restrict__ seq_item,
                                                                  unsigned long long* __restrict__ out_words, uint64_t n_words,
                                                                  unsigned long long* __restrict__ out_items, uint64_t n_items) {
  for (uint64_t i = blockIdx.x * (uint64_t)PACK_THREADS + threadIdx.x; i < n_seq; i += (uint64_t)gridDim.x * PACK_THREADS) {
    const uint32_t L = lens[i];
    const uint32_t nw = (L + 31u) >> 5;
    const uint64_t w0 = (uint64_t)offs[i] >> 5;
    const uint64_t* wp = words + w0;
    uint64_t g = PENGK_FRONT_PAD_BASES + seq_base[i];  // next stream position
    uint64_t it = seq_item[i];
    unsigned long long acc = 0;  // bits gathered for word g >> 5
    bool mine = false;           // ... which this thread began at its first base
    for_each_run_bits(valid ? valid + w0 : nullptr, L, W, [&](uint64_t start, uint64_t len) {
      const uint64_t run0 = g;
      uint64_t t = start, rem = len;
      while (rem) {
        const uint32_t sh = (uint32_t)(g & 31u);
        const uint32_t n = rem < 32u - sh ? (uint32_t)rem : 32u - sh;
        if (sh == 0) mine = true;
        const uint64_t v = bases_at(wp, nw, t);
        acc |= (n == 32u ? v : v & ((1ull << (2u * n)) - 1ull)) << (2u * sh);
        g += n;
        t += n;
        rem -= n;
        if ((g & 31u) == 0) {
          const uint64_t word = (g >> 5) - 1;
          if (word < n_words && acc) {
            if (mine) out_words[word] = acc;
            else atomicOr(&out_words[word], acc);
          }
          acc = 0;
          mine = false;
        }
      }
      const uint64_t nwin = len - W + 1;
      for (uint64_t f = 0; f < nwin; f += M) {
        const uint64_t k = nwin - f < M ? nwin - f : M;
        if (it < n_items) out_items[it] = (run0 + f) | (k << ITEM_NW_SHIFT) | ((uint64_t)(f ? 1 : 0) << ITEM_CONT_SHIFT);
        ++it;
      }
    });
    if (acc && (g >> 5) < n_words) atomicOr(&out_words[g >> 5], acc);
  }
}

int check_pack_args(const char* who, int W, int* item_windows) {
  if (!valid_w(W)) return fail(PENGK_ERR_ARG, "%s: pattern length %d unsupported (even, %d..%d)", who, W, PENGK_MIN_W, PENGK_MAX_W);
  if (*item_windows == 0) *item_windows = PENGK_DEFAULT_ITEM_WINDOWS;
  if (*item_windows < PENGK_MIN_ITEM_WINDOWS || *item_windows > 65535)
    return fail(PENGK_ERR_ARG, "%s: item_windows %d out of range [%d,65535]", who, *item_windows, PENGK_MIN_ITEM_WINDOWS);
  return PENGK_OK;
}

}  // namespace
}  // namespace pengk

using namespace pengk;

extern "C" {

int pengk_mask_sites(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                     const uint32_t* d_lens, uint64_t n_seq, int n_motifs, const int32_t* h_S, const int32_t* h_len,
                     int both_strands, const int32_t* h_thr, uint32_t* d_out_valid, uint64_t* d_sites, uint64_t* d_erased) {
  if (!ctx || n_motifs < 0 || (n_motifs && (!h_S || !h_len || !h_thr || !d_sites)) ||
      (n_seq && (!d_offs || !d_lens || !d_out_valid)) || (n_seq && n_motifs && (!d_words || !d_erased)))
    return fail(PENGK_ERR_ARG, "pengk_mask_sites: bad argument");
  if (n_seq && d_out_valid == d_valid) return fail(PENGK_ERR_ARG, "pengk_mask_sites: the output buffer must differ from the input");
  int rc = check_motifs("pengk_mask_sites", n_motifs, h_S, h_len);
  if (rc) return rc;
  rc = enter(ctx);
  if (rc) return rc;
  if (n_seq == 0) return PENGK_OK;
  StagedMotifs st;
  if (n_motifs) {  // (synchronises with the stream: before the first launch of this call)
    rc = stage_motifs(ctx, n_motifs, h_S, h_len, both_strands ? 2 : 1, h_thr, &st);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(mask_init_kernel, dim3(grid_for(ctx, n_seq, 256, 16)), dim3(256), 0, ctx->stream, d_valid, d_offs, d_lens,
                     n_seq, d_out_valid);
  PENGK_HIP(hipGetLastError());
  if (n_motifs == 0) return PENGK_OK;
  const dim3 grid(grid_for(ctx, n_seq, SCAN_THREADS, 8), (unsigned)st.n_groups);
  unsigned long long* s = (unsigned long long*)d_sites;
  unsigned long long* e = (unsigned long long*)d_erased;
  if (both_strands)
    hipLaunchKernelGGL(mask_sites_kernel<true>, grid, dim3(SCAN_THREADS), 0, ctx->stream, d_words, d_valid, d_offs, d_lens, n_seq,
                       st.tables, st.recs, st.groups, st.thr, d_out_valid, s, e);
  else
    hipLaunchKernelGGL(mask_sites_kernel<false>, grid, dim3(SCAN_THREADS), 0, ctx->stream, d_words, d_valid, d_offs, d_lens, n_seq,
                       st.tables, st.recs, st.groups, st.thr, d_out_valid, s, e);
  PENGK_HIP(hipGetLastError());
  return PENGK_OK;
}

int pengk_pack_scan_sizes(pengk_ctx* ctx, const uint32_t* d_valid, const int64_t* d_offs, const uint32_t* d_lens, uint64_t n_seq,
                          int W, int item_windows, uint64_t* d_seq_base, uint64_t* d_seq_item, pengk_packed* out) {
  if (!ctx || !out || (n_seq && (!d_offs || !d_lens || !d_seq_base || !d_seq_item)))
    return fail(PENGK_ERR_ARG, "pengk_pack_scan_sizes: bad argument");
  memset(out, 0, sizeof *out);
  int rc = check_pack_args("pengk_pack_scan_sizes", W, &item_windows);
  if (rc) return rc;
  rc = enter(ctx);
  if (rc) return rc;
  unsigned long long tot[TOT_N] = {0};
  if (n_seq) {
    const uint64_t n_tiles = (n_seq + PS_TILE - 1) / PS_TILE;
    rc = ensure_scratch(ctx, &ctx->d_sites, &ctx->sites_bytes, (TOT_N + 2 * n_tiles) * sizeof(uint64_t));
    if (rc) return rc;
    unsigned long long* d_tot = (unsigned long long*)ctx->d_sites;
    unsigned long long* part = d_tot + TOT_N;
    unsigned long long* sb = (unsigned long long*)d_seq_base;
    unsigned long long* si = (unsigned long long*)d_seq_item;
    PENGK_HIP(hipMemsetAsync(d_tot, 0, TOT_N * sizeof(uint64_t), ctx->stream));
    hipLaunchKernelGGL(pack_measure_kernel, dim3(grid_for(ctx, n_seq, PACK_THREADS, 16)), dim3(PACK_THREADS), 0, ctx->stream,
                       d_valid, d_offs, d_lens, n_seq, (uint32_t)W, (uint64_t)item_windows, sb, si, d_tot);
    hipLaunchKernelGGL(pscan_tiles_kernel, dim3((unsigned)n_tiles, 2), dim3(PACK_THREADS), 0, ctx->stream, sb, si, n_seq, n_tiles, part);
    hipLaunchKernelGGL(pscan_parts_kernel, dim3(2), dim3(PACK_THREADS), 0, ctx->stream, part, n_tiles, d_tot);
    hipLaunchKernelGGL(pscan_apply_kernel, dim3((unsigned)n_tiles, 2), dim3(PACK_THREADS), 0, ctx->stream, sb, si, n_seq, n_tiles, part);
    PENGK_HIP(hipGetLastError());
    PENGK_HIP(hipMemcpyAsync(tot, d_tot, sizeof tot, hipMemcpyDeviceToHost, ctx->stream));
    PENGK_HIP(hipStreamSynchronize(ctx->stream));
  }
  if (PENGK_FRONT_PAD_BASES + tot[TOT_BASES] > ITEM_WS_MASK)
    return fail(PENGK_ERR_RANGE, "packed stream exceeds 2^40 bases; shard the input");
  out->n_words = (PENGK_FRONT_PAD_BASES + tot[TOT_BASES] + 31) / 32 + 4;  // >= 96 zero bases behind the data
  out->n_items = tot[TOT_ITEMS];
  out->n_bases = tot[TOT_BASES];
  out->n_windows = tot[TOT_WINDOWS];
  out->max_bin_bound = tot[TOT_BOUND];
  out->n_sequences = n_seq;
  out->max_len = tot[TOT_MAX_LEN];
  out->W = W;
  out->item_windows = item_windows;
  out->all_whole = tot[TOT_NOT_WHOLE] ? 0 : 1;
  return PENGK_OK;
}

int pengk_pack_scan(pengk_ctx* ctx, const uint64_t* d_words, const uint32_t* d_valid, const int64_t* d_offs,
                    const uint32_t* d_lens, uint64_t n_seq, int W, int item_windows, const uint64_t* d_seq_base,
                    const uint64_t* d_seq_item, uint64_t* d_out_words, uint64_t n_words, uint64_t* d_out_items, uint64_t n_items) {
  if (!ctx || !d_out_words || n_words < (PENGK_FRONT_PAD_BASES + 31) / 32 + 4 || (n_items && !d_out_items) ||
      (n_seq && (!d_words || !d_offs || !d_lens || !d_seq_base || !d_seq_item)))
    return fail(PENGK_ERR_ARG, "pengk_pack_scan: bad argument");
  int rc = check_pack_args("pengk_pack_scan", W, &item_windows);
  if (rc) return rc;
  rc = enter(ctx);
  if (rc) return rc;
  PENGK_HIP(hipMemsetAsync(d_out_words, 0, n_words * sizeof(uint64_t), ctx->stream));
  if (n_seq == 0) return PENGK_OK;
  hipLaunchKernelGGL(pack_write_kernel, dim3(grid_for(ctx, n_seq, PACK_THREADS, 16)), dim3(PACK_THREADS), 0, ctx->stream, d_words,
                     d_valid, d_offs, d_lens, n_seq, (uint32_t)W, (uint64_t)item_windows, (const unsigned long long*)d_seq_base,
                     (const unsigned long long*)d_seq_item, (unsigned long long*)d_out_words, n_words,
                     (unsigned long long*)d_out_items, n_items);
  PENGK_HIP(hipGetLastError());
  return PENGK_OK;
}

}  // extern "C"
