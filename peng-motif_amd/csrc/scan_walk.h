// scan_walk.h -- what every kernel that walks the scan layout shares (score.hip, sites.hip, site_stats.hip, erase.hip):
// motif groups whose 4-mer chunk tables fit in LDS; one thread per sequence slides a 64-base look-ahead buffer over its
// words, so chunk c of the window is byte c of the buffer.  The kernel prologue that loads a group, the walk for both
// table models, and on the host the grouping rule and the staging of a launch's motifs.  DESIGN.md 10.
#pragma once
#include <type_traits>

#include "pengk_internal.h"

namespace pengk {
namespace scan {

constexpr int SCAN_THREADS = 256;
constexpr int SCAN_TABLES = 40;        // 4-mer chunk tables (256 int each) of one motif group in LDS: 40 KiB, 4 groups per CU
constexpr int SCAN_MAX_MOTIFS = SCAN_TABLES;  // (a motif needs at least one table)
constexpr int MAX_CHUNKS = PENGK_MAX_MOTIF_LEN / 4;
constexpr int SCAN_PASS = 1;           // motifs scored side by side in one pass over a sequence (4 measured 1.4x slower: DESIGN.md 10)
constexpr int HIST_THREADS = 256;      // the histogram kernels over best scores and best sites (score.hip, site_stats.hip)

// The table model of a walk: the ints a motif's chunk owns per strand, and whether pair terms lie behind its 4-mer table.
// Order 1 (--dinuc): the 256-entry 4-mer table -- S0 (chunk 0) plus every pair term whose two columns lie
// inside the chunk -- and behind it the 16-entry boundary table of the one pair that straddles chunks c - 1 and c, indexed
// by bits [8c - 2, 8c + 2) of the look-ahead buffer: the last base of byte c - 1 (low) and the first of byte c (chunk 0
// has no such pair; its 16 entries are not read).
struct Order0 {
  static constexpr int STRIDE = 256;
  static constexpr bool PAIRS = false;
};
struct Order1 {
  static constexpr int STRIDE = 256 + 16;
  static constexpr bool PAIRS = true;
};

struct MotifRec {
  int32_t off;    // first table of the motif within its group's tables (ints)
  int32_t w;      // width
  int32_t nch;    // chunk tables per strand: ceil(w / 4)
  int32_t m;      // motif index (row of d_best)
};
struct GroupRec {
  int32_t m0, m1;       // records [m0, m1)
  int32_t table0;       // first int of the group's tables in the table array
  int32_t n_ints;       // their number
};

// The prologue of every scan kernel: the tables and records of the workgroup's group g = groups[blockIdx.y] into the
// kernel's own LDS arrays; each(t, mr) once per record t for what a kernel keeps beside it.  The caller's barrier follows.
template <class Each>
__device__ __forceinline__ void load_group(const GroupRec& g, const int32_t* tables, const MotifRec* recs, int32_t* tab,
                                           MotifRec* mrec, Each each) {
  for (int t = threadIdx.x; t < g.n_ints; t += SCAN_THREADS) tab[t] = tables[g.table0 + t];
  for (int t = threadIdx.x; t < g.m1 - g.m0; t += SCAN_THREADS) {
    const MotifRec mr = recs[g.m0 + t];
    mrec[t] = mr;
    each(t, mr);
  }
}
__device__ __forceinline__ void load_group(const GroupRec& g, const int32_t* tables, const MotifRec* recs, int32_t* tab,
                                           MotifRec* mrec) {
  load_group(g, tables, recs, tab, mrec, [](int, const MotifRec&) {});
}

__device__ __forceinline__ uint32_t byte_of(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3, int c) {
  const uint32_t v = c < 4 ? b0 : c < 8 ? b1 : c < 12 ? b2 : b3;  // (c is a compile-time constant after unrolling)
  return (v >> (8 * (c & 3))) & 0xFFu;
}

__device__ __forceinline__ uint32_t pair_of(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3, int c) {
  // (c >= 1 is a compile-time constant after unrolling; c = 4, 8, 12: the pair crosses a register)
  const uint32_t hi = c < 4 ? b0 : c < 8 ? b1 : c < 12 ? b2 : b3;
  const uint32_t lo = c <= 4 ? b0 : c <= 8 ? b1 : b2;
  const uint32_t v = (c & 3) ? hi >> (8 * (c & 3) - 2) : __builtin_amdgcn_alignbit(hi, lo, 30);
  return v & 15u;
}

// The scan loop every scan kernel shares: one sequence (its words wp, validity words vp -- NULL: every base valid -- and
// length L) walked under the nrec motifs of a group, whose tables follow Model.  For each pass of SCAN_PASS motifs:
// v.begin(q, r) for the pass's slots q (r = r0 + q, the group record; slots q >= np get the pass's first record),
// v.window(q, pos, sf, sr) for every window at base pos whose bases are all valid (sf the + score; sr the - score,
// computed with BOTH only), v.end(q, r) for the slots q < np.
template <bool BOTH, class Model = Order0, class Visit>
__device__ __forceinline__ void walk_sequence(const uint64_t* wp, const uint32_t* vp, uint32_t L,
                                              const int32_t* tab, const MotifRec* mrec, int nrec, Visit& v) {
  const uint32_t nw = (L + 31u) >> 5;
  auto ldw = [&](uint32_t j) -> uint64_t { return j < nw ? wp[j] : 0ull; };
  auto ldv = [&](uint32_t j) -> uint32_t {
    if (j >= nw) return 0u;
    if (vp) return vp[j];
    const uint32_t rem = L - 32u * j;
    return rem >= 32u ? 0xFFFFFFFFu : ((1u << rem) - 1u);
  };
  // SCAN_PASS motifs per pass over the sequence: the buffer's upkeep per base is shared by them
  for (int r0 = 0; r0 < nrec; r0 += SCAN_PASS) {
    const int np = nrec - r0 < SCAN_PASS ? nrec - r0 : SCAN_PASS;
    uint64_t wmask[SCAN_PASS];
    int nch[SCAN_PASS];
    const int32_t* tf[SCAN_PASS];
    int wmin = PENGK_MAX_MOTIF_LEN;
#pragma unroll
    for (int q = 0; q < SCAN_PASS; ++q) {
      const MotifRec mr = mrec[r0 + (q < np ? q : 0)];
      wmask[q] = mr.w >= 64 ? ~0ull : ((1ull << mr.w) - 1ull);
      nch[q] = mr.nch;
      tf[q] = tab + mr.off;
      v.begin(q, r0 + (q < np ? q : 0));
      wmin = q < np && mr.w < wmin ? mr.w : wmin;
    }
    // (a window past the sequence's end has invalid bits: the passes' wider motifs need no bound of their own)
    const uint32_t nwin = L >= (uint32_t)wmin ? L - (uint32_t)wmin + 1u : 0u;
    // look-ahead buffer: bases s .. s+63 of the sequence (b0 low), their validity bits in vb
    const uint64_t x0 = ldw(0), x1 = ldw(1);
    uint32_t b0 = (uint32_t)x0, b1 = (uint32_t)(x0 >> 32), b2 = (uint32_t)x1, b3 = (uint32_t)(x1 >> 32);
    uint64_t vb = (uint64_t)ldv(0) | ((uint64_t)ldv(1) << 32);
    for (uint32_t s = 0, j = 2; s < nwin; ++j) {
      uint64_t fw = ldw(j);
      uint32_t fv = ldv(j);
      const uint32_t cnt = nwin - s < 32u ? nwin - s : 32u;
      for (uint32_t k = 0; k < cnt; ++k) {
#pragma unroll
        for (int q = 0; q < SCAN_PASS; ++q) {
          if (q < np && (vb & wmask[q]) == wmask[q]) {
            int32_t sf = 0, sr = 0;
#pragma unroll
            for (int c = 0; c < MAX_CHUNKS; ++c) {
              if (c < nch[q]) {
                const uint32_t idx = byte_of(b0, b1, b2, b3, c);
                sf += tf[q][c * Model::STRIDE + idx];
                if (BOTH) sr += tf[q][(nch[q] + c) * Model::STRIDE + idx];
                if (Model::PAIRS && c > 0) {
                  const uint32_t px = pair_of(b0, b1, b2, b3, c);
                  sf += tf[q][c * Model::STRIDE + 256 + px];
                  if (BOTH) sr += tf[q][(nch[q] + c) * Model::STRIDE + 256 + px];
                }
              }
            }
            v.window(q, s + k, sf, sr);
          }
        }
        b0 = __builtin_amdgcn_alignbit(b1, b0, 2);
        b1 = __builtin_amdgcn_alignbit(b2, b1, 2);
        b2 = __builtin_amdgcn_alignbit(b3, b2, 2);
        b3 = __builtin_amdgcn_alignbit((uint32_t)fw, b3, 2);
        fw >>= 2;
        vb = (vb >> 1) | ((uint64_t)(fv & 1u) << 63);
        fv >>= 1;
      }
      s += cnt;
    }
#pragma unroll
    for (int q = 0; q < SCAN_PASS; ++q)
      if (q < np) v.end(q, r0 + q);
  }
}

// The best window score of every motif on every sequence (pengk_motif_scan, pengk_motif_scan_dinuc)
template <bool BOTH>
struct BestVisit {
  const MotifRec* mrec;
  int32_t* best_out;
  uint64_t n_seq, i;
  int best[SCAN_PASS];
  __device__ __forceinline__ void begin(int q, int) { best[q] = PENGK_SCORE_SENTINEL; }
  __device__ __forceinline__ void window(int q, uint32_t, int32_t sf, int32_t sr) { best[q] = max(best[q], BOTH ? max(sf, sr) : sf); }
  __device__ __forceinline__ void end(int q, int r) { best_out[(uint64_t)mrec[r].m * n_seq + i] = best[q]; }
};

// The grouping rule (greedy, in motif order): the ints that the chunk tables of a motif of width w take, and whether
// they open a new group behind one that holds `held` ints.  Everything that cuts motifs into groups asks here.
struct MotifFit {
  int need;
  bool opens;
};
inline MotifFit fit_motif(int held, int w, int strands, int stride) {
  const int need = (w + 3) / 4 * strands * stride;
  return MotifFit{need, held + need > SCAN_TABLES * 256};
}

}  // namespace scan

// ---- host side (score.hip): what a scan launch needs of its motifs -----------------------------------------------------
struct StagedMotifs {
  const int32_t* tables = nullptr;
  const scan::MotifRec* recs = nullptr;
  const scan::GroupRec* groups = nullptr;
  const int32_t* thr = nullptr;  // (h_thr given: n_motifs thresholds, by motif index)
  int n_groups = 0;
};
// widths within 1..PENGK_MAX_MOTIF_LEN, log-odds within [-2000, 2000]; `who` names the caller in the message
int check_motifs(const char* who, int n_motifs, const int32_t* h_S, const int32_t* h_len);
// chunk tables, motif records and groups (greedy, in motif order) -- and h_thr when given -- staged in ctx->d_score
int stage_motifs(pengk_ctx* ctx, int n_motifs, const int32_t* h_S, const int32_t* h_len, int strands, const int32_t* h_thr,
                 StagedMotifs* out);
// the same for first-order tables (scan::Order1): h_S0 the first column's terms, h_D the pair terms
int stage_motifs_dinuc(pengk_ctx* ctx, int n_motifs, const int32_t* h_S0, const int32_t* h_D, const int32_t* h_len, int strands,
                       StagedMotifs* out);
// workgroups for `work` elements, per_block each: at most per_cu per compute unit
int grid_for(pengk_ctx* ctx, uint64_t work, uint32_t per_block, uint32_t per_cu);

// f(std::true_type) or f(std::false_type): a kernel's BOTH instantiation picked once, the launch written once
template <class F>
inline auto by_strands(bool both, F&& f) {
  return both ? f(std::true_type{}) : f(std::false_type{});
}

#define SCORE_ENTER(ctx)                   \
  do {                                     \
    int rc_enter_ = ::pengk::enter(ctx);   \
    if (rc_enter_) return rc_enter_;       \
  } while (0)

}  // namespace pengk
