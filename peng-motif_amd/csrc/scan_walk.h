// scan_walk.h -- the walk over one sequence of the scan layout that every scan kernel shares (score.hip, erase.hip):
// motif groups whose 4-mer chunk tables fit in LDS; one thread per sequence slides a 64-base look-ahead buffer over its
// words, so chunk c of the window is byte c of the buffer.  DESIGN.md 10.
#pragma once
#include "pengk_internal.h"

namespace pengk {
namespace scan {

constexpr int SCAN_THREADS = 256;
constexpr int SCAN_TABLES = 40;        // 4-mer chunk tables (256 int each) of one motif group in LDS: 40 KiB, 4 groups per CU
constexpr int SCAN_MAX_MOTIFS = SCAN_TABLES;  // (a motif needs at least one table)
constexpr int MAX_CHUNKS = PENGK_MAX_MOTIF_LEN / 4;
constexpr int SCAN_PASS = 1;           // motifs scored side by side in one pass over a sequence (4 measured 1.4x slower: DESIGN.md 10)

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

__device__ __forceinline__ uint32_t byte_of(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3, int c) {
  const uint32_t v = c < 4 ? b0 : c < 8 ? b1 : c < 12 ? b2 : b3;  // (c is a compile-time constant after unrolling)
  return (v >> (8 * (c & 3))) & 0xFFu;
}

// The scan loop every scan kernel shares: one sequence (its words wp, validity words vp -- NULL: every base valid -- and
// length L) walked under the nrec motifs of a group.  For each pass of SCAN_PASS motifs: v.begin(q, r) for the pass's
// slots q (r = r0 + q, the group record; slots q >= np get the pass's first record), v.window(q, pos, sf, sr) for every
// window at base pos whose bases are all valid (sf the + score; sr the - score, computed with BOTH only), v.end(q, r)
// for the slots q < np.
template <bool BOTH, class Visit>
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
                sf += tf[q][c * 256 + idx];
                if (BOTH) sr += tf[q][(nch[q] + c) * 256 + idx];
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
// workgroups for `work` elements, per_block each: at most per_cu per compute unit
int grid_for(pengk_ctx* ctx, uint64_t work, uint32_t per_block, uint32_t per_cu);

}  // namespace pengk
