"""Times --positional in one process on the device-generated configs[2] input (pengk_synth_scan_sequences: 10M x 200 bp):
  count   pengk_position_count at width K, B bins of S from the center on both strands over the input as it is, over the
          same input with a 30-base poly-A in every tenth sequence (bases 50 .. 79: one clump head instead of 25 equal
          words), from the start, and on the plus strand alone
  beside  pengk_dyad_count at max_gap G and pengk_motif_scan of N motifs of width 10-14, both on both strands
  long    one sequence of 200 000 bases (only the tiles around its centre are walked)
Device passes between device events, the median of --reps after one warm-up.  Prints one JSON line.
  python tools/positional_probe.py [--n-seq 10000000] [--L 200] [--K 6] [--S 10] [--B 20] [--G 20] [--motifs 16] [--reps 5]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import peng_motif_amd as pk  # noqa: E402
from erase_probe import median_ms, motifs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-seq", type=int, default=10_000_000)
    ap.add_argument("--L", type=int, default=200)
    ap.add_argument("--K", type=int, default=6)
    ap.add_argument("--S", type=int, default=10)
    ap.add_argument("--B", type=int, default=20)
    ap.add_argument("--G", type=int, default=20)
    ap.add_argument("--motifs", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    n, L, K, S, B, G = a.n_seq, a.L, a.K, a.S, a.B, a.G
    ctx = pk.Context(0)
    scan = ctx.synth_scan(1, 0, n, L)
    res = {"probe": "positional", "n_seq": n, "L": L, "K": K, "S": S, "B": B, "G": G, "motifs": a.motifs, "reps": a.reps}

    counts = ctx.to_device(np.zeros((B, 4 ** K), np.uint64))
    res["count_ms"] = median_ms(ctx, lambda: ctx.position_count(scan, K, 2, S, B, True, counts=counts), a.reps)
    c = counts.to_host()  # (added to: reps + 1 times the same figures)
    res["heads_counted"] = int(c.sum()) // (a.reps + 1)
    res["largest_bin"] = int(c.max()) // (a.reps + 1)
    res["count_start_ms"] = median_ms(ctx, lambda: ctx.position_count(scan, K, 0, S, B, True, counts=counts), a.reps)
    res["count_plus_ms"] = median_ms(ctx, lambda: ctx.position_count(scan, K, 2, S, B, False, counts=counts), a.reps)
    res["count_all_valid_ms"] = median_ms(ctx, lambda: ctx.position_count(scan, K, 2, S, B, True, all_valid=True, counts=counts), a.reps)

    dc = ctx.to_device(np.zeros((G + 1, 4096), np.uint64))
    dm = ctx.to_device(np.zeros(64, np.uint64))
    res["dyad_count_ms"] = median_ms(ctx, lambda: ctx.dyad_count(scan, G, True, counts=dc, mono=dm), a.reps)
    del dc
    M = motifs(a.motifs, np.random.default_rng(1))
    best = ctx.empty((a.motifs, n), np.int32)
    res["motif_scan_ms"] = median_ms(ctx, lambda: ctx.motif_scan(scan, M, [len(s) for s in M], True, best=best), a.reps)
    del best
    res["count_over_dyads"] = res["count_ms"] / res["dyad_count_ms"]
    res["count_over_scan"] = res["count_ms"] / res["motif_scan_ms"]

    # ---- a 30-base poly-A in every tenth sequence ----
    if L >= 96:
        wps = (L + 31) // 32
        w = scan[0].to_host().reshape(n, wps)
        w[::10, 1] &= np.uint64((1 << 36) - 1)                      # bases 50 .. 63
        w[::10, 2] &= ~np.uint64((1 << 32) - 1)                     # bases 64 .. 79
        tracts = (ctx.to_device(w.reshape(-1)), scan[1], scan[2], scan[3], n)
        del w
        c2 = ctx.to_device(np.zeros((B, 4 ** K), np.uint64))
        res["count_tracts_ms"] = median_ms(ctx, lambda: ctx.position_count(tracts, K, 2, S, B, True, counts=c2), a.reps)
        res["tracts_poly_a_heads"] = int(c2.to_host()[:, 0].sum()) // (a.reps + 1)
        res["tracts_over_uniform"] = res["count_tracts_ms"] / res["count_ms"]
        del tracts

    # ---- one sequence of 200 000 bases: B * S positions either side of the centre are in range ----
    one = np.random.default_rng(2).integers(1, 5, 200_000).astype(np.uint8)
    one[::1000] = 0
    lscan = ctx.upload_scan(pk.ScanLayout(one, np.array([0, len(one)], np.int64)))
    res["one_200k_sequence_count_ms"] = median_ms(ctx, lambda: ctx.position_count(lscan, K, 2, S, B, True), a.reps)
    res["one_200k_sequence_all_in_range_ms"] = median_ms(ctx, lambda: ctx.position_count(lscan, K, 2, 4096, 64, True), a.reps)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
