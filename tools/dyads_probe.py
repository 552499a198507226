"""Times --dyads in one process on the device-generated configs[2] input (pengk_synth_scan_sequences: 10M x 200 bp):
  count   pengk_dyad_count at max_gap G on both strands over the input as it is, over the same input with a 30-base poly-A
          in every tenth sequence (bases 50 .. 79: the hot bin AAA n AAA), and on the plus strand alone
  beside  pengk_motif_scan of N motifs of width 10-14 on both strands
  long    one sequence of 200 000 bases
Device passes between device events, the median of --reps after one warm-up.  Prints one JSON line.
  python tools/dyads_probe.py [--n-seq 10000000] [--L 200] [--G 20] [--motifs 16] [--reps 5]"""
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
    ap.add_argument("--G", type=int, default=20)
    ap.add_argument("--motifs", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    n, L, G = a.n_seq, a.L, a.G
    ctx = pk.Context(0)
    scan = ctx.synth_scan(1, 0, n, L)
    res = {"probe": "dyads", "n_seq": n, "L": L, "G": G, "motifs": a.motifs, "reps": a.reps}

    counts = ctx.to_device(np.zeros((G + 1, 4096), np.uint64))
    mono = ctx.to_device(np.zeros(64, np.uint64))
    res["count_ms"] = median_ms(ctx, lambda: ctx.dyad_count(scan, G, True, counts=counts, mono=mono), a.reps)
    c = counts.to_host()  # (added to: reps + 1 times the same figures)
    res["occurrences"] = int(c.sum()) // (a.reps + 1)
    res["largest_bin"] = int(c.max()) // (a.reps + 1)
    res["count_plus_ms"] = median_ms(ctx, lambda: ctx.dyad_count(scan, G, False, counts=counts, mono=mono), a.reps)
    res["count_all_valid_ms"] = median_ms(ctx, lambda: ctx.dyad_count(scan, G, True, all_valid=True, counts=counts, mono=mono), a.reps)

    S = motifs(a.motifs, np.random.default_rng(1))
    best = ctx.empty((a.motifs, n), np.int32)
    res["motif_scan_ms"] = median_ms(ctx, lambda: ctx.motif_scan(scan, S, [len(s) for s in S], True, best=best), a.reps)
    del best
    res["count_over_scan"] = res["count_ms"] / res["motif_scan_ms"]

    # ---- a 30-base poly-A in every tenth sequence ----
    if L >= 96:
        wps = (L + 31) // 32
        w = scan[0].to_host().reshape(n, wps)
        w[::10, 1] &= np.uint64((1 << 36) - 1)                      # bases 50 .. 63
        w[::10, 2] &= ~np.uint64((1 << 32) - 1)                     # bases 64 .. 79
        tracts = (ctx.to_device(w.reshape(-1)), scan[1], scan[2], scan[3], n)
        del w
        c2 = ctx.to_device(np.zeros((G + 1, 4096), np.uint64))
        res["count_tracts_ms"] = median_ms(ctx, lambda: ctx.dyad_count(tracts, G, True, counts=c2, mono=mono), a.reps)
        res["tracts_largest_bin"] = int(c2.to_host().max()) // (a.reps + 1)
        res["tracts_over_uniform"] = res["count_tracts_ms"] / res["count_ms"]
        del tracts

    # ---- one sequence of 200 000 bases: 3 125 tiles over the whole grid ----
    one = np.random.default_rng(2).integers(1, 5, 200_000).astype(np.uint8)
    one[::1000] = 0
    lscan = ctx.upload_scan(pk.ScanLayout(one, np.array([0, len(one)], np.int64)))
    res["one_200k_sequence_count_ms"] = median_ms(ctx, lambda: ctx.dyad_count(lscan, G, True), a.reps)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
