#!/usr/bin/env python3
"""What the Markov null of order 3 .. 5 costs (GPU box):  python tools/bg_order_probe.py [--n-seq 10000000] [--L 200]
                                                                                        [--W 10 12] [--nseq 2000000] [--reps 15]

One process.
  count   on the device-generated configs[2] input (pengk_synth_scan_sequences: 10M x 200 bp): pengk_bg_count_order at
          K = 3, 4, 5 beside pengk_strata_bg_count with one stratum (the order-2 counters by ballots), pengk_seq_strata (one
          bandwidth-bound pass over the same words: the floor) and pengk_position_count (K = 6, 20 bins of 10 from the centre,
          both strands: one LDS add per base), alternating, `reps` rounds between two HIP events each after a warm-up of
          all.  Then the same counts on a copy of the input in which every tenth sequence holds a poly-A of 32 bases (one
          word of the layout zeroed): what equal keys cost.  Median, best and worst, and the ratios of the medians.
  sweep   at every W, both strands, k = max_k = 2: a synthetic input is counted and mirrored, then pengk_pattern_stats and
          pengk_pattern_stats_order (K = 3 and 5, a model of random counters) run on the SAME tables, alternating, `reps`
          windows of `batch` launches each; at W >= 12 the existing sweep under both of its kernels.  Before anything is
          timed the new entry at K = 2 on the run's own table must return the existing sweep's bits."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))  # (strata_probe, from wherever this file is started or imported)
import peng_motif_amd as pk  # noqa: E402

from strata_probe import alternating, show  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-seq", type=int, default=10_000_000)
    ap.add_argument("--L", type=int, default=200)
    ap.add_argument("--W", type=int, nargs="+", default=[10, 12])
    ap.add_argument("--nseq", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--batch", type=int, default=20)
    a = ap.parse_args()
    n, L = a.n_seq, a.L
    ctx = pk.Context(0)
    t0, t1 = ctx.timer(), ctx.timer()
    print("library: %s" % os.path.relpath(pk.LIB_PATH, ROOT), flush=True)

    # ---- the counters ----
    scan = ctx.synth_scan(1, 0, n, L)
    stratum, hist = ctx.seq_strata(scan, 10, False)
    one = ctx.to_device(np.zeros(n, np.uint16))
    sbg, win = ctx.to_device(np.zeros((1, 84), np.uint64)), ctx.to_device(np.zeros(1, np.uint64))
    pos = ctx.to_device(np.zeros((20, 4096), np.uint64))
    bg = {K: ctx.to_device(np.zeros(pk.order_table_size(K), np.uint64)) for K in (3, 4, 5)}
    ctx.strata_bg_count(scan, one, 1, 10, bg=sbg, windows=win)
    ctx.bg_count_order(scan, 5, bg=bg[5])
    got = bg[5].to_host()
    assert [int(got[pk.order_table_size(k - 1):pk.order_table_size(k)].sum()) for k in range(6)] == [n * (L - k) for k in range(6)], \
        "the counters do not add up"
    assert np.array_equal(got[:84], sbg.to_host()[0]), "orders 0 .. 2 differ from pengk_strata_bg_count"
    words_bytes = n * ((L + 31) // 32) * 12 + n * 12

    def count_round(scan, title):
        fns = {"pengk_seq_strata": lambda: ctx.seq_strata(scan, 10, False, stratum=stratum, hist=hist),
               "pengk_position_count": lambda: ctx.position_count(scan, 6, 2, 10, 20, True, counts=pos),
               "pengk_strata_bg_count, one stratum": lambda: ctx.strata_bg_count(scan, one, 1, 10, bg=sbg, windows=win)}
        for K in (3, 4, 5):
            fns["pengk_bg_count_order K=%d" % K] = lambda K=K: ctx.bg_count_order(scan, K, bg=bg[K])
        ms = alternating(ctx, fns, t0, t1, a.reps)
        med = {k: v[len(v) // 2] for k, v in ms.items()}
        print("count: %d x %d bp, %s, %d rounds, alternating" % (n, L, title, a.reps), flush=True)
        for k, v in ms.items():
            print("  " + show(k, v), flush=True)
        print("  " + "; ".join("K=%d / strata count %.2f, / seq_strata %.2f, %.0f GB/s of words, validity and offsets"
                               % (K, med["pengk_bg_count_order K=%d" % K] / med["pengk_strata_bg_count, one stratum"],
                                  med["pengk_bg_count_order K=%d" % K] / med["pengk_seq_strata"],
                                  words_bytes / med["pengk_bg_count_order K=%d" % K] / 1e6) for K in (3, 4, 5)), flush=True)

    count_round(scan, "the input as generated")
    words = scan[0].to_host()
    at = (scan[2].to_host()[::10] >> 5) + 2   # bases 64 .. 95 of every tenth sequence
    words[at] = 0
    scan_a = (ctx.to_device(words),) + tuple(scan[1:])
    del words
    count_round(scan_a, "a poly-A of 32 bases in every tenth sequence")
    del scan, scan_a, stratum, one, pos

    # ---- the sweep ----
    rng = np.random.default_rng(1)
    for W in a.W:
        ctx.synth(1, 0, a.nseq, 200, W)
        counts, ltot, bgc = ctx.count_bg(True)
        ctx.mirror(W, counts)
        d_V = ctx.bg_model(bgc, 2)
        plain = ctx.pattern_stats(W, True, 2, 2, d_V, ltot, counts)
        same = ctx.pattern_stats_order(W, True, 2, 2, d_V, 2, d_V, ltot, counts)
        for x, y in zip(plain, same):
            assert x.to_host().tobytes() == y.to_host().tobytes(), "K = 2 on the run's own table differs from pengk_pattern_stats"
        fns = {}
        for K in (3, 5):
            VK = pk.bg_model_order(rng.integers(1, 5000, pk.order_table_size(K)).astype(np.uint64), K, (1.0,) * (K + 1))
            d_VK = ctx.to_device(VK)
            fns["pengk_pattern_stats_order K=%d" % K] = lambda K=K, d_VK=d_VK: ctx.pattern_stats_order(
                W, True, 2, 2, d_V, K, d_VK, ltot, counts, bgprob=same[0], expected=same[1], logp=same[2], z=same[3])
        for pairs in ((1, 0) if W >= 12 else (1,)):
            def run_plain(pairs=pairs):
                ctx.set_option("sweep_pairs", pairs)
                ctx.pattern_stats(W, True, 2, 2, d_V, ltot, counts, *plain)
            fns["pengk_pattern_stats (%s)" % ("twin-tile" if W >= 12 and pairs else "per-pattern")] = run_plain
        ms = alternating(ctx, fns, t0, t1, a.reps, a.batch)
        ctx.set_option("sweep_pairs", 1)
        med = {k: v[len(v) // 2] for k, v in ms.items()}
        print("sweep: W=%d, both strands, %d windows of %d launches each, alternating" % (W, a.reps, a.batch), flush=True)
        for k, v in ms.items():
            print("  " + show(k, v), flush=True)
        for K in (3, 5):
            new = med["pengk_pattern_stats_order K=%d" % K]
            print("  K=%d: " % K + "; ".join("order / %s %.2f" % (k.split("(")[1].rstrip(")"), new / v) for k, v in med.items() if "(" in k)
                  + "; %.0f GB/s written" % (28.0 * 4 ** W / new / 1e6), flush=True)
        for d in plain + same:
            d.free()
    ctx.close()


if __name__ == "__main__":
    main()
