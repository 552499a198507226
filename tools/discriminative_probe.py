#!/usr/bin/env python3
"""What the control null costs (GPU box):  python tools/discriminative_probe.py [--W 10 12] [--nseq 2000000] [--reps 15]

One process, both strands, k = max_k = 2.  A synthetic input and a synthetic control of the same size are counted
(pengk_count, timed each), mirrored, and then pengk_pattern_stats and pengk_pattern_stats_control run on the SAME
tables, alternating, `reps` windows of `batch` launches each between two HIP events after a warm-up of both; median and
best per launch, and the ratio of the medians.  At W >= 12 also with sweep_pairs = 0 (the per-pattern kernel).  The
yardstick is the existing sweep in the same process.  Before anything is timed the new entry with an empty control
(Lc = 0) must return the existing sweep's bits."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import peng_motif_amd as pk  # noqa: E402


def timed(ctx, fn, t0, t1, batch):
    ctx.record(t0)
    for _ in range(batch):
        fn()
    ctx.record(t1)
    return ctx.elapsed_ms(t0, t1) / batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--W", type=int, nargs="+", default=[10, 12])
    ap.add_argument("--nseq", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--batch", type=int, default=20)
    a = ap.parse_args()
    ctx = pk.Context(0)
    t0, t1 = ctx.timer(), ctx.timer()
    print("library: %s" % os.path.relpath(pk.LIB_PATH, ROOT), flush=True)
    for W in a.W:
        count_ms = {}
        tables = {}
        for name, seed in (("control", 7), ("input", 1)):  # (the input last: it stays attached)
            ctx.synth(seed, 0, a.nseq, 200, W)
            counts, ltot, bg = ctx.count_bg(True)
            ms = sorted(timed(ctx, lambda: ctx.count(True, counts, ltot), t0, t1, 1) for _ in range(5))
            count_ms[name] = ms[len(ms) // 2]
            ctx.mirror(W, counts)
            tables[name] = (counts, ltot, bg)
        counts, ltot, bg = tables["input"]
        ctrl, lc, _ = tables["control"]
        V = ctx.bg_model(tables["control"][2], 2)
        print("W=%d nseq=%d x 200 bp, both strands: pengk_count input %.3f ms, control %.3f ms (median of 5)"
              % (W, a.nseq, count_ms["input"], count_ms["control"]), flush=True)
        for pairs in ((1, 0) if W >= 12 else (1,)):
            ctx.set_option("sweep_pairs", pairs)
            plain = ctx.pattern_stats(W, True, 2, 2, V, ltot, counts)
            held = ctx.pattern_stats_control(W, True, 2, 2, V, ltot, counts, ctrl, lc, 1.0)
            # an empty control must leave the existing sweep's bits
            zero = ctx.to_device(np.zeros(1, np.uint64))
            same = ctx.pattern_stats_control(W, True, 2, 2, V, ltot, counts, ctrl, zero, 1.0)
            for x, y in zip(plain, same):
                assert x.to_host().tobytes() == y.to_host().tobytes(), "Lc = 0 differs from pengk_pattern_stats"
            raised = int((held[0].to_host()[2] != plain[0].to_host()[2]).sum())
            run_plain = lambda: ctx.pattern_stats(W, True, 2, 2, V, ltot, counts, *plain)  # noqa: E731
            run_held = lambda: ctx.pattern_stats_control(W, True, 2, 2, V, ltot, counts, ctrl, lc, 1.0, *held)  # noqa: E731
            for fn in (run_plain, run_held):
                timed(ctx, fn, t0, t1, a.batch)
            ms = {"plain": [], "held": []}
            for _ in range(a.reps):
                ms["plain"].append(timed(ctx, run_plain, t0, t1, a.batch))
                ms["held"].append(timed(ctx, run_held, t0, t1, a.batch))
            med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
            kernel = "twin-tile" if (W >= 12 and pairs) else "per-pattern"
            print("W=%d %s kernel: pengk_pattern_stats median %.4f ms (best %.4f, worst %.4f) | pengk_pattern_stats_control median %.4f ms "
                  "(best %.4f, worst %.4f) | ratio %.3f | %d windows of %d launches each, alternating | control raises bgprob[2] of %d patterns of %d"
                  % (W, kernel, med["plain"], min(ms["plain"]), max(ms["plain"]), med["held"], min(ms["held"]), max(ms["held"]),
                     med["held"] / med["plain"], a.reps, a.batch, raised, 4 ** W), flush=True)
            for d in plain + held + same:
                d.free()
        ctx.set_option("sweep_pairs", 1)
    ctx.close()


if __name__ == "__main__":
    main()
