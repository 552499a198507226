#!/usr/bin/env python3
"""What the GC-stratified null costs (GPU box):  python tools/strata_probe.py [--n-seq 10000000] [--L 200] [--gc-bins 10]
                                                                             [--W 10 12] [--nseq 2000000] [--reps 15]

One process.
  count   on the device-generated configs[2] input (pengk_synth_scan_sequences: 10M x 200 bp): pengk_strata_bg_count
          beside pengk_seq_strata (one bandwidth-bound pass over the same words: the floor) and pengk_position_count (K = 6,
          20 bins of 10 from the centre, both strands: one LDS add per base), alternating, `reps` rounds between two HIP
          events each after a warm-up of all; the new entry under the input's own strata and with every sequence in one
          stratum.  Median, best and worst, and the ratios of the medians.
  sweep   at every W, both strands, k = max_k = 2: a synthetic input is counted and mirrored, then pengk_pattern_stats and
          pengk_pattern_stats_strata (S = gc-bins and S = 16 tables, equal weights) run on the SAME tables, alternating,
          `reps` windows of `batch` launches each; at W >= 12 the existing sweep under both of its kernels.  Before anything
          is timed the new entry with one non-zero weight must return the existing sweep's bits."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import peng_motif_amd as pk  # noqa: E402


def timed(ctx, fn, t0, t1, batch=1):
    ctx.record(t0)
    for _ in range(batch):
        fn()
    ctx.record(t1)
    return ctx.elapsed_ms(t0, t1) / batch


def alternating(ctx, fns, t0, t1, reps, batch=1):
    """name -> sorted per-launch times: every function warmed up once, then `reps` rounds of all of them in turn"""
    for fn in fns.values():
        timed(ctx, fn, t0, t1, batch)
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ms[k].append(timed(ctx, fn, t0, t1, batch))
    return {k: sorted(v) for k, v in ms.items()}


def show(name, v):
    return "%s median %.4f ms (best %.4f, worst %.4f)" % (name, v[len(v) // 2], v[0], v[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-seq", type=int, default=10_000_000)
    ap.add_argument("--L", type=int, default=200)
    ap.add_argument("--gc-bins", type=int, default=10)
    ap.add_argument("--W", type=int, nargs="+", default=[10, 12])
    ap.add_argument("--nseq", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--batch", type=int, default=20)
    a = ap.parse_args()
    n, L, G = a.n_seq, a.L, a.gc_bins
    ctx = pk.Context(0)
    t0, t1 = ctx.timer(), ctx.timer()
    print("library: %s" % os.path.relpath(pk.LIB_PATH, ROOT), flush=True)

    # ---- the counters ----
    scan = ctx.synth_scan(1, 0, n, L)
    stratum, hist = ctx.seq_strata(scan, G, False)
    h = hist.to_host()
    one = ctx.to_device(np.zeros(n, np.uint16))
    bg, win = ctx.to_device(np.zeros((G, 84), np.uint64)), ctx.to_device(np.zeros(G, np.uint64))
    pos = ctx.to_device(np.zeros((20, 4096), np.uint64))
    ctx.strata_bg_count(scan, stratum, G, 10, bg=bg, windows=win)
    got = bg.to_host()
    assert int(got[:, :4].sum()) == n * L and int(win.to_host().sum()) == n * (L - 9), "the counters do not add up"
    ms = alternating(ctx, {
        "pengk_seq_strata": lambda: ctx.seq_strata(scan, G, False, stratum=stratum, hist=hist),
        "pengk_position_count": lambda: ctx.position_count(scan, 6, 2, 10, 20, True, counts=pos),
        "pengk_strata_bg_count": lambda: ctx.strata_bg_count(scan, stratum, G, 10, bg=bg, windows=win),
        "pengk_strata_bg_count, one stratum": lambda: ctx.strata_bg_count(scan, one, G, 10, bg=bg, windows=win),
    }, t0, t1, a.reps)
    med = {k: v[len(v) // 2] for k, v in ms.items()}
    words_bytes = n * ((L + 31) // 32) * 12 + n * 14
    print("count: %d x %d bp, %d GC bins, %d in use (largest %.1f %% of the sequences), %d rounds, alternating"
          % (n, L, G, int((h[:G] > 0).sum()), 100.0 * h[:G].max() / max(1, h[:G].sum()), a.reps), flush=True)
    for k, v in ms.items():
        print("  " + show(k, v), flush=True)
    print("  pengk_strata_bg_count / pengk_seq_strata %.2f, / pengk_position_count %.3f; one stratum / own strata %.3f; %.0f GB/s of "
          "words, validity, offsets and strata" % (med["pengk_strata_bg_count"] / med["pengk_seq_strata"],
                                                   med["pengk_strata_bg_count"] / med["pengk_position_count"],
                                                   med["pengk_strata_bg_count, one stratum"] / med["pengk_strata_bg_count"],
                                                   words_bytes / med["pengk_strata_bg_count"] / 1e6), flush=True)
    del scan, stratum, one, pos

    # ---- the sweep ----
    for W in a.W:
        ctx.synth(1, 0, a.nseq, 200, W)
        counts, ltot, bgc = ctx.count_bg(True)
        ctx.mirror(W, counts)
        V = ctx.bg_model(bgc, 2).to_host()
        for S in sorted({G, 16}):
            Vs = np.stack([V] * S)
            for s in range(1, S):  # (other models: the rows of the conditional tables rolled)
                Vs[s, 0:4] = np.roll(V[0:4], s % 4)
                Vs[s, 4:20] = np.roll(V[4:20].reshape(4, 4), s % 4, axis=1).reshape(-1)
                Vs[s, 20:84] = np.roll(V[20:84].reshape(16, 4), s % 4, axis=1).reshape(-1)
            d_V, d_Vs = ctx.to_device(V), ctx.to_device(Vs)
            weights = np.full(S, 1000, np.uint64)
            first = np.zeros(S, np.uint64)
            first[0] = 12345
            plain = ctx.pattern_stats(W, True, 2, 2, d_V, ltot, counts)
            mixed = ctx.pattern_stats_strata(W, True, 2, 2, d_Vs, first, ltot, counts)
            for x, y in zip(plain, mixed):
                assert x.to_host().tobytes() == y.to_host().tobytes(), "one non-zero weight differs from pengk_pattern_stats"
            fns = {"pengk_pattern_stats_strata": lambda: ctx.pattern_stats_strata(W, True, 2, 2, d_Vs, weights, ltot, counts,
                                                                                 bgprob=mixed[0], expected=mixed[1], logp=mixed[2], z=mixed[3])}
            for pairs in ((1, 0) if W >= 12 else (1,)):
                def run_plain(pairs=pairs):
                    ctx.set_option("sweep_pairs", pairs)
                    ctx.pattern_stats(W, True, 2, 2, d_V, ltot, counts, *plain)
                fns["pengk_pattern_stats (%s)" % ("twin-tile" if W >= 12 and pairs else "per-pattern")] = run_plain
            ms = alternating(ctx, fns, t0, t1, a.reps, a.batch)
            ctx.set_option("sweep_pairs", 1)
            med = {k: v[len(v) // 2] for k, v in ms.items()}
            print("sweep: W=%d, both strands, %d strata, %d windows of %d launches each, alternating" % (W, S, a.reps, a.batch), flush=True)
            for k, v in ms.items():
                print("  " + show(k, v), flush=True)
            new = med["pengk_pattern_stats_strata"]
            print("  " + "; ".join("strata / %s %.2f" % (k.split("(")[1].rstrip(")"), new / v) for k, v in med.items() if "(" in k)
                  + "; %.0f GB/s written by the stratified sweep" % (28.0 * 4 ** W / new / 1e6), flush=True)
            for d in plain + mixed:
                d.free()
    ctx.close()


if __name__ == "__main__":
    main()
