"""Times the first-order motif models on the device (include/pengk.h, "first-order motif models") for N motifs over the
device-generated configs[2] input (pengk_synth_scan_sequences: 10M x 200 bp): the first-order scan beside the order-0
scan of the same widths (the yardstick, in the same process, the two alternating), and the pair profiles beside the single
profiles at thresholds few sequences pass (weak, p-value P) and every sequence passes (strong), each between device events
(median of --reps after one warm-up).  Before timing, the first-order scan of the degenerate models must give the order-0
scan's histograms.  Prints one JSON line.
  python tools/dinuc_probe.py [--n-seq 10000000] [--L 200] [--motifs 16] [--p 1e-4] [--flank 0] [--reps 5] [--plus]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import peng_motif_amd as pk  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-seq", type=int, default=10_000_000)
    ap.add_argument("--L", type=int, default=200)
    ap.add_argument("--motifs", type=int, default=16)
    ap.add_argument("--p", type=float, default=1e-4)
    ap.add_argument("--flank", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--plus", action="store_true")
    a = ap.parse_args()
    ctx = pk.Context(0)
    n, L = a.n_seq, a.L
    scan = ctx.synth_scan(1, 0, n, L)
    rng = np.random.default_rng(16)
    widths = [10 + (m % 5) for m in range(a.motifs)]  # 10..14
    S = [rng.integers(-400, 200, (w, 4)).astype(np.int32) for w in widths]
    S0 = [rng.integers(-400, 200, 4).astype(np.int32) for _ in widths]
    D = [rng.integers(-400, 200, (w, 16)).astype(np.int32) for w in widths]
    bg = np.full(4, 0.25, np.float32)
    weak = []
    for s in S:
        lo, tail = pk.score_tail_pvalues(s, bg)
        weak.append(pk.score_threshold(tail, lo, a.p))
    strong = [-2 ** 31 + 1] * len(S)  # every sequence with a window has a site
    both = not a.plus
    M = len(widths)
    best = ctx.empty((M, n), np.int32)
    site = ctx.empty((M, n), np.uint64)

    # the degenerate models: the order-0 scan's scores
    lo = [int(s.min(axis=1).sum()) for s in S]
    hi = [int(s.max(axis=1).sum()) for s in S]
    ctx.motif_scan(scan, S, widths, both, best=best)
    h0 = ctx.score_histograms(best, n, lo, hi)[0].to_host()
    ctx.motif_scan_dinuc(scan, [s[0] for s in S], [np.repeat(s[:, None, :], 4, axis=1).reshape(-1, 16) for s in S], widths, both,
                         best=best)
    h1 = ctx.score_histograms(best, n, lo, hi)[0].to_host()
    assert h0.tobytes() == h1.tobytes() and int(h0.sum()) == n * M, "the degenerate first-order scan is not the order-0 scan"

    c1 = ctx.empty((M, pk.MAX_MOTIF_LEN, 5), np.uint64)
    c2 = ctx.empty((M, pk.MAX_MOTIF_LEN, 17), np.uint64)
    ev = [ctx.timer() for _ in range(8)]
    times = []
    k1 = k2 = None
    for rep in range(a.reps + 1):
        ctx.record(ev[0])
        ctx.motif_scan(scan, S, widths, both, best=best)
        ctx.record(ev[1])
        ctx.motif_scan_dinuc(scan, S0, D, widths, both, best=best)
        ctx.record(ev[2])
        ctx.motif_best_sites(scan, S, widths, both, best=best, site=site)
        ctx.record(ev[3])
        ctx.synchronize()
        t = [ctx.elapsed_ms(ev[0], ev[1]), ctx.elapsed_ms(ev[1], ev[2]), ctx.elapsed_ms(ev[2], ev[3])]
        for thr in (strong, weak):
            pk._check(pk.lib().pengk_memset(ctx.h, c1.ptr, 0, c1.nbytes))
            pk._check(pk.lib().pengk_memset(ctx.h, c2.ptr, 0, c2.nbytes))
            ctx.record(ev[4])
            ctx.site_profiles(scan, best, site, widths, thr, a.flank, counts=c1)
            ctx.record(ev[5])
            ctx.site_pair_profiles(scan, best, site, widths, thr, a.flank, counts=c2)
            ctx.record(ev[6])
            k1, k2 = c1.to_host(), c2.to_host()
            t += [ctx.elapsed_ms(ev[4], ev[5]), ctx.elapsed_ms(ev[5], ev[6])]
            if thr is strong:
                F = [pk.clamp_flank(w, a.flank) for w in widths]
                assert all(int(k1[m, F[m]].sum()) == n for m in range(M))
            for m in range(M):  # every pair row holds the motif's sites
                W = widths[m] + 2 * pk.clamp_flank(widths[m], a.flank)
                assert np.all(k2[m, 1:W].sum(axis=1) == k1[m, 0].sum()), m
        if rep:
            times.append(t)
    t = np.median(np.array(times), axis=0)
    F = [pk.clamp_flank(w, a.flank) for w in widths]
    print(json.dumps({"probe": "motif_dinuc", "n_seq": n, "L": L, "motifs": M, "widths": widths, "p": a.p, "flank": a.flank,
                      "strands": 2 if both else 1, "sites_per_motif_weak": [int(k1[m, F[m]].sum()) for m in range(M)],
                      "scan_order0_ms": round(t[0], 3), "scan_dinuc_ms": round(t[1], 3),
                      "scan_dinuc_over_order0": round(float(t[1] / t[0]), 4), "best_site_scan_ms": round(t[2], 3),
                      "profiles_strong_ms": round(t[3], 3), "pair_profiles_strong_ms": round(t[4], 3),
                      "profiles_weak_ms": round(t[5], 3), "pair_profiles_weak_ms": round(t[6], 3),
                      "pair_over_single_strong": round(float(t[4] / t[3]), 4),
                      "pair_over_single_weak": round(float(t[6] / t[5]), 4), "reps": a.reps}))
    ctx.close()


if __name__ == "__main__":
    main()
