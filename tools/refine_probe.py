"""Times one round of the motif refinement on the device (include/pengk.h, "motif refinement") for N motifs at p-value P
over the device-generated configs[2] input (pengk_synth_scan_sequences: 10M x 200 bp): the best-site scan (the yardstick,
in the same process), the site profiles, their download and the host's new matrices, each between device events or host
clocks (median of --reps after one warm-up).  The weak case takes random motifs at P (few sequences have a site); the
strong case keeps the same motifs and lowers every threshold until nearly every sequence has a site, so nearly every
wave adds to every column's bins.  Prints one JSON line.
  python tools/refine_probe.py [--n-seq 10000000] [--L 200] [--motifs 16] [--p 1e-4] [--flank 8] [--reps 5] [--plus]"""
import argparse
import json
import os
import sys
import time

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
    ap.add_argument("--flank", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--plus", action="store_true")
    a = ap.parse_args()
    ctx = pk.Context(0)
    n, L = a.n_seq, a.L
    scan = ctx.synth_scan(1, 0, n, L)
    rng = np.random.default_rng(16)
    widths = [10 + (m % 5) for m in range(a.motifs)]  # 10..14
    S = [rng.integers(-400, 200, (w, 4)).astype(np.int32) for w in widths]
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
    counts = ctx.empty((M, pk.MAX_MOTIF_LEN, 5), np.uint64)
    ev = [ctx.timer() for _ in range(7)]
    times = []
    for rep in range(a.reps + 1):
        ctx.record(ev[0])
        ctx.motif_best_sites(scan, S, widths, both, best=best, site=site)
        ctx.record(ev[1])
        pk._check(pk.lib().pengk_memset(ctx.h, counts.ptr, 0, counts.nbytes))
        ctx.record(ev[2])
        ctx.site_profiles(scan, best, site, widths, strong, a.flank, counts=counts)
        ctx.record(ev[3])
        ks = counts.to_host()
        pk._check(pk.lib().pengk_memset(ctx.h, counts.ptr, 0, counts.nbytes))
        ctx.record(ev[4])
        ctx.site_profiles(scan, best, site, widths, weak, a.flank, counts=counts)
        ctx.record(ev[5])
        kw = counts.to_host()
        ctx.record(ev[6])
        ctx.synchronize()
        t0 = time.perf_counter()
        res = [pk.profile_refine(kw[m], widths[m], a.flank, bg, 0.25) for m in range(M)]
        host_ms = (time.perf_counter() - t0) * 1e3
        t = [ctx.elapsed_ms(ev[0], ev[1]), ctx.elapsed_ms(ev[2], ev[3]), ctx.elapsed_ms(ev[4], ev[5]), ctx.elapsed_ms(ev[5], ev[6]),
             host_ms]
        if rep:
            times.append(t)
    t = np.median(np.array(times), axis=0)
    F = [pk.clamp_flank(w, a.flank) for w in widths]
    sites_weak = [int(kw[m, F[m]].sum()) for m in range(M)]
    sites_strong = [int(ks[m, F[m]].sum()) for m in range(M)]
    assert sites_weak == [r["sites"] for r in res] and all(s == n for s in sites_strong)
    print(json.dumps({"probe": "motif_refine", "n_seq": n, "L": L, "motifs": M, "widths": widths, "p": a.p, "flank": a.flank,
                      "strands": 2 if both else 1, "sites_per_motif_weak": sites_weak, "sites_per_motif_strong": sites_strong[0],
                      "best_site_scan_ms": round(t[0], 3), "profiles_strong_ms": round(t[1], 3), "profiles_weak_ms": round(t[2], 3),
                      "download_ms": round(t[3], 3), "new_matrices_host_ms": round(t[4], 3),
                      "round_ms_weak": round(float(t[0] + t[2] + t[3] + t[4]), 3),
                      "profiles_over_best_site_scan_weak": round(float(t[2] / t[0]), 4),
                      "profiles_over_best_site_scan_strong": round(float(t[1] / t[0]), 4), "reps": a.reps}))
    ctx.close()


if __name__ == "__main__":
    main()
