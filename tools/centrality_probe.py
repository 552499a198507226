"""Times the central-enrichment test on the device (include/pengk.h, "central enrichment") for N motifs at p-value P
over the device-generated configs[2] input (pengk_synth_scan_sequences: 10M x 200 bp): the best-site scan, the
histograms, their download and the host summary, each between device events or host clocks (median of --reps after one
warm-up), plus the scoring scan (pengk_motif_scan) over the same input in the same process as the yardstick.  Prints one
JSON line.
  python tools/centrality_probe.py [--n-seq 10000000] [--L 200] [--motifs 16] [--p 1e-4] [--reps 5] [--plus]"""
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
    thr = []
    for s in S:
        lo, tail = pk.score_tail_pvalues(s, bg)
        thr.append(pk.score_threshold(tail, lo, a.p))
    both = not a.plus
    M = len(widths)
    best = ctx.empty((M, n), np.int32)
    site = ctx.empty((M, n), np.uint64)
    hd = ctx.empty((M, 2 * L + 1), np.uint64)
    hl = ctx.empty((M, L + 1), np.uint64)
    ev = [ctx.timer() for _ in range(6)]
    times = []
    for rep in range(a.reps + 1):
        ctx.record(ev[0])
        ctx.motif_scan(scan, S, widths, both, best=best)
        ctx.record(ev[1])
        ctx.motif_best_sites(scan, S, widths, both, best=best, site=site)
        ctx.record(ev[2])
        pk._check(pk.lib().pengk_memset(ctx.h, hd.ptr, 0, hd.nbytes))
        pk._check(pk.lib().pengk_memset(ctx.h, hl.ptr, 0, hl.nbytes))
        ctx.record(ev[3])
        ctx.centrality_histograms(best, site, scan[3], n, widths, thr, L, hd=hd, hl=hl)
        ctx.record(ev[4])
        hdh, hlh = hd.to_host(), hl.to_host()
        ctx.record(ev[5])
        ctx.synchronize()
        t0 = time.perf_counter()
        res = [pk.centrality_summary(hdh[m], hlh[m], L, widths[m], M) for m in range(M)]
        summary_ms = (time.perf_counter() - t0) * 1e3
        t = [ctx.elapsed_ms(ev[0], ev[1]), ctx.elapsed_ms(ev[1], ev[2]), ctx.elapsed_ms(ev[3], ev[4]), ctx.elapsed_ms(ev[4], ev[5]),
             summary_ms]
        if rep:
            times.append(t)
    t = np.median(np.array(times), axis=0)
    sites = [r["sites"] for r in res]
    assert all(int(hlh[m].sum()) == sites[m] for m in range(M))
    print(json.dumps({"probe": "motif_centrality", "n_seq": n, "L": L, "motifs": M, "widths": widths, "p": a.p,
                      "strands": 2 if both else 1, "sites_per_motif": sites,
                      "min_log10_evalue": round(min(r["log10_evalue"] for r in res), 3),
                      "scoring_scan_ms": round(t[0], 3), "best_site_scan_ms": round(t[1], 3), "histograms_ms": round(t[2], 3),
                      "download_ms": round(t[3], 3), "summary_host_ms": round(t[4], 3),
                      "total_ms": round(float(t[1] + t[2] + t[3] + t[4]), 3), "reps": a.reps}))
    ctx.close()


if __name__ == "__main__":
    main()
