"""Times the motif pair histograms on the device (include/pengk.h, "motif pair spacing") for N motifs at p-value P over
the device-generated configs[2] input (pengk_synth_scan_sequences: 10M x 200 bp): the best-site scan and the pair
histograms between device events (median of --reps after one warm-up), their download and the host summary of every
pair by host clocks.  Twice: with random motifs, whose pairs spread over every bin, and "planted" -- the best sites of
motifs 0 and 1 overwritten so that in --planted-share of the sequences motif 1 starts 7 bases after motif 0 ends, both on
+: nearly every co-occurring sequence of that pair in one gap bin, the contended case.  Prints one JSON line per case.
  python tools/spacing_probe.py [--n-seq 10000000] [--L 200] [--motifs 16] [--p 1e-4] [--max-gap 150] [--reps 5] [--plus]"""
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
    ap.add_argument("--max-gap", type=int, default=150)
    ap.add_argument("--planted-share", type=float, default=0.9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--plus", action="store_true")
    a = ap.parse_args()
    ctx = pk.Context(0)
    n, L, G, M = a.n_seq, a.L, a.max_gap, a.motifs
    scan = ctx.synth_scan(1, 0, n, L)
    rng = np.random.default_rng(16)
    widths = [10 + (m % 5) for m in range(M)]  # 10..14
    S = [rng.integers(-400, 200, (w, 4)).astype(np.int32) for w in widths]
    bg = np.full(4, 0.25, np.float32)
    thr = []
    for s in S:
        lo, tail = pk.score_tail_pvalues(s, bg)
        thr.append(pk.score_threshold(tail, lo, a.p))
    both = not a.plus
    pairs = M * (M - 1) // 2
    B = 4 * (G + 1) + 2
    best = ctx.empty((M, n), np.int32)
    site = ctx.empty((M, n), np.uint64)
    hg, hl, hm = ctx.empty((pairs, B), np.uint64), ctx.empty((pairs, L + 1), np.uint64), ctx.empty(M, np.uint64)
    ev = [ctx.timer() for _ in range(5)]
    for case in ("random", "planted"):
        times = []
        for rep in range(a.reps + 1):
            ctx.record(ev[0])
            if case == "random" or rep == 0:
                ctx.motif_best_sites(scan, S, widths, both, best=best, site=site)
            ctx.record(ev[1])
            if case == "planted" and rep == 0:
                # motifs 0 and 1: a site in the chosen sequences, motif 1 seven bases after motif 0's end
                on = rng.random(n) < a.planted_share
                p0 = rng.integers(0, L - widths[0] - widths[1] - 7 + 1, n).astype(np.uint64)
                for m, p in ((0, p0), (1, p0 + np.uint64(widths[0] + 7))):
                    b = np.where(on, np.int32(thr[m]), np.int32(pk.SCORE_SENTINEL)).astype(np.int32)
                    c = np.where(on, np.uint64(2) * p, np.uint64(0)).astype(np.uint64)
                    pk._check(pk.lib().pengk_memcpy_h2d(ctx.h, best.ptr + 4 * m * n, b.ctypes.data, b.nbytes))
                    pk._check(pk.lib().pengk_memcpy_h2d(ctx.h, site.ptr + 8 * m * n, c.ctypes.data, c.nbytes))
            for h in (hg, hl, hm):
                pk._check(pk.lib().pengk_memset(ctx.h, h.ptr, 0, h.nbytes))
            ctx.record(ev[2])
            ctx.spacing_histograms(best, site, scan[3], n, widths, thr, G, max(widths), L, hg, hl, hm)
            ctx.record(ev[3])
            hgh, hlh, hmh = hg.to_host(), hl.to_host(), hm.to_host()
            ctx.record(ev[4])
            ctx.synchronize()
            t0 = time.perf_counter()
            res = {}
            for b in range(1, M):
                for q0 in range(b):
                    q = b * (b - 1) // 2 + q0
                    res[(q0, b)] = pk.spacing_summary(hgh[q], hlh[q], G, L, widths[q0], widths[b], 4 if both else 2, n, hmh[q0],
                                                      hmh[b], pairs)
            summary_ms = (time.perf_counter() - t0) * 1e3
            if rep:
                times.append([ctx.elapsed_ms(ev[0], ev[1]), ctx.elapsed_ms(ev[2], ev[3]), ctx.elapsed_ms(ev[3], ev[4]), summary_ms])
        t = np.median(np.array(times), axis=0)
        top = min(res, key=lambda k: res[k]["log10_evalue"])
        r = res[top]
        out = {"probe": "motif_spacing", "case": case, "n_seq": n, "L": L, "motifs": M, "pairs": pairs, "max_gap": G, "p": a.p,
               "strands": 2 if both else 1, "sites_per_motif": [int(x) for x in hmh],
               "pair_sequences_total": int(hgh.sum()), "top_pair": [top[0] + 1, top[1] + 1],
               "top_orientation": pk.SPACING_CLASSES[r["orientation"]], "top_gap": r["gap"], "top_count": r["count"],
               "top_log10_evalue": round(r["log10_evalue"], 3), "histograms_ms": round(float(t[1]), 3),
               "download_ms": round(float(t[2]), 3), "summary_host_ms": round(float(t[3]), 3), "reps": a.reps}
        if case == "random":
            out["best_site_scan_ms"] = round(float(t[0]), 3)
        print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
