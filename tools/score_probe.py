"""Times the motif scoring on the device (include/pengk.h, "motif scoring") for N motifs over the device-generated
configs[2] input (pengk_synth_scan_sequences: 10M x 200 bp) plus as many sampled negatives: sampling, the two scans and
the two histogram passes, each between device events (median of --reps after one warm-up).  Prints one JSON line.
--negatives shuffled: the negatives are the input's dinucleotide-preserving shuffles (pengk_shuffle_sequences, DESIGN.md
16) and are scanned with their own validity words; the first time is then the shuffle kernel's alone.
  python tools/score_probe.py [--n-seq 10000000] [--L 200] [--motifs 16] [--reps 5] [--plus] [--negatives sampled|shuffled]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import peng_motif_amd as pk  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-seq", type=int, default=10_000_000)
    ap.add_argument("--L", type=int, default=200)
    ap.add_argument("--motifs", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--plus", action="store_true")
    ap.add_argument("--negatives", choices=["sampled", "shuffled"], default="sampled")
    a = ap.parse_args()
    ctx = pk.Context(0)
    n, L = a.n_seq, a.L
    scan = ctx.synth_scan(1, 0, n, L)
    rng = np.random.default_rng(16)
    widths = [10 + (m % 5) for m in range(a.motifs)]  # 10..14
    S = [rng.integers(-400, 200, (w, 4)).astype(np.int32) for w in widths]
    lo = [int(s.min(axis=1).sum()) for s in S]
    hi = [int(s.max(axis=1).sum()) for s in S]
    V = [rng.dirichlet(np.ones(4) * 2, 4 ** k).astype(np.float64).reshape(-1, 4) for k in range(3)]
    th = np.array([min(int(np.floor(c * 2.0 ** 32)), 2 ** 32 - 1) for k in range(3) for row in V[k] for c in np.cumsum(row)[:3]],
                  np.uint32)
    neg = ctx.empty(scan[0].shape, np.uint64)
    shuffled = a.negatives == "shuffled"
    neg_valid = ctx.empty(scan[1].shape, np.uint32) if shuffled else None
    neg_scan = (neg, neg_valid, scan[2], scan[3], n)
    best = ctx.empty((len(widths), n), np.int32)
    both = not a.plus
    ev = [ctx.timer() for _ in range(6)]
    times = []
    for rep in range(a.reps + 1):
        hist = None
        ctx.record(ev[0])
        if shuffled:
            ctx.shuffle_sequences(scan, 1, 0, words=neg, valid=neg_valid)
        else:
            ctx.sample_background(scan, 1, 0, 2, th, words=neg)
        ctx.record(ev[1])
        ctx.motif_scan(scan, S, widths, both, best=best)
        ctx.record(ev[2])
        hist, _ = ctx.score_histograms(best, n, lo, hi)
        ctx.record(ev[3])
        if shuffled:
            ctx.motif_scan(neg_scan, S, widths, both, best=best)
        else:
            ctx.motif_scan(scan, S, widths, both, words=neg, all_valid=True, best=best)
        ctx.record(ev[4])
        ctx.score_histograms(best, n, lo, hi, hist=hist)
        ctx.record(ev[5])
        ctx.synchronize()
        t = [ctx.elapsed_ms(ev[i], ev[i + 1]) for i in range(5)]
        if rep:
            times.append(t)
        h = hist.to_host()
        assert int(h.sum()) == 2 * n * len(widths), "histogram totals"
    t = np.median(np.array(times), axis=0)
    windows = sum(2 * n * (L - w + 1) for w in widths)  # (both sets; per strand)
    total = float(t.sum())
    print(json.dumps({"probe": "motif_score", "n_seq": n, "L": L, "motifs": len(widths), "widths": widths,
                      "strands": 2 if both else 1, "negatives": a.negatives,
                      "shuffle_ms" if shuffled else "sample_ms": round(t[0], 3), "scan_pos_ms": round(t[1], 3),
                      "hist_pos_ms": round(t[2], 3), "scan_neg_ms": round(t[3], 3), "hist_neg_ms": round(t[4], 3),
                      "total_ms": round(total, 3), "window_scores_per_s": windows * (2 if both else 1) / (total * 1e-3),
                      "reps": a.reps}))
    ctx.close()


if __name__ == "__main__":
    main()
