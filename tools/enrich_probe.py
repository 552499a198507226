"""Times pengk_motif_enrich over a database of random motifs (widths 8..20, thresholds at p-value P) beside
pengk_motif_scan + pengk_score_histograms on 16 of them, in one process, on pengk_synth_scan_sequences input: at
configs[2] size (10M x 200 bp) and at 100 000 x 200 bp.  The three timed passes -- scan + histograms of the 16, the
enrichment of the same 16, the enrichment of the whole database -- alternate within every repetition, between device
events, after one warm-up round; minimum, median and maximum of --reps are printed, so that the scan's own run-to-run
spread stands beside the difference.  The 16 motifs' enrichment histograms are checked against d_best on the way.
Prints one JSON line per input.
  python tools/enrich_probe.py [--motifs 2000] [--p 1e-3] [--reps 5] [--plus] [--sizes 10000000,100000] [--L 200]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import peng_motif_amd as pk  # noqa: E402


def stats(v):
    v = np.asarray(v, np.float64)
    return {"min": round(float(v.min()), 3), "median": round(float(np.median(v)), 3), "max": round(float(v.max()), 3)}


def measure(ctx, scan, S, widths, both, thr, hi, lo, reps, n_small=16):
    n, nm = scan[4], len(widths)
    L = pk.lib()
    Sp, ln = pk._pad_motifs(S, widths)
    th, hi = np.ascontiguousarray(thr, np.int32), np.ascontiguousarray(hi, np.int32)
    nb = np.maximum(hi.astype(np.int64) - th + 1, 0)
    offs = np.concatenate([[0], np.cumsum(nb)]).astype(np.uint64)
    best = ctx.empty((n_small, n), np.int32)
    ev = [ctx.timer() for _ in range(4)]
    times = []

    def enrich(k, hist):
        pk._check(L.pengk_motif_enrich(ctx.h, scan[0].ptr, scan[1].ptr, scan[2].ptr, scan[3].ptr, n, k, Sp.ctypes.data,
                                       ln.ctypes.data, int(both), th.ctypes.data, hi.ctypes.data, offs.ctypes.data, hist.ptr,
                                       hist.ptr + 8 * int(offs[-1])))
    for rep in range(reps + 1):
        small = ctx.to_device(np.zeros(int(offs[-1]) + nm, np.uint64))  # the bins, then the scored counters
        whole = ctx.to_device(np.zeros(int(offs[-1]) + nm, np.uint64))
        ctx.record(ev[0])
        ctx.motif_scan(scan, S[:n_small], widths[:n_small], both, best=best)
        sh, _ = ctx.score_histograms(best, n, lo[:n_small], hi[:n_small])
        ctx.record(ev[1])
        enrich(n_small, small)
        ctx.record(ev[2])
        enrich(nm, whole)
        ctx.record(ev[3])
        ctx.synchronize()
        if rep:
            times.append([ctx.elapsed_ms(ev[k], ev[k + 1]) for k in range(3)])
    hs, hw, b = small.to_host(), whole.to_host(), best.to_host()
    for m in range(n_small):
        had = b[m] != pk.SCORE_SENTINEL
        want = np.bincount(b[m][had & (b[m] >= th[m])].astype(np.int64) - int(th[m]), minlength=int(nb[m]))
        a0, a1 = int(offs[m]), int(offs[m + 1])
        assert np.array_equal(hs[a0:a1], want.astype(np.uint64)) and np.array_equal(hw[a0:a1], hs[a0:a1]), "histograms of motif %d" % m
        assert int(hs[int(offs[-1]) + m]) == int(had.sum()) == int(hw[int(offs[-1]) + m])
    t = np.array(times)
    scan_ms, e16, eall = stats(t[:, 0]), stats(t[:, 1]), stats(t[:, 2])
    hits = hw[:int(offs[-1])]
    return {"scan_hist_16_ms": scan_ms, "enrich_16_ms": e16, "enrich_all_ms": eall,
            "scan_hist_ms_per_motif": round(scan_ms["median"] / n_small, 4),
            "enrich_16_ms_per_motif": round(e16["median"] / n_small, 4),
            "enrich_all_ms_per_motif": round(eall["median"] / nm, 4),
            "ratio_16": round(e16["median"] / scan_ms["median"], 4),
            "ratio_all_per_motif": round((eall["median"] / nm) / (scan_ms["median"] / n_small), 4),
            "scan_spread": round((scan_ms["max"] - scan_ms["min"]) / scan_ms["median"], 4),
            "bins": int(offs[-1]), "hits": int(hits.sum()), "groups_per_launch": ctx.info("enrich_groups_per_launch")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000000,100000")
    ap.add_argument("--L", type=int, default=200)
    ap.add_argument("--motifs", type=int, default=2000)
    ap.add_argument("--p", type=float, default=1e-3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--plus", action="store_true")
    a = ap.parse_args()
    ctx = pk.Context(0)
    rng = np.random.default_rng(19)
    widths = rng.integers(8, 21, a.motifs).tolist()
    S = [rng.integers(-400, 200, (w, 4)).astype(np.int32) for w in widths]
    bg = np.full(4, 0.25, np.float32)
    thr, hi, lo = [], [], []
    for s in S:
        l, tail = pk.score_tail_pvalues(s, bg)
        thr.append(pk.score_threshold(tail, l, a.p))
        hi.append(l + len(tail) - 1)
        lo.append(l)
    both = not a.plus
    for n in [int(x) for x in a.sizes.split(",")]:
        head = {"probe": "motif_enrich", "n_seq": n, "L": a.L, "motifs": a.motifs, "widths": "8..20", "p": a.p,
                "strands": 2 if both else 1, "reps": a.reps}
        scan = ctx.synth_scan(1, 0, n, a.L)
        print(json.dumps(dict(head, **measure(ctx, scan, S, widths, both, thr, hi, lo, a.reps))), flush=True)
        del scan
    ctx.close()


if __name__ == "__main__":
    main()
