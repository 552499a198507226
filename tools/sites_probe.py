"""Times the motif sites on the device (include/pengk.h, "motif sites") for N motifs at p-value P over the
device-generated configs[2] input (pengk_synth_scan_sequences: 10M x 200 bp): the count pass, the slicing (block totals
and their download), the offsets scans with the emit pass, and the records' download, each between device events (median
of --reps after one warm-up).  Prints one JSON line.
  python tools/sites_probe.py [--n-seq 10000000] [--L 200] [--motifs 16] [--p 1e-4] [--reps 5] [--plus]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import peng_motif_amd as pk  # noqa: E402
import motif_sites_model as mst  # noqa: E402


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
    counts = ctx.empty((len(widths), n), np.uint64)
    ev = [ctx.timer() for _ in range(5)]
    times, wall = [], []
    for rep in range(a.reps + 1):
        t0 = time.perf_counter()
        ctx.record(ev[0])
        ctx.sites_count(scan, S, widths, both, thr, counts=counts)
        ctx.record(ev[1])
        bounds, recs, tot = ctx.sites_slices(counts, n, len(widths))
        ctx.record(ev[2])
        ctx.synchronize()
        slices_ms = ctx.elapsed_ms(ev[1], ev[2])
        cap = max(int(recs.max()), 1)
        if rep == 0:
            buf = ctx.empty(cap * pk.SITE.itemsize, np.uint8)
            host = np.empty(cap * pk.SITE.itemsize, np.uint8)
        emit_ms = dl_ms = 0.0
        for k in range(len(recs)):
            ctx.record(ev[2])
            ctx.sites_emit(scan, S, widths, both, thr, counts, int(bounds[k]), int(bounds[k + 1]), buf, cap)
            ctx.record(ev[3])
            pk._check(pk.lib().pengk_memcpy_d2h(ctx.h, host.ctypes.data, buf.ptr, int(recs[k]) * pk.SITE.itemsize))
            ctx.record(ev[4])
            ctx.synchronize()
            emit_ms += ctx.elapsed_ms(ev[2], ev[3])
            dl_ms += ctx.elapsed_ms(ev[3], ev[4])
        ctx.synchronize()
        wall.append(time.perf_counter() - t0)
        t = [ctx.elapsed_ms(ev[0], ev[1]), slices_ms, emit_ms, dl_ms]
        if rep:
            times.append(t)
        assert int(recs.sum()) == int(tot.sum()), "count totals"
    t = np.median(np.array(times), axis=0)
    print(json.dumps({"probe": "motif_sites", "n_seq": n, "L": L, "motifs": len(widths), "widths": widths, "p": a.p,
                      "strands": 2 if both else 1, "sites": int(tot.sum()), "sites_per_motif": [int(x) for x in tot],
                      "slices": len(recs), "count_ms": round(t[0], 3), "slices_ms": round(t[1], 3),
                      "scan_emit_ms": round(t[2], 3), "download_ms": round(t[3], 3), "total_ms": round(float(t.sum()), 3),
                      "wall_ms": round(float(np.median(wall[1:])) * 1e3, 3), "reps": a.reps}))
    ctx.close()


if __name__ == "__main__":
    main()
