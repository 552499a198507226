"""Times the count pass of --sites-qvalue (pengk_sites_histograms with d_counts) against the plain count pass
(pengk_sites_count) in one process, for N motifs at p-value P: on the device-generated configs[2] input
(pengk_synth_scan_sequences: 10M x 200 bp, sites rare) and on an input of the same size in which every sequence carries
the consensus of motif 0 (100 000 host-made sequences, tiled), so that one motif sends a site per sequence to its top
bins.  Each pass between device events, median of --reps after one warm-up.  Prints one JSON line per input.
  python tools/qvalue_probe.py [--n-seq 10000000] [--L 200] [--motifs 16] [--p 1e-4] [--reps 5] [--plus]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import peng_motif_amd as pk  # noqa: E402


def planted_scan(ctx, n, L, cons, distinct=100_000):
    """n sequences of L bases, each with `cons` at a random position: `distinct` of them made here, tiled up to n"""
    rng = np.random.default_rng(3)
    d = min(distinct, n)
    codes = rng.integers(1, 5, (d, L), dtype=np.uint8)
    pos = rng.integers(0, L - len(cons) + 1, d)
    codes[np.arange(d)[:, None], pos[:, None] + np.arange(len(cons))[None, :]] = cons[None, :]
    lay = pk.ScanLayout(codes.reshape(-1), np.arange(d + 1, dtype=np.int64) * L)
    wps = (L + 31) // 32
    reps = (n + d - 1) // d
    words = np.tile(lay.words[:d * wps], reps)[:n * wps]
    valid = np.tile(lay.valid[:d * wps], reps)[:n * wps]
    offs = np.arange(n, dtype=np.int64) * (wps * 32)
    lens = np.full(n, L, np.uint32)
    return ctx.to_device(words), ctx.to_device(valid), ctx.to_device(offs), ctx.to_device(lens), n


def measure(ctx, scan, S, widths, both, thr, hi, reps):
    n, nm = scan[4], len(widths)
    Sp, ln = pk._pad_motifs(S, widths)
    th, hi = np.ascontiguousarray(thr, np.int32), np.ascontiguousarray(hi, np.int32)
    nb = np.maximum(hi.astype(np.int64) - th + 1, 0)
    offs = np.concatenate([[0], np.cumsum(nb)]).astype(np.uint64)
    counts = ctx.empty((nm, n), np.uint64)
    counts2 = ctx.empty((nm, n), np.uint64)
    ev = [ctx.timer() for _ in range(3)]
    L = pk.lib()
    times = []
    for rep in range(reps + 1):
        hist = ctx.to_device(np.zeros(int(offs[-1]) + nm, np.uint64))  # the bins, then the tests
        ctx.record(ev[0])
        ctx.sites_count(scan, S, widths, both, thr, counts=counts)
        ctx.record(ev[1])
        pk._check(L.pengk_sites_histograms(ctx.h, scan[0].ptr, scan[1].ptr, scan[2].ptr, scan[3].ptr, n, nm, Sp.ctypes.data,
                                           ln.ctypes.data, int(both), th.ctypes.data, hi.ctypes.data, offs.ctypes.data,
                                           hist.ptr, hist.ptr + 8 * int(offs[-1]), counts2.ptr))
        ctx.record(ev[2])
        ctx.synchronize()
        if rep:
            times.append([ctx.elapsed_ms(ev[0], ev[1]), ctx.elapsed_ms(ev[1], ev[2])])
    h = hist.to_host()
    _, _, tot = ctx.sites_slices(counts, n, nm)
    _, _, tot2 = ctx.sites_slices(counts2, n, nm)
    per_motif = [int(h[int(offs[m]):int(offs[m + 1])].sum()) for m in range(nm)]
    assert per_motif == [int(x) for x in tot] == [int(x) for x in tot2], "histogram and count totals"
    t = np.median(np.array(times), axis=0)
    top = [int(h[int(offs[m + 1]) - 1]) if nb[m] else 0 for m in range(nm)]
    return {"count_ms": round(float(t[0]), 3), "hist_count_ms": round(float(t[1]), 3), "ratio": round(float(t[1] / t[0]), 4),
            "sites": int(sum(per_motif)), "sites_per_motif": per_motif, "top_bin": top,
            "tests_per_motif": [int(x) for x in h[int(offs[-1]):]], "bins": [int(x) for x in nb]}


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
    rng = np.random.default_rng(16)
    widths = [10 + (m % 5) for m in range(a.motifs)]  # 10..14
    S = [rng.integers(-400, 200, (w, 4)).astype(np.int32) for w in widths]
    bg = np.full(4, 0.25, np.float32)
    thr, hi = [], []
    for s in S:
        lo, tail = pk.score_tail_pvalues(s, bg)
        thr.append(pk.score_threshold(tail, lo, a.p))
        hi.append(lo + len(tail) - 1)
    both = not a.plus
    head = {"probe": "sites_qvalue", "n_seq": n, "L": L, "motifs": len(widths), "widths": widths, "p": a.p,
            "strands": 2 if both else 1, "reps": a.reps}
    scan = ctx.synth_scan(1, 0, n, L)
    print(json.dumps(dict(head, input="configs[2], device-generated", **measure(ctx, scan, S, widths, both, thr, hi, a.reps))),
          flush=True)
    del scan
    cons = (np.argmax(S[0], axis=1) + 1).astype(np.uint8)
    scan = planted_scan(ctx, n, L, cons)
    print(json.dumps(dict(head, input="every sequence carries the consensus of motif 0",
                          **measure(ctx, scan, S, widths, both, thr, hi, a.reps))), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
