"""Times --positional-null composition in one process on the device-generated configs[2] input (pengk_synth_scan_sequences:
10M x 200 bp), width K, B bins of S from the center:
  pairs    pengk_position_pairs beside pengk_position_count with the same arguments and beside pengk_seq_strata (one
           bandwidth-bound pass over the same words: the floor), in alternating rounds -- pairs, count, strata, pairs, ... --
           between device events: the median of --rounds rounds after one warm-up round, --repeats times over, so that the
           spread of a kernel's own repeated medians stands beside the difference between two kernels
  inputs   both strands on the input as it is; the same with a 30-base poly-A in every tenth sequence (bases 50 .. 79: 25
           standing words on one counter); the plus strand alone; one sequence of 200 000 bases
  summary  pengk_position_summary_null with and without the pair table on a K = 7, B = 64 table of the first million
           sequences, on the host clock, once
Prints one JSON line.
  python tools/positional_null_probe.py [--n-seq 10000000] [--L 200] [--K 6] [--S 10] [--B 20] [--rounds 15] [--repeats 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import peng_motif_amd as pk  # noqa: E402


def alternating(ctx, fns, rounds, repeats):
    """{name: [median ms of `rounds` alternating rounds, `repeats` times]}; one warm-up round first"""
    a, b = ctx.timer(), ctx.timer()
    for fn in fns.values():
        fn()
    ctx.synchronize()
    out = {name: [] for name in fns}
    for _ in range(repeats):
        t = {name: [] for name in fns}
        for _ in range(rounds):
            for name, fn in fns.items():
                ctx.record(a)
                fn()
                ctx.record(b)
                ctx.synchronize()
                t[name].append(ctx.elapsed_ms(a, b))
        for name in fns:
            out[name].append(float(np.median(t[name])))
    return out


def figures(res, label, med):
    for name, m in med.items():
        res["%s_%s_ms" % (label, name)] = [round(x, 4) for x in m]
    count, pairs = med["count"], med["pairs"]
    res["%s_count_spread_ms" % label] = round(max(count) - min(count), 4)
    res["%s_pairs_minus_count_ms" % label] = round(float(np.median(pairs)) - float(np.median(count)), 4)
    res["%s_pairs_over_count" % label] = round(float(np.median(pairs)) / float(np.median(count)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-seq", type=int, default=10_000_000)
    ap.add_argument("--L", type=int, default=200)
    ap.add_argument("--K", type=int, default=6)
    ap.add_argument("--S", type=int, default=10)
    ap.add_argument("--B", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    n, L, K, S, B = a.n_seq, a.L, a.K, a.S, a.B
    ctx = pk.Context(0)
    scan = ctx.synth_scan(1, 0, n, L)
    res = {"probe": "positional_null", "n_seq": n, "L": L, "K": K, "S": S, "B": B, "rounds": a.rounds, "repeats": a.repeats}
    counts = ctx.to_device(np.zeros((B, 4 ** K), np.uint64))
    pairs = ctx.to_device(np.zeros((B, 16), np.uint64))
    stratum, hist = ctx.empty(max(n, 1), np.uint16), ctx.to_device(np.zeros(256, np.uint64))

    def kernels(s, both):
        return {"pairs": lambda: ctx.position_pairs(s, K, 2, S, B, both, pairs=pairs),
                "count": lambda: ctx.position_count(s, K, 2, S, B, both, counts=counts),
                "strata": lambda: ctx.seq_strata(s, stratum=stratum, hist=hist)}

    figures(res, "both", alternating(ctx, kernels(scan, True), a.rounds, a.repeats))
    calls = 1 + a.rounds * a.repeats
    res["pairs_counted"] = int(pairs.to_host().sum()) // calls
    figures(res, "plus", alternating(ctx, kernels(scan, False), a.rounds, a.repeats))

    # ---- a 30-base poly-A in every tenth sequence ----
    if L >= 96:
        wps = (L + 31) // 32
        w = scan[0].to_host().reshape(n, wps)
        w[::10, 1] &= np.uint64((1 << 36) - 1)                      # bases 50 .. 63
        w[::10, 2] &= ~np.uint64((1 << 32) - 1)                     # bases 64 .. 79
        tracts = (ctx.to_device(w.reshape(-1)), scan[1], scan[2], scan[3], n)
        del w
        figures(res, "tracts", alternating(ctx, kernels(tracts, True), a.rounds, a.repeats))
        res["tracts_pairs_over_uniform"] = round(float(np.median(res["tracts_pairs_ms"])) / float(np.median(res["both_pairs_ms"])), 4)
        del tracts

    # ---- one sequence of 200 000 bases ----
    one = np.random.default_rng(2).integers(1, 5, 200_000).astype(np.uint8)
    one[::1000] = 0
    lscan = ctx.upload_scan(pk.ScanLayout(one, np.array([0, len(one)], np.int64)))
    c64, p64 = ctx.to_device(np.zeros((64, 4 ** K), np.uint64)), ctx.to_device(np.zeros((64, 16), np.uint64))
    med = alternating(ctx, {"pairs": lambda: ctx.position_pairs(lscan, K, 2, 4096, 64, True, pairs=p64),
                            "count": lambda: ctx.position_count(lscan, K, 2, 4096, 64, True, counts=c64)}, a.rounds, a.repeats)
    figures(res, "one_200k_all_in_range", med)

    # ---- the summary's extra CPU work at K = 7, B = 64 ----
    m = min(n, 1_000_000)
    part = (scan[0], scan[1], scan[2], scan[3], m)
    t7 = ctx.position_count(part, 7, 2, 2, 64, True).to_host()
    p7 = ctx.position_pairs(part, 7, 2, 2, 64, True).to_host()
    ctx.close()
    for name, kw in (("flat", {}), ("composition", {"pairs": p7})):
        t0 = time.perf_counter()
        rep = pk.position_summary(t7, 7, True, 5, 0.01, capacity=1 << 16, **kw)
        res["summary_%s_ms" % name] = round((time.perf_counter() - t0) * 1e3, 3)
        res["summary_%s_words" % name] = len(rep)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
