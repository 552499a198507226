"""Times the control matching (--score-negatives control) in one process on the device-generated configs[2] input
(pengk_synth_scan_sequences: 10M x 200 bp) as input (seed 1) and as control (seed 2):
  strata   pengk_seq_strata of the control beside pengk_pack_scan_sizes on the same layout (the existing
           one-thread-per-sequence walk over the validity words; W = 10), both with and without validity words
  select   pengk_select_strata of the control at the quotas of --control-ratio 1 and at a third of every stratum
  paths    the three ways to build the negatives of --score-motifs side by side: sampled (pengk_sample_background, order 2),
           shuffled (pengk_shuffle_sequences), control (two stratum passes, the quotas, the selection)
Device passes between device events, the median of --reps after one warm-up.  Prints one JSON line.
  python tools/match_probe.py [--n-seq 10000000] [--L 200] [--gc-bins 10] [--reps 5]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import peng_motif_amd as pk  # noqa: E402


def median_ms(ctx, fn, reps):
    a, b = ctx.timer(), ctx.timer()
    t = []
    for rep in range(reps + 1):
        ctx.record(a)
        fn()
        ctx.record(b)
        ctx.synchronize()
        if rep:
            t.append(ctx.elapsed_ms(a, b))
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-seq", type=int, default=10_000_000)
    ap.add_argument("--L", type=int, default=200)
    ap.add_argument("--gc-bins", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    n, L, G = a.n_seq, a.L, a.gc_bins
    ctx = pk.Context(0)
    lib = pk.lib()
    inp, ctl = ctx.synth_scan(1, 0, n, L), ctx.synth_scan(2, 0, n, L)
    wps = (L + 31) // 32
    res = {"probe": "match", "n_seq": n, "L": L, "gc_bins": G, "reps": a.reps,
           "stratum_pass_bytes": n * (wps * 12 + 8 + 4 + 2), "measure_pass_bytes": n * (wps * 4 + 8 + 4 + 16)}

    # ---- the stratum pass beside the packer's measure pass ----
    base, item = ctx.empty(n, np.uint64), ctx.empty(n, np.uint64)
    st = pk.PackedStruct()
    stratum, hist = ctx.empty(n, np.uint16), ctx.to_device(np.zeros(256, np.uint64))
    for key, valid in (("", ctl[1].ptr), ("_all_valid", None)):
        res["pack_scan_sizes%s_ms" % key] = median_ms(ctx, lambda: pk._check(lib.pengk_pack_scan_sizes(
            ctx.h, valid, ctl[2].ptr, ctl[3].ptr, n, 10, 0, base.ptr, item.ptr, C.byref(st))), a.reps)
        res["seq_strata%s_ms" % key] = median_ms(ctx, lambda: ctx.seq_strata(ctl, G, True, all_valid=valid is None, stratum=stratum,
                                                                            hist=hist), a.reps)
    res["strata_over_measure"] = res["seq_strata_ms"] / res["pack_scan_sizes_ms"]
    res["seq_strata_GBps"] = res["stratum_pass_bytes"] / res["seq_strata_ms"] / 1e6
    del base, item

    # ---- the selection ----
    s_in, h_in = ctx.seq_strata(inp, G, True)
    s_ctl, h_ctl = ctx.seq_strata(ctl, G, True)
    h_in, h_ctl = h_in.to_host(), h_ctl.to_host()
    zero = np.zeros(256, np.uint64)
    quota, short = pk.match_quotas(h_in, h_ctl, 1)
    res["strata_in_use"] = int((h_in > 0).sum())
    res["kept"], res["shortfall"] = int(quota.sum()), short
    kept = []
    res["select_strata_ms"] = median_ms(ctx, lambda: kept.append(ctx.select_strata(s_ctl, n, h_ctl, quota, zero, ctl[2], ctl[3])[3]),
                                        a.reps)
    assert set(kept) == {res["kept"]}
    res["select_strata_third_ms"] = median_ms(ctx, lambda: ctx.select_strata(s_ctl, n, h_ctl, h_ctl // 3, zero, ctl[2], ctl[3]), a.reps)

    # ---- the three ways to the negatives ----
    thresholds = np.tile(np.array([1 << 30, 1 << 31, 3 << 30], np.uint32), 21)  # uniform contexts of orders 0..2
    words, valid = ctx.empty(inp[0].shape, np.uint64), ctx.empty(inp[1].shape, np.uint32)
    res["negatives_sampled_ms"] = median_ms(ctx, lambda: ctx.sample_background(inp, 1, 0, 2, thresholds, words=words), a.reps)
    res["negatives_shuffled_ms"] = median_ms(ctx, lambda: ctx.shuffle_sequences(inp, 1, 0, words=words, valid=valid), a.reps)

    def control():
        hh = ctx.to_device(np.zeros(512, np.uint64))
        ctx.seq_strata(inp, G, True, stratum=s_in, hist=hh.ptr)
        ctx.seq_strata(ctl, G, True, stratum=s_ctl, hist=hh.ptr + 256 * 8)
        h = hh.to_host()
        q, _ = pk.match_quotas(h[:256], h[256:], 1)
        ctx.select_strata(s_ctl, n, h[256:], q, zero, ctl[2], ctl[3])

    res["negatives_control_ms"] = median_ms(ctx, control, a.reps)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
