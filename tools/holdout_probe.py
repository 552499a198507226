"""Times the pieces of --holdout in one process on the device-generated configs[2] input (pengk_synth_scan_sequences:
10M x 200 bp; W = 10, both strands), for N motifs of width 10-14 at p-value P and a hold-out fraction F:
  split   pengk_split_sequences beside pengk_select_strata on the same layout (quotas that keep every second sequence)
  enrich  the four pengk_motif_enrich calls of the report (training and hold-out share, input and shuffled negatives)
          beside the two calls over the whole input and the whole negatives: the same bases
  pack    pengk_pack_scan_sizes + pengk_pack_scan of the training share beside the same two over the whole input
  cli     (--cli) wall time of peng_motif on the same input as a FASTA file, with and without --holdout
Device passes between device events, the median of --reps after one warm-up (the split and the selection synchronise
with the host inside the call: their figures hold that wait, as a caller meets it).  Prints one JSON line and writes it to
--out (default profiles/holdout_probe.log).
  python tools/holdout_probe.py [--n-seq 10000000] [--L 200] [--motifs 16] [--p 1e-3] [--fraction 0.1] [--reps 5] [--cli]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import peng_motif_amd as pk  # noqa: E402
import motif_sites_model as mst  # noqa: E402
from erase_probe import median_ms, motifs  # noqa: E402

W = 10
BG = np.full(4, 0.25, np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-seq", type=int, default=10_000_000)
    ap.add_argument("--L", type=int, default=200)
    ap.add_argument("--motifs", type=int, default=16)
    ap.add_argument("--p", type=float, default=1e-3)
    ap.add_argument("--fraction", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cli", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "holdout_probe.log"))
    a = ap.parse_args()
    n, L = a.n_seq, a.L
    lib = pk.lib()
    ctx = pk.Context(0)
    scan = ctx.synth_scan(1, 0, n, L)
    S = motifs(a.motifs, np.random.default_rng(1))
    lens = [len(s) for s in S]
    hi = [int(np.asarray(s, np.int64).max(axis=1).sum()) for s in S]
    thr = [mst.threshold(*mst.tail_pvalues(s, BG), a.p) for s in S]
    threshold = int(a.fraction * 4294967296.0)
    res = {"probe": "holdout", "n_seq": n, "L": L, "W": W, "motifs": a.motifs, "p": a.p, "fraction": a.fraction, "reps": a.reps}

    # ---- the split beside the selection of --score-negatives control ----
    out = [(ctx.empty(n, np.int64), ctx.empty(n, np.uint32), ctx.empty(n, np.uint32)) for _ in range(2)]
    n0, n1 = C.c_uint64(), C.c_uint64()

    def split():
        pk._check(lib.pengk_split_sequences(ctx.h, 1, 0, n, threshold, None, scan[2].ptr, scan[3].ptr, None, out[0][0].ptr,
                                            out[0][1].ptr, out[0][2].ptr, C.byref(n0), out[1][0].ptr, out[1][1].ptr, out[1][2].ptr,
                                            C.byref(n1)))

    res["split_ms"] = median_ms(ctx, split, a.reps)
    res["n_train"], res["n_hold"] = int(n0.value), int(n1.value)
    stratum, hist = ctx.seq_strata(scan, 10, True)
    count = hist.to_host().astype(np.uint64)
    quota, rank0 = count // np.uint64(2), np.zeros(256, np.uint64)
    sel = (ctx.empty(n, np.int64), ctx.empty(n, np.uint32), ctx.empty(n, np.uint32))
    n_sel = C.c_uint64()

    def select():
        pk._check(lib.pengk_select_strata(ctx.h, stratum.ptr, n, count.ctypes.data, quota.ctypes.data, rank0.ctypes.data, scan[2].ptr,
                                          scan[3].ptr, sel[0].ptr, sel[1].ptr, sel[2].ptr, C.byref(n_sel)))

    res["select_strata_ms"] = median_ms(ctx, select, a.reps)
    res["n_selected"] = int(n_sel.value)
    res["split_over_select"] = res["split_ms"] / res["select_strata_ms"]
    del sel, stratum

    # ---- the four scans of the report beside the two over the whole sets ----
    nwords, nvalid = ctx.shuffle_sequences(scan, 1, 0)
    nb = np.maximum(np.asarray(hi, np.int64) - np.asarray(thr, np.int64) + 1, 0)
    d_hist = ctx.to_device(np.zeros(4 * max(int(nb.sum()), 1), np.uint64))
    d_scored = ctx.to_device(np.zeros(4 * a.motifs, np.uint64))
    train = (scan[0], scan[1], out[0][0], out[0][1], int(n0.value))
    hold = (scan[0], scan[1], out[1][0], out[1][1], int(n1.value))

    def enrich(sets):
        for layout, negative in sets:
            ctx.motif_enrich(layout, S, lens, True, thr, hi, words=nwords if negative else None, valid=nvalid if negative else None,
                             hist=d_hist, scored=d_scored)

    res["enrich_whole_2_calls_ms"] = median_ms(ctx, lambda: enrich([(scan, False), (scan, True)]), a.reps)
    res["enrich_shares_4_calls_ms"] = median_ms(ctx, lambda: enrich([(train, False), (train, True), (hold, False), (hold, True)]),
                                                a.reps)
    res["enrich_shares_over_whole"] = res["enrich_shares_4_calls_ms"] / res["enrich_whole_2_calls_ms"]
    del nwords, nvalid

    # ---- the training share in the count layout beside the whole input ----
    base, item = ctx.empty(n, np.uint64), ctx.empty(n, np.uint64)
    st = pk.PackedStruct()

    def sizes(layout):
        pk._check(lib.pengk_pack_scan_sizes(ctx.h, scan[1].ptr, layout[2].ptr, layout[3].ptr, layout[4], W, 0, base.ptr, item.ptr,
                                            C.byref(st)))

    for key, layout in (("whole", scan), ("train", train)):
        sizes(layout)
        words, items = ctx.empty(st.n_words, np.uint64), ctx.empty(max(st.n_items, 1), np.uint64)

        def write():
            pk._check(lib.pengk_pack_scan(ctx.h, scan[0].ptr, scan[1].ptr, layout[2].ptr, layout[3].ptr, layout[4], W, 0, base.ptr,
                                          item.ptr, words.ptr, st.n_words, items.ptr, st.n_items))

        res["pack_scan_sizes_%s_ms" % key] = median_ms(ctx, lambda: sizes(layout), a.reps)
        res["pack_scan_%s_ms" % key] = median_ms(ctx, write, a.reps)
        res["packed_%s" % key] = {"n_words": st.n_words, "n_items": st.n_items, "n_windows": st.n_windows}
        del words, items
    ctx.close()

    # ---- the CLI, with and without the flag (a fresh process each: its own device context) ----
    if a.cli:
        cli, gen = os.path.join(ROOT, "peng-motif_amd", "host", "peng_motif"), os.path.join(ROOT, "tools", "synth_fasta")
        with tempfile.TemporaryDirectory() as d:
            fa = os.path.join(d, "s.fa")
            subprocess.run([gen, fa, str(n), str(L), "1", "0"], check=True)
            for key, extra in (("cli_s", []), ("cli_holdout_s", ["--holdout", os.path.join(d, "holdout.tsv")])):
                t = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    subprocess.run([cli, fa, "-w", str(W), "-o", os.path.join(d, "o.meme")] + extra, check=True,
                                   stdout=subprocess.DEVNULL, timeout=600)
                    t.append(time.perf_counter() - t0)
                res[key] = float(np.median(t))
            r = subprocess.run([cli, fa, "-w", str(W), "-o", os.path.join(d, "o.meme"), "--holdout", os.path.join(d, "holdout.tsv")],
                               check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=600, env=dict(os.environ, PENGK_TIMING="1"))
            res["cli_holdout_timing"] = [l for l in r.stderr.decode().splitlines() if "holdout" in l or "total" in l]
            with open(os.path.join(d, "holdout.tsv")) as f:
                res["cli_holdout_report"] = f.read().splitlines()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
