"""Times --mask-low-complexity in one process on the device-generated configs[2] input (pengk_synth_scan_sequences:
10M x 200 bp) at threshold T:
  mask    pengk_mask_low_complexity over the input as it is, and over the same input with a 30-base poly-A in every tenth
          sequence (bases 50 .. 79)
  beside  pengk_motif_scan of N motifs of width 10-14 on both strands, and pengk_pack_scan_sizes + pengk_pack_scan of the
          masked set (W = 10)
  long    one sequence of 200 000 bases
  cli     (--cli) wall time of peng_motif on the same input as a FASTA file, with and without --mask-low-complexity
Device passes between device events, the median of --reps after one warm-up.  Prints one JSON line.
  python tools/dust_probe.py [--n-seq 10000000] [--L 200] [--T 20] [--motifs 16] [--reps 5] [--cli]"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import peng_motif_amd as pk  # noqa: E402
from erase_probe import median_ms, motifs  # noqa: E402

W = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-seq", type=int, default=10_000_000)
    ap.add_argument("--L", type=int, default=200)
    ap.add_argument("--T", type=int, default=20)
    ap.add_argument("--motifs", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cli", action="store_true")
    a = ap.parse_args()
    n, L = a.n_seq, a.L
    ctx = pk.Context(0)
    scan = ctx.synth_scan(1, 0, n, L)
    res = {"probe": "dust", "n_seq": n, "L": L, "T": a.T, "motifs": a.motifs, "reps": a.reps}

    # ---- the mask ----
    out_valid = ctx.empty(scan[0].shape, np.uint32)
    cnt = ctx.to_device(np.zeros(2, np.uint64))
    res["mask_ms"] = median_ms(ctx, lambda: ctx.mask_low_complexity(scan, a.T, out_valid=out_valid, masked=cnt), a.reps)
    c = cnt.to_host()  # (added to: reps + 1 times the same figures)
    res["bases_masked"], res["sequences_touched"] = int(c[0]) // (a.reps + 1), int(c[1]) // (a.reps + 1)
    res["mask_all_valid_ms"] = median_ms(ctx, lambda: ctx.mask_low_complexity(scan, a.T, all_valid=True, out_valid=out_valid,
                                                                             masked=cnt), a.reps)

    # ---- beside it: a 16-motif scan and the device packer ----
    S = motifs(a.motifs, np.random.default_rng(1))
    best = ctx.empty((a.motifs, n), np.int32)
    res["motif_scan_ms"] = median_ms(ctx, lambda: ctx.motif_scan(scan, S, [len(s) for s in S], True, best=best), a.reps)
    del best
    base, item = ctx.empty(n, np.uint64), ctx.empty(n, np.uint64)
    st = pk.PackedStruct()
    lib = pk.lib()

    def sizes():
        pk._check(lib.pengk_pack_scan_sizes(ctx.h, out_valid.ptr, scan[2].ptr, scan[3].ptr, n, W, 0, base.ptr, item.ptr, C.byref(st)))

    sizes()
    words, items = ctx.empty(st.n_words, np.uint64), ctx.empty(max(st.n_items, 1), np.uint64)
    res["pack_scan_sizes_ms"] = median_ms(ctx, sizes, a.reps)
    res["pack_scan_ms"] = median_ms(ctx, lambda: pk._check(lib.pengk_pack_scan(
        ctx.h, scan[0].ptr, out_valid.ptr, scan[2].ptr, scan[3].ptr, n, W, 0, base.ptr, item.ptr, words.ptr, st.n_words, items.ptr,
        st.n_items)), a.reps)
    res["mask_over_scan"] = res["mask_ms"] / res["motif_scan_ms"]
    del words, items, base, item

    # ---- a 30-base poly-A in every tenth sequence ----
    if L >= 96:
        wps = (L + 31) // 32
        w = scan[0].to_host().reshape(n, wps)
        w[::10, 1] &= np.uint64((1 << 36) - 1)                      # bases 50 .. 63
        w[::10, 2] &= ~np.uint64((1 << 32) - 1)                     # bases 64 .. 79
        tracts = (ctx.to_device(w.reshape(-1)), scan[1], scan[2], scan[3], n)
        del w
        cnt2 = ctx.to_device(np.zeros(2, np.uint64))
        res["mask_tracts_ms"] = median_ms(ctx, lambda: ctx.mask_low_complexity(tracts, a.T, out_valid=out_valid, masked=cnt2), a.reps)
        c = cnt2.to_host()
        res["tracts_bases_masked"], res["tracts_sequences_touched"] = int(c[0]) // (a.reps + 1), int(c[1]) // (a.reps + 1)
        del tracts

    # ---- one sequence of 200 000 bases: 1 563 tiles over the whole grid ----
    one = np.random.default_rng(2).integers(1, 5, 200_000).astype(np.uint8)
    one[::1000] = 0
    lscan = ctx.upload_scan(pk.ScanLayout(one, np.array([0, len(one)], np.int64)))
    res["one_200k_sequence_mask_ms"] = median_ms(ctx, lambda: ctx.mask_low_complexity(lscan, a.T), a.reps)
    ctx.close()

    # ---- the CLI, with and without the flag (a fresh process each: its own device context) ----
    if a.cli:
        cli, gen = os.path.join(ROOT, "peng-motif_amd", "host", "peng_motif"), os.path.join(ROOT, "tools", "synth_fasta")
        with tempfile.TemporaryDirectory() as d:
            fa = os.path.join(d, "s.fa")
            subprocess.run([gen, fa, str(n), str(L), "1", "0"], check=True)
            for key, extra in (("cli_s", []), ("cli_mask_s", ["--mask-low-complexity"])):
                t = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    r = subprocess.run([cli, fa, "-w", str(W), "-o", os.path.join(d, "o.meme")] + extra, check=True,
                                       stdout=subprocess.PIPE, timeout=600)
                    t.append(time.perf_counter() - t0)
                res[key] = float(np.median(t))
                if extra:
                    res["cli_mask_line"] = next(l for l in r.stdout.decode().splitlines() if l.startswith("low-complexity mask"))
            # where the flag's time goes: the phase report of one more run
            r = subprocess.run([cli, fa, "-w", str(W), "-o", os.path.join(d, "o.meme"), "--mask-low-complexity"], check=True,
                               stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=600, env=dict(os.environ, PENGK_TIMING="1"))
            res["cli_mask_timing"] = [l for l in r.stderr.decode().splitlines() if l.startswith("[timing]")]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
