"""Times the pieces of an --erase round in one process on the device-generated configs[2] input (pengk_synth_scan_sequences:
10M x 200 bp; W = 10, both strands), for N motifs of width 10-14 at p-value P (motif 0 holds the planted GCTGAGTCAT):
  mask   pengk_mask_sites beside pengk_sites_count with the same arguments (the same walk plus an atomic per touched word)
  pack   pengk_pack_scan_sizes + pengk_pack_scan of the masked set beside the host's pengk_pack_threads of the same
         sequences as byte codes (what a round would cost without the device packer, before the download and upload)
  count  pengk_count of the masked, device-packed set beside pengk_count of the input
  cli    (--cli) wall time of peng_motif on the same input as a FASTA file, with and without --erase
Device passes between device events, the median of --reps after one warm-up.  Prints one JSON line.
  python tools/erase_probe.py [--n-seq 10000000] [--L 200] [--motifs 16] [--p 1e-4] [--reps 5] [--host-threads 16] [--cli]"""
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

W = 10
BG = np.full(4, 0.25, np.float32)


def motifs(n, rng):
    """n log-odds matrices of width 10..14: sharp columns (0.85 on a letter); motif 0's first ten are GCTGAGTCAT"""
    out = []
    for m in range(n):
        w = 10 + m % 5
        letters = rng.integers(0, 4, w)
        if m == 0:
            letters[:10] = ["ACGT".index(x) for x in "GCTGAGTCAT"]
        p = np.full((w, 4), 0.05)
        p[np.arange(w), letters] = 0.85
        out.append(np.clip(np.round(100 * np.log2(p / 0.25)), -2000, 2000).astype(np.int32))
    return out


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


def host_codes(scan, n, L):
    """the byte codes of the synthetic sequences (every base valid), from the scan words, a million sequences at a time"""
    wps = (L + 31) // 32
    words = scan[0].to_host().reshape(n, wps)
    codes = np.empty((n, L), np.uint8)
    sh = (2 * np.arange(32, dtype=np.uint64))[None, None, :]
    for a in range(0, n, 1 << 20):
        w = words[a:a + (1 << 20)]
        codes[a:a + len(w)] = (((w[:, :, None] >> sh) & np.uint64(3)).astype(np.uint8) + 1).reshape(len(w), wps * 32)[:, :L]
    return codes.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-seq", type=int, default=10_000_000)
    ap.add_argument("--L", type=int, default=200)
    ap.add_argument("--motifs", type=int, default=16)
    ap.add_argument("--p", type=float, default=1e-4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--cli", action="store_true")
    a = ap.parse_args()
    n, L = a.n_seq, a.L
    ctx = pk.Context(0)
    scan = ctx.synth_scan(1, 0, n, L)
    S = motifs(a.motifs, np.random.default_rng(1))
    lens = [len(s) for s in S]
    thr = [mst.threshold(*mst.tail_pvalues(s, BG), a.p) for s in S]
    res = {"probe": "erase", "n_seq": n, "L": L, "W": W, "motifs": a.motifs, "p": a.p, "reps": a.reps}

    # ---- mask beside the count pass of --sites ----
    counts = ctx.empty((a.motifs, n), np.uint64)
    out_valid = ctx.empty(scan[0].shape, np.uint32)
    sites, erased = ctx.to_device(np.zeros(a.motifs, np.uint64)), ctx.to_device(np.zeros(1, np.uint64))
    res["sites_count_ms"] = median_ms(ctx, lambda: ctx.sites_count(scan, S, lens, True, thr, counts=counts), a.reps)
    res["mask_sites_ms"] = median_ms(ctx, lambda: ctx.mask_sites(scan, S, lens, True, thr, out_valid=out_valid, sites=sites,
                                                                erased=erased), a.reps)
    res["mask_over_count"] = res["mask_sites_ms"] / res["sites_count_ms"]
    # (the counters are added to, and every pass starts from the input's validity: reps + 1 times the same figures)
    res["sites"] = int(sites.to_host().sum()) // (a.reps + 1)
    res["bases_erased"] = int(erased.to_host()[0]) // (a.reps + 1)
    del counts

    # ---- the device packer beside the host packer ----
    base, item = ctx.empty(n, np.uint64), ctx.empty(n, np.uint64)
    st = pk.PackedStruct()
    lib = pk.lib()

    def sizes(valid):
        pk._check(lib.pengk_pack_scan_sizes(ctx.h, valid, scan[2].ptr, scan[3].ptr, n, W, 0, base.ptr, item.ptr, C.byref(st)))

    sizes(out_valid.ptr)
    words, items = ctx.empty(st.n_words, np.uint64), ctx.empty(max(st.n_items, 1), np.uint64)

    def write(valid):
        pk._check(lib.pengk_pack_scan(ctx.h, scan[0].ptr, valid, scan[2].ptr, scan[3].ptr, n, W, 0, base.ptr, item.ptr, words.ptr,
                                      st.n_words, items.ptr, st.n_items))

    res["pack_scan_sizes_ms"] = median_ms(ctx, lambda: sizes(out_valid.ptr), a.reps)
    res["pack_scan_ms"] = median_ms(ctx, lambda: write(out_valid.ptr), a.reps)
    res["masked"] = {"n_words": st.n_words, "n_items": st.n_items, "n_windows": st.n_windows, "all_whole": st.all_whole}
    codes = host_codes(scan, n, L)
    offs = np.arange(n + 1, dtype=np.int64) * L
    hp = pk.PackedStruct()
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        pk._check(lib.pengk_pack_threads(codes.ctypes.data, offs.ctypes.data, n, W, 0, a.host_threads, C.byref(hp)))
        t.append((time.perf_counter() - t0) * 1e3)
        lib.pengk_packed_free(C.byref(hp))
    res["host_pack_ms"] = float(np.median(t))
    res["host_pack_threads"] = a.host_threads
    res["bytes_a_host_round_moves"] = int(scan[0].nbytes + out_valid.nbytes + st.n_words * 8 + st.n_items * 8)
    del codes

    # ---- one thread per sequence: what a single 200 000-base sequence costs (an invalid base every 1000) ----
    one = np.random.default_rng(2).integers(1, 5, 200_000).astype(np.uint8)
    one[::1000] = 0
    lscan = ctx.upload_scan(pk.ScanLayout(one, np.array([0, len(one)], np.int64)))
    res["one_200k_sequence_pack_ms"] = median_ms(ctx, lambda: ctx.pack_scan(lscan, W), a.reps)
    res["one_200k_sequence_mask_ms"] = median_ms(ctx, lambda: ctx.mask_sites(lscan, S, lens, True, thr), a.reps)

    # ---- the second round's count beside the first's ----
    ltot = ctx.empty(1, np.uint64)
    table = ctx.empty(4 ** W, np.uint32)
    ctx.set_sequences(words, items, st.n_words, st.n_items, W, st.item_windows, st.max_bin_bound, st.all_whole)
    ctx.set_option("n_windows_hint", st.n_windows)
    res["count_masked_ms"] = median_ms(ctx, lambda: ctx.count(True, counts=table, ltot=ltot), a.reps)
    res["ltot_masked"] = int(ltot.to_host()[0])
    sizes(None)
    words1, items1 = ctx.empty(st.n_words, np.uint64), ctx.empty(max(st.n_items, 1), np.uint64)
    pk._check(lib.pengk_pack_scan(ctx.h, scan[0].ptr, None, scan[2].ptr, scan[3].ptr, n, W, 0, base.ptr, item.ptr, words1.ptr,
                                  st.n_words, items1.ptr, st.n_items))
    ctx.set_sequences(words1, items1, st.n_words, st.n_items, W, st.item_windows, st.max_bin_bound, st.all_whole)
    ctx.set_option("n_windows_hint", st.n_windows)
    res["count_input_ms"] = median_ms(ctx, lambda: ctx.count(True, counts=table, ltot=ltot), a.reps)
    res["ltot_input"] = int(ltot.to_host()[0])
    ctx.close()

    # ---- the CLI, with and without the flag (a fresh process each: its own device context) ----
    if a.cli:
        cli, gen = os.path.join(ROOT, "peng-motif_amd", "host", "peng_motif"), os.path.join(ROOT, "tools", "synth_fasta")
        with tempfile.TemporaryDirectory() as d:
            fa = os.path.join(d, "s.fa")
            subprocess.run([gen, fa, str(n), str(L), "1", "0"], check=True)
            for key, extra in (("cli_s", []), ("cli_erase_s", ["--erase", os.path.join(d, "erase.tsv")])):
                t = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    subprocess.run([cli, fa, "-w", str(W), "-o", os.path.join(d, "o.meme")] + extra, check=True,
                                   stdout=subprocess.DEVNULL, timeout=600)
                    t.append(time.perf_counter() - t0)
                res[key] = float(np.median(t))
            with open(os.path.join(d, "erase.tsv")) as f:
                res["cli_erase_report"] = f.read().splitlines()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
