"""Times the motif comparison on the device (include/pengk.h, "motif comparison"): Q queries of widths 10..14 against T
synthetic targets of widths 6..19 (Dirichlet(0.3) columns), both orientations -- pengk_compare_nulls alone and the whole
of pengk_compare_motifs (upload, nulls, tails, alignments, download), wall clock around the calls (they synchronise with the
host), median of --reps after one warm-up; then one query of width 64 alone (the longest chains of convolutions).  Before
timing, a sample of the records is held to the numpy model (tests/motif_compare_model.py).  Prints one JSON line.
  python tools/compare_probe.py [--queries 16] [--targets 10000] [--min-overlap 5] [--reps 5] [--plus]"""
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
import motif_compare_model as mc  # noqa: E402


def timed(fn, reps):
    out, times = None, []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        out = fn()
        if rep:
            times.append((time.perf_counter() - t0) * 1e3)
    return out, float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=16)
    ap.add_argument("--targets", type=int, default=10000)
    ap.add_argument("--min-overlap", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--plus", action="store_true")
    a = ap.parse_args()
    both = not a.plus
    rng = np.random.default_rng(18)
    targets = mc.decoys(rng, a.targets)
    queries = [mc.random_motif(rng, 10 + (m % 5)) for m in range(a.queries)]
    ctx = pk.Context(0)

    # (the ctypes calls alone: padding 10 000 motifs in Python takes longer than the device does)
    L = pk.lib()

    def padded(motifs):
        X, ln = pk._pad_columns(motifs)
        return X, ln, len(motifs)

    def nulls(Q, T):
        hist = np.zeros((Q[2], pk.MAX_MOTIF_LEN, pk.COMPARE_BINS), np.uint64)
        pk._check(L.pengk_compare_nulls(ctx.h, Q[2], Q[0].ctypes.data, Q[1].ctypes.data, T[2], T[0].ctypes.data, T[1].ctypes.data,
                                        int(both), hist.ctypes.data))
        return hist

    def compare(Q, T):
        align, p = np.zeros((Q[2], T[2], 5), np.int32), np.zeros((Q[2], T[2]), np.float64)
        pk._check(L.pengk_compare_motifs(ctx.h, Q[2], Q[0].ctypes.data, Q[1].ctypes.data, T[2], T[0].ctypes.data, T[1].ctypes.data,
                                         int(both), a.min_overlap, align.ctypes.data, p.ctypes.data))
        return align, p

    wide = [mc.random_motif(rng, 64)]
    Qp, Tp, Wp = padded(queries), padded(targets), padded(wide)
    hist, nulls_ms = timed(lambda: nulls(Qp, Tp), a.reps)
    (align, p), all_ms = timed(lambda: compare(Qp, Tp), a.reps)
    _, wide_ms = timed(lambda: compare(Wp, Tp), a.reps)

    # a sample against the model: query 0's histograms, and its records for the first 50 targets
    h = mc.null_histograms(queries[0], targets, both)
    assert hist[0, :len(queries[0])].tobytes() == h.tobytes(), "null histograms differ from the model's"
    rec = mc.compare_query(queries[0], targets, both, a.min_overlap, h=h, only=range(50))
    for t in range(50):
        mine = [x for x in rec["all"][t] if (x["offset"], x["orientation"]) == (align[0, t, 0], align[0, t, 1])]
        assert len(mine) == 1 and (mine[0]["overlap"], mine[0]["score"]) == (align[0, t, 2], align[0, t, 3]), t
        assert abs(p[0, t] - mine[0]["p"]) <= 1e-9 * mine[0]["p"] + 1e-300, t
        assert mine[0]["p"] == rec["p_offset"][t] or mine[0] in rec["near"][t], t
    t0 = time.perf_counter()
    for m in range(len(queries)):
        pk.compare_summary(p[m], align[m, :, 4])
    summary_ms = (time.perf_counter() - t0) * 1e3
    cols = int(sum(len(t) for t in targets))
    print(json.dumps({"probe": "motif_compare", "queries": len(queries), "query_widths": [len(q) for q in queries],
                      "targets": len(targets), "database_columns": cols, "strands": 2 if both else 1,
                      "min_overlap": a.min_overlap, "nulls_ms": round(nulls_ms, 3), "compare_ms": round(all_ms, 3),
                      "summary_cpu_ms": round(summary_ms, 3), "one_query_of_width_64_ms": round(wide_ms, 3),
                      "best_evalue": float(min(pk.compare_summary(p[m], align[m, :, 4])[1].min() for m in range(len(queries)))),
                      "reps": a.reps}))
    ctx.close()


if __name__ == "__main__":
    main()
