"""numpy restatement of the motif refinement (--refine; include/pengk.h, "motif refinement"): the site
profiles of the best sites, the new matrix and its kept columns, the rounds and the MEME file the CLI writes.  Up to the
counts everything is integer, so the device must agree with it bit for bit; the new matrix is a fixed sequence of double
operations on those integers (log2 through math.log2, the C library's, one call per entry as the library makes it)."""
import math

import numpy as np

import motif_centrality_model as mc
import motif_score_model as ms
import motif_sites_model as mst

MAX_MOTIF_LEN = 64


def clamp_flank(w, flank):
    return min(int(flank), (MAX_MOTIF_LEN - int(w)) // 2)


def site_profile(seqs, best, site, w, t, flank):
    """counts (MAX_MOTIF_LEN x 5 uint64; rows c + F, c in [-F, w + F)) of one motif from its best sites: sequences with
    a score (not SENTINEL) >= t; seqs: byte codes (1..4 = A,C,G,T, else invalid)"""
    F = clamp_flank(w, flank)
    counts = np.zeros((MAX_MOTIF_LEN, 5), np.uint64)
    for i, c in enumerate(seqs):
        if best[i] == ms.SENTINEL or best[i] < t or len(c) < w:
            continue
        p, s, L = int(site[i]) >> 1, int(site[i]) & 1, len(c)
        if p > L - w:
            continue
        for col in range(-F, w + F):
            q = p + col if s == 0 else p + w - 1 - col
            if q < 0 or q >= L or not 1 <= c[q] <= 4:
                counts[col + F, 4] += np.uint64(1)
            else:
                b = int(c[q]) - 1
                counts[col + F, b if s == 0 else 3 - b] += np.uint64(1)
    return counts


def profile_refine(counts, w, flank, bg, min_ic):
    """pengk_profile_refine: a dict with q, ic, first, last, pwm (float32), sites"""
    F = clamp_flank(w, flank)
    n_col = w + 2 * F
    g = [float(x) for x in np.asarray(bg, np.float32)]
    q = np.zeros((n_col, 4), np.float64)
    ic = np.zeros(n_col, np.float64)
    for c in range(n_col):
        k = [int(x) for x in counts[c]]
        n = k[0] + k[1] + k[2] + k[3]
        acc = 0.0
        for b in range(4):
            v = (float(k[b]) + g[b]) / (float(n) + 1.0)
            acc += v * math.log2(v / g[b])
            q[c, b] = v
        ic[c] = acc
    keep = np.nonzero(ic >= min_ic)[0]
    first, last = (int(keep[0]), int(keep[-1]) + 1) if len(keep) else (0, 0)
    return {"q": q, "ic": ic, "first": first, "last": last, "pwm": q[first:last].astype(np.float32),
            "sites": int(np.asarray(counts[F], np.uint64).sum())}


def refine(seqs, pwms, bg, both, pvalue=1e-4, flank=8, iterations=3, min_ic=0.25, S0=None, only=None):
    """the rounds of every motif: a list of dicts with pwm (float32), sites, rounds, left, right.  Every motif is scanned
    in every round under its own index (the tie-break's key holds it); S0: the first round's log-odds, if not those of
    pwms (a caller that knows them better than an 8-decimal PWM does); only: run this motif alone, under its index (the
    others' entries are not looked at: motifs do not depend on each other)"""
    mot = [{"pwm": np.asarray(p, np.float32), "w0": len(p), "sites": 0, "rounds": 0, "left": 0, "right": 0, "active": True,
            "prev": None} if only in (None, m) else {"active": False} for m, p in enumerate(pwms)]
    for t in range(iterations):
        if not any(r["active"] for r in mot):
            break
        for m, r in enumerate(mot):
            if not r["active"]:
                continue
            S = np.asarray(S0[m], np.int32) if (t == 0 and S0 is not None) else ms.log_odds(r["pwm"], bg)
            w = len(S)
            lo, tail = mst.tail_pvalues(S, bg)
            thr = mst.threshold(lo, tail, pvalue)
            best, site = mc.best_sites(seqs, S, both, m)
            counts = site_profile(seqs, best, site, w, thr, flank)
            got = profile_refine(counts, w, flank, bg, min_ic)
            if got["sites"] == 0 or got["first"] == got["last"]:
                r["active"] = False
                continue
            F = clamp_flank(w, flank)
            a, b = -r["left"] - F + got["first"], -r["left"] - F + got["last"]
            kept = counts[got["first"]:got["last"]].tobytes()
            if r["prev"] == (a, b, kept):
                r["active"] = False
            r["prev"] = (a, b, kept)
            r["pwm"], r["left"], r["right"] = got["pwm"], -a, b - r["w0"]
            r["rounds"] += 1
            r["sites"] = got["sites"]
    return mot


def render(ids, mot, bg):
    """the MEME file of --refine"""
    o = "MEME version 4\n\nALPHABET= ACGT\n\nBackground letter frequencies\n"
    o += " ".join("%s %g" % (a, float(x)) for a, x in zip("ACGT", np.asarray(bg, np.float32))) + "\n\n"
    for name, r in zip(ids, mot):
        o += "MOTIF %s\n" % name
        o += "letter-probability matrix: alength= 4 w= %d nsites= %d iterations= %d left= %d right= %d\n" % (
            len(r["pwm"]), r["sites"], r["rounds"], r["left"], r["right"])
        for row in r["pwm"]:
            o += " ".join("%.8f" % float(x) for x in row) + "\n"
        o += "\n"
    return o
