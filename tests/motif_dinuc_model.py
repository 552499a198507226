"""numpy restatement of the first-order motif models (--dinuc; include/pengk.h, "first-order motif models"; INTEGRATION.md
7i): the pair profiles of the best sites, the interpolated model with its mutual information and integer log-odds, the
first-order scan, and the two files the CLI writes.  The counts and the scan are integer, so the device must agree with
them bit for bit; the model between them is a fixed sequence of double operations (log2 through math.log2, the C
library's, one call per entry as the library makes it).

Two versions of the counts and of the scan: one per sequence, written from the definitions, and one vectorised over
sequences of one length (the approach of scan_batch_model.window_scores) for the sets too large for the first; the CPU
tests hold them equal."""
import math

import numpy as np

import motif_centrality_model as mc
import motif_refine_model as mr
import motif_score_model as ms
import motif_sites_model as mst
import scan_batch_model as sb

MAX_MOTIF_LEN = 64
SENTINEL = ms.SENTINEL
clamp_flank = mr.clamp_flank


# ---- 1. pair profiles ----------------------------------------------------------------------------------------------------
def _site_letter(c, L, p, s, w, col):
    """the letter 0..3 at column col of the site (p, s) read on its strand, or None (outside the sequence, not A/C/G/T)"""
    q = p + col if s == 0 else p + w - 1 - col
    if q < 0 or q >= L or not 1 <= c[q] <= 4:
        return None
    b = int(c[q]) - 1
    return b if s == 0 else 3 - b


def pair_profile(seqs, best, site, w, t, flank):
    """counts (MAX_MOTIF_LEN x 17 uint64; rows c + F, c in (-F, w + F); row 0 untouched) of one motif from its best sites,
    selected as motif_refine_model.site_profile selects them"""
    F = clamp_flank(w, flank)
    counts = np.zeros((MAX_MOTIF_LEN, 17), np.uint64)
    for i, c in enumerate(seqs):
        if best[i] == SENTINEL or best[i] < t or len(c) < w:
            continue
        p, s, L = int(site[i]) >> 1, int(site[i]) & 1, len(c)
        if p > L - w:
            continue
        for col in range(-F + 1, w + F):
            a, b = _site_letter(c, L, p, s, w, col - 1), _site_letter(c, L, p, s, w, col)
            counts[col + F, 16 if a is None or b is None else 4 * a + b] += np.uint64(1)
    return counts


def pair_profile_batch(codes, best, site, w, t, flank):
    """pair_profile of an (n, L) code array, without a loop over sequences"""
    codes = np.asarray(codes, np.uint8)
    n, L = codes.shape
    F = clamp_flank(w, flank)
    counts = np.zeros((MAX_MOTIF_LEN, 17), np.uint64)
    best = np.asarray(best, np.int64)
    p = (np.asarray(site, np.uint64) >> np.uint64(1)).astype(np.int64)
    s = (np.asarray(site, np.uint64) & np.uint64(1)).astype(np.int64)
    rows = np.nonzero((best != SENTINEL) & (best >= t) & (L >= w) & (p <= L - w))[0]
    if len(rows) == 0:
        return counts
    p, s = p[rows], s[rows]

    def letter(col):
        q = np.where(s == 0, p + col, p + w - 1 - col)
        c = codes[rows, np.clip(q, 0, L - 1)].astype(np.int64)
        ok = (q >= 0) & (q < L) & (c >= 1) & (c <= 4)
        return ok, np.where(s == 0, c - 1, 4 - c)

    pok, pb = letter(-F)
    for col in range(-F + 1, w + F):
        ok, b = letter(col)
        counts[col + F] += np.bincount(np.where(ok & pok, 4 * pb + b, 16), minlength=17).astype(np.uint64)
        pok, pb = ok, b
    return counts


def pair_profile_mixed(codes, offs, best, site, w, t, flank):
    counts = np.zeros((MAX_MOTIF_LEN, 17), np.uint64)
    for L, idx in sb.length_classes(offs):
        if L:
            counts += pair_profile_batch(sb.class_codes(codes, offs, idx, L), np.asarray(best)[idx], np.asarray(site)[idx], w, t,
                                         flank)
    return counts


# ---- 2. the model --------------------------------------------------------------------------------------------------------
def lo(p, g):
    """clamp(lround(100 log2(p / g)), -2000, 2000): lround takes halves away from zero"""
    v = max(-2000.0, min(2000.0, 100.0 * math.log2(p / g)))
    r = math.floor(abs(v))
    if abs(v) - r >= 0.5:  # (exact: both are doubles below 2^53)
        r += 1
    return int(r) if v >= 0 else -int(r)


def dinuc_model(counts1, counts2, w, flank, bg0, bg1, alpha):
    """pengk_dinuc_model: a dict with q0 (W x 4), q1 (W x 16), mi (W), S0 (4), D1, D0 (W x 16 int32, row 0 zero), sites and
    flank (the clamped F); counts1: W x 5, counts2: W x 17 rows at least"""
    F = clamp_flank(w, flank)
    W = w + 2 * F
    g0 = [float(x) for x in np.asarray(bg0, np.float32)]
    g1 = [float(x) for x in np.asarray(bg1, np.float32).reshape(-1)]
    alpha = float(alpha)
    q0, q1, mi = np.zeros((W, 4), np.float64), np.zeros((W, 16), np.float64), np.zeros(W, np.float64)
    S0, D1, D0 = np.zeros(4, np.int32), np.zeros((W, 16), np.int32), np.zeros((W, 16), np.int32)
    for c in range(W):
        k1 = [int(x) for x in counts1[c]]
        k2 = [int(x) for x in counts2[c]]
        n1 = k1[0] + k1[1] + k1[2] + k1[3]
        for b in range(4):
            q0[c, b] = (float(k1[b]) + g0[b]) / (float(n1) + 1.0)
        if c == 0:
            for b in range(4):
                S0[b] = lo(q0[0, b], g0[b])
        row = [k2[4 * a] + k2[4 * a + 1] + k2[4 * a + 2] + k2[4 * a + 3] for a in range(4)]
        col = [k2[b] + k2[4 + b] + k2[8 + b] + k2[12 + b] for b in range(4)]
        for a in range(4):
            for b in range(4):
                x = 4 * a + b
                if c == 0:
                    q1[c, x] = q0[0, b]
                    continue
                q1[c, x] = (float(k2[x]) + alpha * float(q0[c, b])) / (float(row[a]) + alpha)
                D1[c, x] = lo(float(q1[c, x]), g1[x])
                D0[c, x] = lo(float(q0[c, b]), g1[x])
        N = sum(row)
        acc = 0.0
        if c >= 1 and N > 0:
            for a in range(4):
                for b in range(4):
                    k = k2[4 * a + b]
                    if k > 0:
                        acc += (float(k) / float(N)) * math.log2((float(k) * float(N)) / (float(row[a]) * float(col[b])))
        mi[c] = acc
    return {"q0": q0, "q1": q1, "mi": mi, "S0": S0, "D1": D1, "D0": D0, "flank": F,
            "sites": int(np.asarray(counts1[F], np.uint64).sum())}


def degenerate(S):
    """(S0, D) of the first-order model that scores like the PWM log-odds S: D[c][4a + b] = S[c][b]"""
    S = np.asarray(S, np.int32)
    return S[0].copy(), np.ascontiguousarray(np.repeat(S[:, None, :], 4, axis=1).reshape(len(S), 16))


# ---- 3. the first-order scan -----------------------------------------------------------------------------------------------
def window_score(x, S0, D):
    """S0[x_0] + sum_{c >= 1} D[c][4 x_{c-1} + x_c] of one window of bases 0..3"""
    return int(S0[x[0]]) + sum(int(D[c][4 * x[c - 1] + x[c]]) for c in range(1, len(x)))


def best_scores(seqs, S0, D, both):
    """best window score of every sequence (SENTINEL without a window of A/C/G/T only); seqs: byte codes; D: w x 16"""
    S0, D = np.asarray(S0, np.int64), np.asarray(D, np.int64).reshape(-1, 16)
    w = len(D)
    out = np.full(len(seqs), SENTINEL, np.int64)
    for i, c in enumerate(seqs):
        c = np.asarray(c, np.int64)
        L = len(c)
        if L < w:
            continue
        ok = (c >= 1) & (c <= 4)
        bad = np.concatenate([[0], np.cumsum(~ok)])
        starts = np.arange(L - w + 1)
        good = (bad[starts + w] - bad[starts]) == 0
        if not good.any():
            continue
        x = np.where(ok, c - 1, 0)[starts[:, None] + np.arange(w)[None, :]][good]
        strands = [x, 3 - x[:, ::-1]] if both else [x]  # y_j = 3 - x_{w-1-j}
        best = None
        for y in strands:
            sc = S0[y[:, 0]]
            for col in range(1, w):
                sc = sc + D[col][4 * y[:, col - 1] + y[:, col]]
            best = int(sc.max()) if best is None else max(best, int(sc.max()))
        out[i] = best
    return out


def window_scores(codes, S0, D, both):
    """(sc, good) as scan_batch_model.window_scores, for a first-order model.  The - strand in window positions: the single
    term S0[3 - x_{w-1}] and, for the positions (j - 1, j), D[w - j][4 (3 - x_j) + (3 - x_{j-1})]."""
    codes = np.asarray(codes, np.uint8)
    n, L = codes.shape
    S0, D = np.asarray(S0, np.int32), np.asarray(D, np.int32).reshape(-1, 16)
    w = len(D)
    ns = 2 if both else 1
    nwin = max(L - w + 1, 0)
    sc = np.zeros((ns, n, nwin), np.int32)
    if nwin == 0 or n == 0:
        return sc, np.zeros((n, nwin), bool)
    ok = (codes >= 1) & (codes <= 4)
    bad = np.zeros((n, L + 1), np.int32)
    np.cumsum(~ok, axis=1, out=bad[:, 1:])
    good = (bad[:, w:] - bad[:, :nwin]) == 0
    b = np.where(ok, codes, 1).astype(np.intp) - 1
    sc[0] += np.take(S0, b[:, 0:nwin])
    for j in range(1, w):
        sc[0] += np.take(D[j], 4 * b[:, j - 1:j - 1 + nwin] + b[:, j:j + nwin])
    if both:
        sc[1] += np.take(S0, 3 - b[:, w - 1:w - 1 + nwin])
        for j in range(1, w):
            sc[1] += np.take(D[w - j], 4 * (3 - b[:, j:j + nwin]) + (3 - b[:, j - 1:j - 1 + nwin]))
    return sc, good


def best_scores_batch(codes, S0, D, both):
    """best_scores of an (n, L) code array, CHUNK_CELLS bases at a time"""
    codes = np.asarray(codes, np.uint8)
    n, L = codes.shape
    out = np.full(n, SENTINEL, np.int64)
    step = max(1, sb.CHUNK_CELLS // max(L, 1))
    for a in range(0, n, step):
        sc, good = window_scores(codes[a:a + step], S0, D, both)
        if sc.shape[2]:
            out[a:a + step] = np.where(good[None], sc, SENTINEL).max(axis=(0, 2))
    return out


def best_scores_mixed(codes, offs, S0, D, both):
    out = np.full(len(offs) - 1, SENTINEL, np.int64)
    for L, idx in sb.length_classes(offs):
        out[idx] = best_scores_batch(sb.class_codes(codes, offs, idx, L), S0, D, both)
    return out


def score_range(S0, D):
    S0, D = np.asarray(S0, np.int64), np.asarray(D, np.int64).reshape(-1, 16)
    return int(S0.min() + D[1:].min(axis=1).sum()), int(S0.max() + D[1:].max(axis=1).sum())


# ---- the step and its two files ------------------------------------------------------------------------------------------
def mi_summary(mod):
    """(mi_total, mi_max, mi_max_pair): the pair's second member as a 1-based column of the found PWM; the smaller column
    wins ties; zeros without sites or without a pair"""
    W, F = len(mod["mi"]), mod["flank"]
    total, best, pair = 0.0, 0.0, 0
    if mod["sites"]:
        for c in range(1, W):
            total += float(mod["mi"][c])
            if c == 1 or mod["mi"][c] > best:
                best, pair = float(mod["mi"][c]), c - F + 1
    return total, best, pair


def site_counts(seqs, S, m, both, pvalue, flank, bg0, batch=False):
    """(counts1, counts2) of the best sites of the found PWM's log-odds S, scanned as motif m (its index seeds the
    tie-break), at p-value pvalue or below; batch: by the vectorised versions, one length class at a time"""
    S = np.asarray(S, np.int32)
    w = len(S)
    lo_, tail = mst.tail_pvalues(S, bg0)
    thr = mst.threshold(lo_, tail, pvalue)
    if batch:
        codes, offs = ms.flatten(seqs)
        r = sb.scan_mixed(codes, offs, S, both, m=m)
        return (sb.site_profile_mixed(codes, offs, r["best_site"], r["site"], w, thr, flank),
                pair_profile_mixed(codes, offs, r["best_site"], r["site"], w, thr, flank))
    best, site = mc.best_sites(seqs, S, both, m)
    return mr.site_profile(seqs, best, site, w, thr, flank), pair_profile(seqs, best, site, w, thr, flank)


def analyse(seqs, negs, S, m, bg0, bg1, both, pvalue=1e-4, flank=0, alpha=20.0, batch=False, counts=None):
    """the step for one motif: seqs / negs byte codes, S and m as in site_counts (counts: its result, if the caller has
    it).  A dict: the model's fields, width, auc0, auc1, gain, mi_total, mi_max, mi_max_pair"""
    w = len(S)
    k1, k2 = counts if counts is not None else site_counts(seqs, S, m, both, pvalue, flank, bg0, batch)
    mod = dinuc_model(k1, k2, w, flank, bg0, bg1, alpha)
    mod["width"] = w + 2 * mod["flank"]
    if batch:
        flat = [ms.flatten(x) for x in (seqs, negs)]
        scan = lambda k, D: best_scores_mixed(flat[k][0], flat[k][1], mod["S0"], D, both)
    else:
        scan = lambda k, D: best_scores((seqs, negs)[k], mod["S0"], D, both)
    for k, D in (("auc0", mod["D0"]), ("auc1", mod["D1"])):
        a, b = score_range(mod["S0"], D)
        P = ms.histogram(scan(0, D), a, b)
        N = ms.histogram(scan(1, D), a, b)
        mod[k] = ms.auc(P, N)
    mod["gain"] = mod["auc1"] - mod["auc0"]
    mod["mi_total"], mod["mi_max"], mod["mi_max_pair"] = mi_summary(mod)
    return mod


REPORT_HEAD = "motif\tindex\twidth\tflank\tsites\tauc_order0\tauc_order1\tauc_gain\tmi_total\tmi_max\tmi_max_pair\n"


def report_line(name, index, r):
    """one line of the --dinuc report (index 1-based)"""
    if not r["sites"]:
        return "%s\t%d\t%d\t%d\t0\t%.6f\t%.6f\t%.6f\t%.6f\t%.6f\t0\n" % (name, index, r["width"], r["flank"], 0, 0, 0, 0, 0)
    return "%s\t%d\t%d\t%d\t%d\t%.6f\t%.6f\t%.6f\t%.6f\t%.6f\t%d\n" % (
        name, index, r["width"], r["flank"], r["sites"], r["auc0"], r["auc1"], r["gain"], r["mi_total"], r["mi_max"],
        r["mi_max_pair"])


def models_head(alpha, bg_order):
    return "# first-order motif models: alpha= %g bg_order= %d\n" % (float(alpha), 1 if bg_order >= 1 else 0)


def models_block(name, r):
    """one motif of the --dinuc-models file"""
    o = "MOTIF %s w= %d nsites= %d left= %d right= %d\n" % (name, r["width"], r["sites"], r["flank"], r["flank"])
    for c in range(r["width"]):
        o += " ".join("%.8f" % float(x) for x in r["q0"][c]) + "\n"
        o += " ".join("%.8f" % float(x) for x in r["q1"][c]) + "\n"
    return o + "\n"
