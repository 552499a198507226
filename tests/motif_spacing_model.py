"""numpy restatement of the motif pair test (--spacing; include/pengk.h, "motif pair spacing"): the
pair histograms from the best sites, the co-occurrence and gap tests and the TSV the CLI writes.  Up to the histograms
everything is integer, so the device must agree with it bit for bit; the summary is floating point and agrees to
rounding."""
import math

import numpy as np

import motif_centrality_model as mc
from motif_score_model import SENTINEL

MAX_LEN = mc.MAX_LEN
MAX_MOTIFS = 64
MAX_GAP = 1024
CLASSES = ("same_downstream", "same_upstream", "opposite_downstream", "opposite_upstream")
HEADER = ("#motif_a\tid_a\tmotif_b\tid_b\tsequences\tsites_a\tsites_b\tboth\texpected_both\tlog10_pvalue_both\toverlapping\t"
          "apart\tfar\torientation\tgap\tcount\texpected\tenrichment\tlog10_pvalue\tlog10_evalue\tgaps\n")


def n_bins(G):
    return 4 * (G + 1) + 2


def pair_index(a, b):
    assert a < b
    return b * (b - 1) // 2 + a


def classify(pa, sa, wa, pb, sb, wb, G):
    """the gap bin of one pair of sites, and whether they are apart"""
    if pa < pb + wb and pb < pa + wa:
        return 4 * (G + 1), False
    side = 0 if pb >= pa + wa else 1
    g = pb - pa - wa if side == 0 else pa - pb - wb
    c = 2 * (sa ^ sb) + (side ^ sa)
    return (c * (G + 1) + g if g <= G else 4 * (G + 1) + 1), True


def has_site(best, site, lens, w, t, min_len, max_len):
    """the sequences where a motif has a site: considered, a window at all, score >= t, the window inside the sequence"""
    best = np.asarray(best, np.int64)
    lens = np.asarray(lens, np.int64)
    p = (np.asarray(site, np.uint64) >> np.uint64(1)).astype(np.int64)
    return (lens >= min_len) & (lens <= max_len) & (best != SENTINEL) & (best >= t) & (p <= lens - w)


def histograms(best, site, lens, widths, thr, G, min_len, max_len):
    """(hg, hl, hm) uint64: pairs x B gap bins, pairs x (max_len + 1) length bins, n_m per motif; best / site: n_motifs
    x n_seq as pengk_motif_best_sites leaves them"""
    M = len(widths)
    lens = np.asarray(lens, np.int64)
    best = np.asarray(best).reshape(M, -1)
    site = np.asarray(site, np.uint64).reshape(M, -1)
    pairs = M * (M - 1) // 2
    B = n_bins(G)
    hg = np.zeros((max(pairs, 1), B), np.uint64)
    hl = np.zeros((max(pairs, 1), max_len + 1), np.uint64)
    has = [has_site(best[m], site[m], lens, widths[m], thr[m], min_len, max_len) for m in range(M)]
    hm = np.array([int(h.sum()) for h in has] + [0] * (M == 0), np.uint64)
    P = (site >> np.uint64(1)).astype(np.int64)
    S = (site & np.uint64(1)).astype(np.int64)
    for b in range(1, M):
        for a in range(b):
            sel = has[a] & has[b]
            if not sel.any():
                continue
            pa, pb, sa, sb, L = P[a][sel], P[b][sel], S[a][sel], S[b][sel], lens[sel]
            wa, wb = widths[a], widths[b]
            over = (pa < pb + wb) & (pb < pa + wa)
            side = np.where(pb >= pa + wa, 0, 1)
            g = np.where(side == 0, pb - pa - wa, pa - pb - wb)
            c = 2 * (sa ^ sb) + (side ^ sa)
            bins = np.where(over, 4 * (G + 1), np.where(g <= G, c * (G + 1) + np.minimum(g, G), 4 * (G + 1) + 1))
            q = pair_index(a, b)
            hg[q] = np.bincount(bins, minlength=B).astype(np.uint64)
            hl[q] = np.bincount(L[~over], minlength=max_len + 1).astype(np.uint64)
    return hg, hl, hm


def placements(L, wa, wb, g):
    """k(L, g): the placements of one side with gap g on a sequence of L bases"""
    return max(0, L - wa - wb - g + 1)


def gap_probability(hl, wa, wb, g, C):
    """p(g) of one pair from its length bins: the mean over the apart sequences of k(L, g) / (C K(L)), ascending L"""
    hl = np.asarray(hl, np.int64)
    Na = int(hl.sum())
    s = 0.0
    for L in np.nonzero(hl)[0]:
        T = int(L) - wa - wb + 1
        k = placements(int(L), wa, wb, g)
        if k > 0:
            s += float(int(hl[L])) * float(k) / (float(C) * float(T * (T + 1) // 2))
    return s / float(Na)


def summary(hg, hl, G, max_len, wa, wb, C, n, n_a, n_b, n_pairs):
    """the test of one pair, as pengk_spacing_summary returns it"""
    hg = np.asarray(hg, np.int64)
    hl = np.asarray(hl, np.int64)
    G1 = G + 1
    out = dict(both=0, overlapping=int(hg[4 * G1]), apart=0, far=int(hg[4 * G1 + 1]), expected_both=0.0, log10_pvalue_both=0.0,
               orientation=0, gap=0, count=0, expected=0.0, log10_pvalue=0.0, log10_evalue=0.0, tested_gaps=0)
    out["apart"] = int(hg[:4 * G1].sum()) + out["far"]
    out["both"] = out["overlapping"] + out["apart"]
    assert out["apart"] == int(hl.sum())
    if n:
        p_co = (float(n_a) / float(n)) * (float(n_b) / float(n))
        out["expected_both"] = float(n) * p_co
        out["log10_pvalue_both"] = mc.log10_sf(n, out["both"], p_co)
    Na = out["apart"]
    if Na == 0:
        return out
    pg = [gap_probability(hl, wa, wb, g, C) for g in range(G1)]
    out["tested_gaps"] = sum(p > 0.0 for p in pg)
    best = None
    for c in range(C):
        for g in range(G1):
            if not pg[g] > 0.0:
                continue
            H = int(hg[c * G1 + g])
            lp = mc.log10_sf(Na, H, min(1.0, pg[g]))
            if best is None or lp < best[0]:
                best = (lp, c, g, H)
    lp, c, g, H = best
    out.update(orientation=c, gap=g, count=H, expected=float(Na) * pg[g], log10_pvalue=lp,
               log10_evalue=lp + math.log10(float(C) * float(out["tested_gaps"])) + math.log10(float(n_pairs)))
    return out


def line(a, id_a, b, id_b, n, n_a, n_b, hg, G, sm):
    """one TSV line (without the newline) from a summary; a, b 0-based"""
    head = "%d\t%s\t%d\t%s\t%d\t%d\t%d\t%d\t%.2f\t%.3f\t%d\t%d\t%d" % (
        a + 1, id_a, b + 1, id_b, n, n_a, n_b, sm["both"], sm["expected_both"], sm["log10_pvalue_both"], sm["overlapping"],
        sm["apart"], sm["far"])
    if sm["apart"] == 0:
        return head + "\tNA" * 8
    c = sm["orientation"]
    gaps = ",".join(str(int(x)) for x in np.asarray(hg)[c * (G + 1):(c + 1) * (G + 1)])
    return head + "\t%s\t%d\t%d\t%.2f\t%.3f\t%.3f\t%.3f\t%s" % (CLASSES[c], sm["gap"], sm["count"], sm["expected"],
                                                               sm["count"] / sm["expected"], sm["log10_pvalue"],
                                                               sm["log10_evalue"], gaps)


def render(seqs, motif_ids, Ss, ts, both, G=150, n_motifs=16, max_len=None):
    """the --spacing TSV (str) of the first n_motifs of the motifs Ss (MEME order) with thresholds ts over seqs (byte
    codes)"""
    Ss, ts, motif_ids = Ss[:n_motifs], ts[:n_motifs], motif_ids[:n_motifs]
    M = len(Ss)
    lens = np.array([len(c) for c in seqs], np.int64)
    if max_len is None:
        ok = lens[lens <= MAX_LEN]
        max_len = max(int(ok.max()) if len(ok) else 1, 1)
    out = [HEADER]
    if M < 2:
        return HEADER
    widths = [len(S) for S in Ss]
    wmax = max(widths)
    n = int(((lens >= wmax) & (lens <= max_len)).sum())
    bs = [mc.best_sites(seqs, S, both, m) for m, S in enumerate(Ss)]
    hg, hl, hm = histograms(np.stack([b for b, _ in bs]), np.stack([s for _, s in bs]), lens, widths, ts, G, wmax, max_len)
    pairs = M * (M - 1) // 2
    for b in range(1, M):
        for a in range(b):
            q = pair_index(a, b)
            sm = summary(hg[q], hl[q], G, max_len, widths[a], widths[b], 4 if both else 2, n, int(hm[a]), int(hm[b]), pairs)
            out.append(line(a, motif_ids[a], b, motif_ids[b], n, int(hm[a]), int(hm[b]), hg[q], G, sm) + "\n")
    return "".join(out)
