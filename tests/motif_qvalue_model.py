"""numpy restatement of the sites' q-values (--sites-qvalue; include/pengk.h, pengk_sites_histograms /
pengk_sites_qvalues / pengk_qvalue_threshold): per motif the histogram of the site scores and the
number of scored window strands, Benjamini-Hochberg over the reported set with the full number of tests, and the TSV
with its q_value column.  The histogram is integer and the q-values a fixed sequence of IEEE double operations on it, so
the library must agree with this file bit for bit, the "%.3g" text included."""
import numpy as np

import motif_sites_model as mst
import scan_batch_model as sb

HEADER = "#motif_index\tmotif_id\tsequence_name\tstart\tstop\tstrand\tscore\tp_value\tq_value\tmatched_sequence\n"


def score_hi(S):
    """the highest score of S: the sum of the column maxima"""
    return int(np.asarray(S, np.int64).max(axis=1).sum())


def n_bins(S, t):
    return max(0, score_hi(S) - int(t) + 1)


def histogram(seqs, S, t, both):
    """(hist, N) of one motif over seqs (a list of byte-code arrays): hist[s - t] (uint64, hi - t + 1 bins, none when
    t = hi + 1) the window strands with score exactly s >= t -- the sites of motif_sites_model.sites --, N the scored
    window strands: the windows whose w bases are all A/C/G/T, counted twice with `both`"""
    S = np.asarray(S, np.int64)
    w = S.shape[0]
    hist = np.zeros(n_bins(S, t), np.uint64)
    sc = np.array([s[3] for s in mst.sites(seqs, S, t, both)], np.int64)
    if len(sc):
        hist += np.bincount(sc - int(t), minlength=len(hist)).astype(np.uint64)
    N = 0
    for c in seqs:
        c = np.asarray(c, np.int64)
        if len(c) < w:
            continue
        bad = np.concatenate([[0], np.cumsum((c < 1) | (c > 4))])
        N += int(((bad[w:] - bad[:len(c) - w + 1]) == 0).sum())
    return hist, N * (2 if both else 1)


def histogram_batch(codes, S, t, both):
    """histogram() of an (n, L) code array, through scan_batch_model.window_scores, a chunk of sequences at a time"""
    codes = np.asarray(codes, np.uint8)
    n, L = codes.shape
    hist = np.zeros(n_bins(S, t), np.uint64)
    N = 0
    step = max(1, sb.CHUNK_CELLS // max(L, 1))
    for a in range(0, n, step):
        sc, good = sb.window_scores(codes[a:a + step], S, both)
        N += int(good.sum()) * sc.shape[0]
        for k in range(sc.shape[0]):
            s = sc[k][good & (sc[k] >= t)].astype(np.int64)
            if len(s):
                hist += np.bincount(s - int(t), minlength=len(hist)).astype(np.uint64)
    return hist, N


def qvalues(hist, N, tail_from_thr):
    """q[k] of the sites with score t + k.  n(k) = sum over k' >= k of hist[k'] (uint64, from the top down);
    r(k) = double(N) * tail_from_thr[k] / double(n(k)) -- one multiplication, then one division -- or +inf when n(k) = 0;
    q[k] = min(1.0, min over k' <= k of r(k')), a running minimum from bin 0 up"""
    h = np.asarray(hist, np.uint64)
    nb = len(h)
    n = np.cumsum(h[::-1], dtype=np.uint64)[::-1]
    r = np.full(nb, np.inf)
    nz = n > 0
    x = np.float64(int(N)) * np.asarray(tail_from_thr, np.float64)[:nb][nz]
    r[nz] = x / n[nz].astype(np.float64)
    return np.minimum(1.0, np.minimum.accumulate(r)) if nb else r


def qvalue_threshold(q, t, Q):
    """the smallest score t + k with q[k] <= Q, else t + len(q)"""
    ok = np.nonzero(np.asarray(q) <= Q)[0]
    return int(t) + (int(ok[0]) if len(ok) else len(q))


def motif_qvalues(seqs, S, bg, P, both):
    """(lo, tail, t, hist, N, q) of one motif at --sites-pvalue P"""
    lo, tail = mst.tail_pvalues(S, bg)
    t = mst.threshold(lo, tail, P)
    hist, N = histogram(seqs, S, t, both)
    return lo, tail, t, hist, N, qvalues(hist, N, tail[t - lo:])


def render(seqs, names, motif_ids, Ss, bg, P, both, Q=None, header=True, first_index=1):
    """the --sites --sites-qvalue TSV (str); Q: --sites-qvalue-max, only the lines with q <= Q (the q-values stay those
    of the set at P)"""
    lines = [HEADER] if header else []
    for m, S in enumerate(Ss):
        lo, tail, t, hist, N, q = motif_qvalues(seqs, S, bg, P, both)
        t2 = t if Q is None else qvalue_threshold(q, t, Q)
        w = len(S)
        for i, p, st, sc in mst.sites(seqs, S, t2, both):
            bases = "".join("ACGT"[x - 1] for x in seqs[i][p:p + w])
            if st:
                bases = bases[::-1].translate(str.maketrans("ACGT", "TGCA"))
            lines.append("%d\t%s\t%s\t%d\t%d\t%s\t%s\t%.3g\t%.3g\t%s\n" % (m + first_index, motif_ids[m], names[i], p + 1, p + w, "+-"[st],
                                                                          mst.fmt_score(sc), tail[sc - lo], q[sc - t], bases))
    return "".join(lines)
