"""numpy restatement of the central-enrichment test (--centrality; include/pengk.h, "central enrichment"; INTEGRATION.md
7d): the best window strand of every motif on every sequence with its keyed tie-break, the offset and length histograms,
the null f(L, w, r), the binomial tail in log space and the TSV the CLI writes.  Up to the histograms everything is
integer, so the device must agree with it bit for bit; the summary is floating point and agrees to rounding."""
import math

import numpy as np

from motif_score_model import GOLDEN, SENTINEL, mix64, revcomp_S

MAX_LEN = 65536
HEADER = ("#motif_index\tmotif_id\twidth\tsequences\tsites\tcenter_distance\tsites_in_window\texpected_in_window\t"
          "enrichment\tlog10_pvalue\tlog10_evalue\toffsets\n")


def keys(g, m, c):
    """key = mix64(mix64(GOLDEN * (g + 1) ^ m) ^ c) for window strands c = 2p + s of sequence g (uint64 wraparound)"""
    with np.errstate(over="ignore"):
        h = mix64((np.uint64(GOLDEN) * (np.uint64(g) + np.uint64(1))) ^ np.uint64(m))
    return mix64(h ^ np.asarray(c, np.uint64))


def best_sites(seqs, S, both, m, seq0=0):
    """(best int32, site uint64) of motif m (index m, matrix S) on every sequence: the largest (score, key) over the
    scored window strands, an equal key -> the smaller 2p + s; SENTINEL and 0 without a window of A/C/G/T only"""
    S = np.asarray(S, np.int64)
    w = S.shape[0]
    mats = [S, revcomp_S(S)] if both else [S]
    best = np.full(len(seqs), SENTINEL, np.int32)
    site = np.zeros(len(seqs), np.uint64)
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
        b = np.where(ok, c - 1, 0)
        cols = b[starts[:, None] + np.arange(w)[None, :]]
        sc = np.stack([M[np.arange(w)[None, :], cols].sum(axis=1) for M in mats], axis=1)  # (windows, strands)
        cand = 2 * starts[:, None] + np.arange(len(mats))[None, :]
        sc, cand = sc[good].ravel(), cand[good].ravel()
        top = sc.max()
        tied = np.sort(cand[sc == top]).astype(np.uint64)
        k = keys(seq0 + i, m, tied)
        best[i] = top
        site[i] = tied[np.nonzero(k == k.max())[0][0]]  # (sorted: the first of the largest key is the smallest 2p + s)
    return best, site


def considered(lens, w, max_len=MAX_LEN):
    lens = np.asarray(lens, np.int64)
    return int(((lens >= w) & (lens <= max_len)).sum())


def histograms(best, site, lens, w, t, max_len):
    """(hd, hl): offset bins hd[max_len + d], d = 2p + w - L, and length bins hl[L] of the best sites with score >= t on
    the sequences with w <= L <= max_len"""
    lens = np.asarray(lens, np.int64)
    sel = (np.asarray(best, np.int64) >= t) & (lens >= w) & (lens <= max_len)
    p = (np.asarray(site, np.uint64)[sel] >> np.uint64(1)).astype(np.int64)
    d = 2 * p + w - lens[sel]
    hd = np.bincount(d + max_len, minlength=2 * max_len + 1).astype(np.uint64)
    hl = np.bincount(lens[sel], minlength=max_len + 1).astype(np.uint64)
    return hd, hl


def f(L, w, r):
    """the null: the share of window starts p in 0..L-w with |2p + w - L| <= r"""
    D = L - w  # the offsets 2p - D: -D, -D + 2, ..., D
    return (D + 1 if r >= D else r + ((r - D) % 2 == 0)) / (D + 1)


_LF = {}


def _log_factorials(n):
    if n not in _LF:
        _LF.clear()
        _LF[n] = np.array([math.lgamma(k + 1.0) for k in range(n + 1)])
    return _LF[n]


def log10_sf(N, K, p):
    """log10 P(X >= K), X ~ Binomial(N, p), by the terms' log-sum-exp (math.lgamma)"""
    if K == 0 or p >= 1.0:
        return 0.0
    if p <= 0.0:
        return -math.inf
    lf = _log_factorials(N)
    k = np.arange(K, N + 1)
    lt = lf[N] - lf[k] - lf[N - k] + k * math.log(p) + (N - k) * math.log1p(-p)
    mx = lt.max()
    return float((mx + math.log(np.exp(lt - mx).sum())) / math.log(10.0))


def window(hd, hl, max_len, w, r):
    """(K(r), N p(r), log10 P(r)) of one motif, p(r) = (1/N) sum over ascending L of n_L f(L, w, r)"""
    hd = np.asarray(hd, np.int64)
    hl = np.asarray(hl, np.int64)
    N = int(hl.sum())
    K = int(hd[max_len - r:max_len + r + 1].sum())
    s = 0.0
    for L in np.nonzero(hl)[0]:
        s += int(hl[L]) * f(int(L), w, r)
    return K, s, log10_sf(N, K, min(s / N, 1.0)) if s > 0.0 else 0.0


def summary(hd, hl, max_len, w, M):
    """the test of one motif, as pengk_centrality_summary returns it: the r in 0..Dm with p(r) > 0 and the smallest
    log10 P(r), the smaller r on ties"""
    hl = np.asarray(hl, np.int64)
    N = int(hl.sum())
    out = dict(sites=N, max_offset=0, window=0, in_window=0, expected=0.0, log10_pvalue=0.0, log10_evalue=0.0)
    if N == 0:
        return out
    Dm = int(np.nonzero(hl)[0].max()) - w
    best = None
    for r in range(Dm + 1):
        K, e, lp = window(hd, hl, max_len, w, r)
        if e > 0.0 and (best is None or lp < best[0]):
            best = (lp, r, K, e)
    lp, r, K, e = best
    out.update(max_offset=Dm, window=r, in_window=K, expected=e, log10_pvalue=lp,
               log10_evalue=lp + math.log10(Dm + 1) + math.log10(M))
    return out


def center_distance(r):
    return "%d" % (r // 2) if r % 2 == 0 else "%d.5" % (r // 2)


def line(index, motif_id, w, sequences, hd, max_len, sm):
    """one TSV line (without the newline) from a summary"""
    head = "%d\t%s\t%d\t%d\t%d" % (index, motif_id, w, sequences, sm["sites"])
    if sm["sites"] == 0:
        return head + "\tNA" * 7
    Dm, r = sm["max_offset"], sm["window"]
    offs = ",".join(str(int(x)) for x in np.asarray(hd)[max_len - Dm:max_len + Dm + 1])
    return head + "\t%s\t%d\t%.2f\t%.3f\t%.3f\t%.3f\t%s" % (center_distance(r), sm["in_window"], sm["expected"],
                                                            sm["in_window"] / sm["expected"], sm["log10_pvalue"],
                                                            sm["log10_evalue"], offs)


def render(seqs, motif_ids, Ss, ts, both, max_len=None):
    """the --centrality TSV (str) of motifs Ss (MEME order) with thresholds ts over seqs (byte codes)"""
    lens = np.array([len(c) for c in seqs], np.int64)
    if max_len is None:
        ok = lens[lens <= MAX_LEN]
        max_len = max(int(ok.max()) if len(ok) else 1, 1)
    out = [HEADER]
    for m, (S, t) in enumerate(zip(Ss, ts)):
        w = len(S)
        b, s = best_sites(seqs, S, both, m)
        hd, hl = histograms(b, s, lens, w, t, max_len)
        sm = summary(hd, hl, max_len, w, len(Ss))
        out.append(line(m + 1, motif_ids[m], w, considered(lens, w), hd, max_len, sm) + "\n")
    return "".join(out)
