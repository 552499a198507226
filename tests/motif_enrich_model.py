"""numpy restatement of the database enrichment (--enrich; include/pengk.h, "database enrichment"): the
log-odds of a database motif, the best score per sequence, the two histograms and the scored counts of
pengk_motif_enrich, Fisher's one-sided tail (exact in Python integers where that is feasible, in log space beyond), the
summary over the thresholds, the Benjamini-Hochberg step and the TSV the CLI writes.  Up to the histograms everything is
integer, so the device must agree with it bit for bit."""
import decimal
import math

import numpy as np

import motif_score_model as ms
import motif_sites_model as mst

HEADER = ("rank\tmotif_id\talt_id\twidth\tthreshold\tthreshold_pvalue\tpos_hits\tpos_scored\tneg_hits\tneg_scored\tenrichment\t"
          "log10_pvalue\tlog10_adj_pvalue\tlog10_evalue\tq_value\n")
SENTINEL = ms.SENTINEL


# ---- log-odds of a database motif ------------------------------------------------------------------------------------------
def db_log_odds(rows, bg0):
    """row r -> p_a = (r_a / sum(r) + 0.01 bg0_a) / 1.01 in double (sum = ((r_0 + r_1) + r_2) + r_3), rounded to float32,
    then motif_score_model.log_odds against bg0"""
    r = np.asarray(rows, np.float64)
    b = np.asarray(bg0, np.float32).astype(np.float64)
    s = ((r[:, 0] + r[:, 1]) + r[:, 2]) + r[:, 3]
    p = (r / s[:, None] + 0.01 * b[None, :]) / 1.01
    return ms.log_odds(p.astype(np.float32), bg0)


# ---- best scores, histograms, scored counts -----------------------------------------------------------------------------
class Packed:
    """the sequences of a set side by side (byte codes 1..4 = A,C,G,T, else invalid), 64 invalid positions behind them:
    what best_scores needs of them, built once for every motif.  kmer[p]: the four bases from p on, base k in bits 2k,
    2k + 1; run[p]: the valid bases from p on before the first invalid one or the end of p's sequence"""

    def __init__(self, seqs):
        self.lens = np.array([len(s) for s in seqs], np.int64)
        self.starts = np.concatenate([[0], np.cumsum(self.lens)])[:-1].astype(np.int64)
        self.n = n = int(self.lens.sum())
        c = np.concatenate([np.asarray(s, np.int64) for s in seqs] + [np.zeros(64 + 4, np.int64)])
        ok = (c >= 1) & (c <= 4)
        b = np.where(ok, c - 1, 0)
        m = len(c) - 3
        self.kmer = (b[0:m] | (b[1:m + 1] << 2) | (b[2:m + 2] << 4) | (b[3:m + 3] << 6)).astype(np.uint8)
        nxt = np.where(~ok[:n], np.arange(n), n)
        nxt = np.minimum.accumulate(nxt[::-1])[::-1]  # the next invalid base at or behind p
        ends = np.repeat(self.starts + self.lens, self.lens)  # the end of p's sequence
        self.run = (np.minimum(nxt, ends) - np.arange(n)).astype(np.int32)


def chunk_tables(S):
    """T[c][idx]: the sum of columns 4c .. 4c+3 of S (those below the width) over the four bases of idx, base k in bits
    2k, 2k+1"""
    S = np.asarray(S, np.int32)
    w = len(S)
    idx = np.arange(256)
    T = np.zeros(((w + 3) // 4, 256), np.int32)
    for j in range(w):
        T[j // 4] += S[j][(idx >> (2 * (j % 4))) & 3]
    return T


def best_scores(packed, S, both):
    """best window-strand score of every sequence of `packed` (SENTINEL without a window of valid bases): what
    motif_score_model.best_scores gives, for all sequences at once"""
    S = np.asarray(S, np.int32)
    w = len(S)
    n = packed.n
    out = np.full(len(packed.lens), SENTINEL, np.int64)
    if n == 0:
        return out
    sc = None
    for M in ([S, ms.revcomp_S(S)] if both else [S]):
        T = chunk_tables(M)
        s = T[0].take(packed.kmer[0:n])
        for c in range(1, len(T)):
            s += T[c].take(packed.kmer[4 * c:4 * c + n])
        sc = s if sc is None else np.maximum(sc, s)
    sc = np.where(packed.run >= w, sc, np.int32(SENTINEL))  # a window is one: inside its sequence and of valid bases only
    has = packed.lens > 0
    out[has] = np.maximum.reduceat(sc, packed.starts[has])
    return out


def score_hi(S):
    return int(np.asarray(S, np.int64).max(axis=1).sum())


def histogram(best, thr, hi):
    """(hist, scored): hist[k] the sequences with best score thr + k (max(0, hi - thr + 1) bins), scored those with a
    window at all"""
    best = np.asarray(best, np.int64)
    had = best != SENTINEL
    nb = max(0, hi - thr + 1)
    b = best[had & (best >= thr)] - thr
    assert nb > 0 or len(b) == 0
    return np.bincount(b, minlength=nb).astype(np.uint64)[:nb], int(had.sum())


# ---- Fisher's one-sided tail ------------------------------------------------------------------------------------------------
def support(N, K, n):
    return max(0, n + K - N), min(K, n)


def falling(a, k):
    out = 1
    for i in range(k):
        out *= a - i
    return out


def exact_tail(N, K, n, k):
    """P(X >= k) for X ~ Hypergeometric(N, K marked, n drawn) as (numerator, denominator), Python integers: C(K, x)
    C(N - K, n - x) / C(N, n) for N <= 2e5, else (K <= 2000) the same ratio as C(K, x) [n]_x [N - n]_{K - x} / [N]_K; the
    terms follow from the first by their ratio (K - x)(n - x) / ((x + 1)(N - K - n + x + 1)), an exact division"""
    lo, hi = support(N, K, n)
    if N <= 200000:
        t, den = math.comb(K, lo) * math.comb(N - K, n - lo), math.comb(N, n)
    else:
        assert K <= 2000
        t, den = math.comb(K, lo) * falling(n, lo) * falling(N - n, K - lo), falling(N, K)
    up = 0
    for x in range(lo, hi + 1):
        if x >= k:
            up += t
        if x < hi:
            t = t * (K - x) * (n - x) // ((x + 1) * (N - K - n + x + 1))
    return up, den


def exact_log10_sf(N, K, n, k):
    lo, hi = support(N, K, n)
    if k <= lo:
        return 0.0
    if k > hi:
        return -math.inf
    up, den = exact_tail(N, K, n, k)
    return math.log10(up) - math.log10(den)  # (math.log10 takes integers of any size)


_CTX = decimal.Context(prec=50)
_PI = decimal.Decimal("3.14159265358979323846264338327950288419716939937511")
_STIRLING = [(1, 12), (-1, 360), (1, 1260), (-1, 1680), (1, 1188), (-691, 360360), (1, 156)]


def _ln_factorial(n):
    """ln n! to 50 digits: the integer below 40, Stirling's series from there on (its first omitted term is below 1e-26)"""
    D = decimal.Decimal
    if n < 40:
        return _CTX.ln(D(math.factorial(n)))
    x = D(n)
    s = (x + D("0.5")) * _CTX.ln(x) - x + _CTX.ln(2 * _PI) / 2
    for j, (a, b) in enumerate(_STIRLING):
        s += D(a) / (D(b) * x ** (2 * j + 1))
    return s


def _ln_pmf(N, K, n, x):
    """ln P(X = x): from math.lgamma up to N = 1e5 (nine terms of at most 1.1e6, each to 1e-16 relative: 1e-9 absolute at
    the worst, far less at the sizes of the tests), from 50-digit logarithms beyond"""
    if N <= 100000:
        def lf(v):
            return math.lgamma(v + 1.0)
        return (lf(K) - lf(x) - lf(K - x)) + (lf(N - K) - lf(n - x) - lf(N - K - n + x)) - (lf(N) - lf(n) - lf(N - n))
    with decimal.localcontext(_CTX):
        lf = _ln_factorial
        v = (lf(K) - lf(x) - lf(K - x)) + (lf(N - K) - lf(n - x) - lf(N - K - n + x)) - (lf(N) - lf(n) - lf(N - n))
        return float(v)


def log10_sf(N, K, n, k):
    """log10 P(X >= k) in log space, for any size: the point mass at the end of the shorter tail, then the sum of the terms
    relative to it, by their ratio P(x + 1) / P(x) = (K - x)(n - x) / ((x + 1)(N - K - n + x + 1)) away from the mode --
    upwards from k, or downwards from k - 1 and the complement.  The terms fall at least geometrically (the point masses
    are log-concave) and faster than a normal tail's: beyond 60 standard deviations + 200 steps nothing is left of them."""
    lo, hi = support(N, K, n)
    if k <= lo:
        return 0.0
    if k > hi:
        return -math.inf
    reach = int(60.0 * math.sqrt(n * (K / N) * ((N - K) / N) * ((N - n) / max(N - 1, 1)))) + 200

    def up(x):
        x = np.asarray(x, np.float64)
        return (K - x) * (n - x) / ((x + 1.0) * (N - K - n + x + 1.0))
    if float(up(k)) <= 1.0:
        x = np.arange(k, min(hi, k + reach))
        total = 1.0 + float(np.cumprod(up(x)).sum())
        return (_ln_pmf(N, K, n, k) + math.log(total)) / math.log(10.0)
    x = np.arange(k - 1, max(lo, k - 1 - reach), -1)
    total = 1.0 + float(np.cumprod(1.0 / up(x - 1)).sum())
    lower = math.exp(_ln_pmf(N, K, n, k - 1) + math.log(total))
    return math.log1p(-lower) / math.log(10.0)


# ---- the summary over the thresholds ---------------------------------------------------------------------------------------
def tried(h_pos, h_neg):
    """[(k, a, b)] from the top bin down, for the bins with a count in either histogram"""
    out, a, b = [], 0, 0
    for k in range(len(h_pos) - 1, -1, -1):
        a += int(h_pos[k])
        b += int(h_neg[k])
        if int(h_pos[k]) + int(h_neg[k]) > 0:
            out.append((k, a, b))
    return out


def log10_p_at(h_pos, h_neg, k, n_pos, n_neg):
    a, b = sum(int(x) for x in h_pos[k:]), sum(int(x) for x in h_neg[k:])
    return log10_sf(n_pos + n_neg, a + b, n_pos, a)


def enrichment(a, b, n_pos, n_neg):
    return ((a + 1.0) / (n_pos + 1.0)) / ((b + 1.0) / (n_neg + 1.0))


def summary(h_pos, h_neg, thr, n_pos, n_neg):
    """pengk_enrich_summary: a dict with the fields of pengk_enrichment"""
    tr = tried(h_pos, h_neg)
    out = dict(threshold=thr + len(h_pos), n_thresholds=len(tr), pos_hits=0, neg_hits=0, log10_pvalue=0.0, log10_adj_pvalue=0.0)
    best = None
    for k, a, b in tr:  # (from the top down: the higher threshold wins a tie)
        lp = log10_sf(n_pos + n_neg, a + b, n_pos, a)
        if best is None or lp < best:
            best = lp
            out.update(threshold=thr + k, pos_hits=a, neg_hits=b, log10_pvalue=lp)
    if tr:
        out["log10_adj_pvalue"] = min(0.0, out["log10_pvalue"] + math.log10(len(tr)))
    out["enrichment"] = enrichment(out["pos_hits"], out["neg_hits"], n_pos, n_neg)
    return out


# ---- the database: order, E-values, q-values, the file -----------------------------------------------------------------------
def order_of(summaries):
    """database indices by log10_adj_pvalue, then log10_pvalue, then database order"""
    return sorted(range(len(summaries)), key=lambda m: (summaries[m]["log10_adj_pvalue"], summaries[m]["log10_pvalue"], m))


def log10_qvalues(summaries, order):
    """Benjamini-Hochberg over the database's adjusted p-values, in log10, by rank in `order`: from the last rank down a
    running minimum (from 0) of log10_adj + log10(n_db) - log10(rank)"""
    n = len(order)
    lq, mn = [0.0] * n, 0.0
    for k in range(n - 1, -1, -1):
        mn = min(mn, summaries[order[k]]["log10_adj_pvalue"] + math.log10(n) - math.log10(k + 1))
        lq[k] = mn
    return lq


def analyse(pos, neg, rows, bg0, P, both):
    """per database motif (rows: its matrix as read): (S, lo, tail, thr, hi, h_pos, n_pos, h_neg, n_neg, summary); pos /
    neg: Packed sets"""
    out = []
    for r in rows:
        S = db_log_odds(r, bg0)
        lo, tail = mst.tail_pvalues(S, bg0)
        thr, hi = mst.threshold(lo, tail, P), score_hi(S)
        hp, n_pos = histogram(best_scores(pos, S, both), thr, hi)
        hn, n_neg = histogram(best_scores(neg, S, both), thr, hi)
        out.append(dict(S=S, lo=lo, tail=tail, thr=thr, hi=hi, h_pos=hp, n_pos=n_pos, h_neg=hn, n_neg=n_neg,
                        summary=summary(hp, hn, thr, n_pos, n_neg)))
    return out


def render(names, alts, results, E=10.0):
    """the --enrich TSV (str) from analyse()'s results"""
    sums = [r["summary"] for r in results]
    order = order_of(sums)
    lq = log10_qvalues(sums, order)
    n = len(results)
    lines = [HEADER]
    for k, m in enumerate(order):
        r, s = results[m], sums[m]
        le = s["log10_adj_pvalue"] + math.log10(n)
        if not le <= math.log10(E):
            continue
        t = s["threshold"]
        tp = r["tail"][t - r["lo"]] if t <= r["hi"] else 0.0
        lines.append("%d\t%s\t%s\t%d\t%s\t%.3g\t%d\t%d\t%d\t%d\t%.3f\t%.3f\t%.3f\t%.3f\t%.3g\n" % (
            k + 1, names[m], alts[m] or ".", len(r["S"]), mst.fmt_score(t), tp, s["pos_hits"], r["n_pos"], s["neg_hits"], r["n_neg"],
            s["enrichment"], s["log10_pvalue"], s["log10_adj_pvalue"], le, 10.0 ** lq[k] if lq[k] > -320 else 0.0))
    return "".join(lines)
