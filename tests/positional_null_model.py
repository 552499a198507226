"""numpy restatement of --positional-null composition (include/pengk.h, "the composition null of the positional report";
INTEGRATION.md 7t) beside motif_positional_model, which it imports and leaves as it is.  This project's own definitions: the
pair table is integer, so the device must agree bit for bit; the summary is fp64 in one stated order, so the library must
agree bit for bit as well.  The numbers are NOT promised to be RSAT's.

pair table  pairs[b, 4x + y] (n_bins x 16 uint64): every position p at which a word stands (K consecutive valid bases from p
            on -- all standing words, not only clump heads) with b = coordinate(p) // bin_size < n_bins adds 1 at x = s[p],
            y = s[p+1] and, on both strands, 1 more at x = 3 - s[p+K-1], y = 3 - s[p+K-2]
shares      n1[b][x] = sum_y pairs[b, 4x + y];  T_b[x][y] = (pairs + 1) / (n1[b][x] + 4);  f_b[x] = n1[b][x] / sum_x n1[b][x];
            P_b(w) = f_b[w_0] * T_b[w_0][w_1] * .. left to right; on both strands P_b(key) + P_b(rc(key)); a bin without a
            pair: 0;  g_b = N[b] * P_b(key);  G = sum_b g_b, b ascending;  q_key[b] = g_b / G;  G = 0: the key is skipped
test        as motif_positional_model.summary with q_key[b] in place of q[b]"""
import math

import numpy as np

import motif_positional_model as mp

COLUMNS = mp.COLUMNS[:7] + ["flat_expected"] + mp.COLUMNS[7:]


# ---- the pair table ------------------------------------------------------------------------------------------------------
def pair_tables(seqs, K, anchor, bin_size, n_bins, both, weights=None):
    """pairs (n_bins x 16 uint64) of the sequences; weights: how many times each one counts.  Laid end to end with one
    invalid base between them, as mp.tables lays them."""
    assert mp.MIN_K <= K <= mp.MAX_K and anchor in (0, 1, 2) and 1 <= bin_size <= mp.MAX_BIN_SIZE and 1 <= n_bins <= mp.MAX_BINS
    pairs = np.zeros((n_bins, 16), np.uint64)
    parts, wts, starts, lens = [], [], [], []
    at = 0
    for i, c in enumerate(seqs):
        c = np.asarray(c, np.uint8)
        parts += [c, np.zeros(1, np.uint8)]
        n1 = len(c) + 1
        wts.append(np.full(n1, 1 if weights is None else int(weights[i]), np.int64))
        starts.append(np.full(n1, at, np.int64))
        lens.append(np.full(n1, len(c), np.int64))
        at += n1
    if not parts:
        return pairs
    c = np.concatenate(parts)
    w, start, L = np.concatenate(wts), np.concatenate(starts), np.concatenate(lens)
    n = len(c)
    v = (c >= 1) & (c <= 4)
    s = np.zeros(n + K, np.int64)
    s[:n] = np.where(v, c.astype(np.int64) - 1, 0)
    pos = np.arange(n)
    nxt = np.minimum.accumulate(np.where(v, n, pos)[::-1])[::-1]  # the first invalid base at or behind p
    stands = (nxt - pos) >= K
    b = mp.coordinate(anchor, pos - start, L, K) // bin_size
    on = stands & (b < n_bins)
    fwd = 4 * s[0:n] + s[1:n + 1]
    flat = np.bincount(b[on] * 16 + fwd[on], weights=w[on], minlength=n_bins * 16)  # (exact: far below 2^53)
    if both:
        rev = 4 * (3 - s[K - 1:K - 1 + n]) + (3 - s[K - 2:K - 2 + n])
        flat = flat + np.bincount(b[on] * 16 + rev[on], weights=w[on], minlength=n_bins * 16)
    pairs += flat.astype(np.uint64).reshape(n_bins, 16)
    return pairs


def pair_tables_literal(codes, K, anchor, bin_size, n_bins, both):
    """(pairs, standing words per bin): the definition read position by position, for one sequence"""
    c = [int(x) for x in codes]
    L = len(c)
    pairs = np.zeros((n_bins, 16), np.uint64)
    standing = np.zeros(n_bins, np.int64)
    for p in range(L - K + 1):
        if not all(1 <= x <= 4 for x in c[p:p + K]):
            continue
        cc = p if anchor == mp.START else L - K - p if anchor == mp.END else abs(2 * p + K - L) >> 1
        b = cc // bin_size
        if b >= n_bins:
            continue
        standing[b] += 1
        pairs[b, 4 * (c[p] - 1) + (c[p + 1] - 1)] += 1
        if both:
            pairs[b, 4 * (3 - (c[p + K - 1] - 1)) + (3 - (c[p + K - 2] - 1))] += 1
    return pairs, standing


# ---- the summary ---------------------------------------------------------------------------------------------------------
def chains(pairs):
    """per bin (f, T) or None: f[x] and T[x][y] as Python floats"""
    out = []
    for row in np.asarray(pairs, np.uint64):
        c = [[int(row[4 * x + y]) for y in range(4)] for x in range(4)]
        n1 = [sum(c[x]) for x in range(4)]
        total = sum(n1)
        if total == 0:
            out.append(None)
            continue
        f = [float(n1[x]) / float(total) for x in range(4)]
        T = [[float(c[x][y] + 1) / float(n1[x] + 4) for y in range(4)] for x in range(4)]
        out.append((f, T))
    return out


def word_probability(chain, key, K):
    f, T = chain
    w = mp.columns(key, K)
    P = f[w[0]]
    for i in range(K - 1):
        P *= T[w[i]][w[i + 1]]
    return P


def shares(counts, pairs, K, both, key, ch=None):
    """q_key[b] as a list of floats, or None where G = 0"""
    counts = np.asarray(counts, np.uint64)
    ch = chains(pairs) if ch is None else ch
    g, G = [], 0.0
    for b in range(counts.shape[0]):
        P = 0.0
        if ch[b] is not None:
            P = word_probability(ch[b], key, K)
            if both:
                P = P + word_probability(ch[b], int(mp.revcomp(key, K)), K)
        g.append(float(int(counts[b].sum())) * P)
        G += g[-1]
    if G == 0.0:
        return None
    return [x / G for x in g]


def summary(counts, pairs, K, both, sf, min_count=5, max_evalue=0.01):
    """mp.summary under the composition null: the same fields, in the same order"""
    counts = np.asarray(counts, np.uint64)
    B = counts.shape[0]
    N = [int(x) for x in counts.sum(axis=1)]
    Cs = counts.sum(axis=0)
    if sum(N) == 0:
        return []
    ch = chains(pairs)
    log_tests = math.log10(float(B * mp.n_keys(K, both)))
    log_max = math.log10(max_evalue)
    rep = []
    for key in np.flatnonzero(Cs).tolist():
        C = int(Cs[key])
        q = shares(counts, pairs, K, both, key, ch)
        if q is None:
            continue
        best, significant = None, 0
        for b in range(B):
            c = int(counts[b, key])
            if c == 0 or c < min_count:
                continue
            expected = float(C) * q[b]
            if not float(c) > expected:
                continue
            lp = sf(C, c, q[b])
            le = lp + log_tests
            if le <= log_max:
                significant += 1
            if best is None or le < best["log10_evalue"]:
                best = dict(key=key, bin=b, count=c, total=C, bin_positions=N[b], expected=expected, log10_pvalue=lp, log10_evalue=le)
        if best is None or not best["log10_evalue"] <= log_max:
            continue
        best.update(bins_significant=significant, family=0, is_head=0)
        rep.append(best)
    rep.sort(key=lambda d: (d["log10_evalue"], d["bin"], d["key"]))
    heads = []
    for k, d in enumerate(rep):
        Y = [mp.columns(d["key"], K)] + ([mp.columns(d["key"], K, True)] if both else [])
        for h in heads:
            if abs(rep[h]["bin"] - d["bin"]) > 1:
                continue
            X = mp.columns(rep[h]["key"], K)
            if any(mp.related(X, y) for y in Y):
                d["family"] = h + 1
                break
        else:
            heads.append(k)
            d["family"], d["is_head"] = k + 1, 1
    return rep


def render_tsv(rep, counts, K):
    """the TSV of the CLI under the composition null: mp.render_tsv with flat_expected = total * (bin_positions / counted
    words) behind expected"""
    counted = int(np.asarray(counts, np.uint64).sum())
    out = ["\t".join(COLUMNS)]
    for k, d in enumerate(rep):
        out.append("%d\t%s\t%d\t%d\t%d\t%d\t%.2f\t%.2f\t%.3f\t%.3f\t%.3f\t%d\t%d\t%d\t%s"
                   % (k + 1, mp.word_string(d["key"], K), d["bin"], d["count"], d["total"], d["bin_positions"], d["expected"],
                      float(d["total"]) * (float(d["bin_positions"]) / float(counted)), d["count"] / d["expected"], d["log10_pvalue"],
                      d["log10_evalue"], d["bins_significant"], d["family"], d["is_head"], ",".join(str(int(x)) for x in counts[:, d["key"]])))
    return "\n".join(out) + "\n"


# ---- inputs --------------------------------------------------------------------------------------------------------------
def gradient(seed, frac=0.0, n=2000, motif="TGACTCA"):
    """n sequences of 200 bases whose G+C share falls linearly from 65 % at the centre to 35 % at both ends, every base drawn
    independently; `motif` laid on the plus strand of a share `frac` of them at the centre +- 3 (the place is drawn only where
    it is laid; frac = 0: nothing is laid)"""
    rng = np.random.default_rng(seed)
    x = np.abs(np.arange(200) - 99.5) / 99.5
    gc = 0.65 - 0.30 * x
    w = np.array([mp.LETTERS.index(a) for a in motif])
    out = []
    for _ in range(n):
        u = rng.random(200)
        v = rng.random(200) < 0.5
        s = np.where(u < gc, np.where(v, 1, 2), np.where(v, 0, 3))   # C or G where u < gc, else A or T; A or C where v
        lay = rng.random() < frac
        if lay:
            p = 100 - 3 + rng.integers(-3, 4)
            s[p:p + len(w)] = w
        out.append((s + 1).astype(np.uint8))
    return out


def ramp(seed, n=2000):
    """n sequences of 200 bases whose G+C share rises linearly from 35 % at the start to 65 % at the end"""
    rng = np.random.default_rng(seed)
    gc = 0.35 + 0.30 * np.arange(200) / 199.0
    out = []
    for _ in range(n):
        u = rng.random(200)
        v = rng.random(200) < 0.5
        out.append((np.where(u < gc, np.where(v, 1, 2), np.where(v, 0, 3)) + 1).astype(np.uint8))
    return out


def gc_letters(key, K):
    """how many of the word's letters are C or G"""
    return sum(1 for x in mp.columns(key, K) if x in (1, 2))


def shares_a_4mer(word, motif="TGACTCA"):
    rc = "".join("ACGT"[3 - "ACGT".index(a)] for a in reversed(motif))
    four = {m[i:i + 4] for m in (motif, rc) for i in range(len(m) - 3)}
    return any(word[i:i + 4] in four for i in range(len(word) - 3))
