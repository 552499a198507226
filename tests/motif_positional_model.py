"""numpy restatement of --positional (include/pengk.h, "positional words"): words of K = 4..7 letters
counted per position bin, overlapping repeats of a word once.  This project's own definitions, integer up to the summary,
so the device must agree with the table bit for bit.  The numbers are NOT promised to be those of RSAT's position-analysis.

Per sequence, letters s[0..L) in 0..3 and validity bits v; r[p] = the consecutive valid bases from p on:
  word        stands at p iff r[p] >= K; value = sum s[p+i] 4^(K-1-i); key = value, on both strands min(value, rc(value))
  clump head  counted iff no word with the same key stands at any of p-1 .. p-(K-1)
  coordinate  anchor 0: c = p;  1: c = L - K - p;  2: c = |2p + K - L| >> 1
  bin         b = c // bin_size, counted iff b < n_bins;  counts[b, key] += 1

tables    the table of a set of sequences (byte codes, 0 = other, A,C,G,T = 1..4)
summary   the report: candidates, binomial tail (the library's own: `sf`), E-value, best bin, order, families"""
import math

import numpy as np

MIN_K, MAX_K = 4, 7
MAX_BINS = 64
MAX_BIN_SIZE = 65536
START, END, CENTER = 0, 1, 2
LETTERS = "ACGT"
COLUMNS = ("rank word bin count total bin_positions expected enrichment log10_pvalue log10_evalue bins_significant family is_head "
           "profile").split()


def codes_of(s):
    return np.array(["NACGT".index(x) for x in s], np.uint8)


def key_of(word):
    v = 0
    for x in word:
        v = 4 * v + LETTERS.index(x)
    return v


def word_string(key, K):
    return "".join(LETTERS[(key >> (2 * (K - 1 - c))) & 3] for c in range(K))


def revcomp(v, K):
    """the reverse complement of a value or an array of values of K digits"""
    v = np.asarray(v, np.int64)
    out = np.zeros_like(v)
    for _ in range(K):
        out = 4 * out + (3 - (v & 3))
        v = v >> 2
    return out


def canonical(key, K):
    return min(int(key), int(revcomp(key, K)))


def n_keys(K, both):
    if not both:
        return 4 ** K
    return 4 ** K // 2 if K % 2 else (4 ** K + 4 ** (K // 2)) // 2


def coordinate(anchor, p, L, K):
    if anchor == START:
        return p
    if anchor == END:
        return L - K - p
    return np.abs(2 * p + K - L) >> 1


# ---- the table -----------------------------------------------------------------------------------------------------------
def tables(seqs, K, anchor, bin_size, n_bins, both, weights=None):
    """counts (n_bins x 4^K uint64) of the sequences; weights: how many times each one counts.  The sequences are laid end
    to end with one invalid base between them, which cuts every word as a sequence's end does."""
    assert MIN_K <= K <= MAX_K and anchor in (0, 1, 2) and 1 <= bin_size <= MAX_BIN_SIZE and 1 <= n_bins <= MAX_BINS
    NK = 4 ** K
    counts = np.zeros((n_bins, NK), np.uint64)
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
        return counts
    c = np.concatenate(parts)
    w, start, L = np.concatenate(wts), np.concatenate(starts), np.concatenate(lens)
    n = len(c)
    v = (c >= 1) & (c <= 4)
    s = np.zeros(n + K, np.int64)
    s[:n] = np.where(v, c.astype(np.int64) - 1, 0)
    pos = np.arange(n)
    nxt = np.minimum.accumulate(np.where(v, n, pos)[::-1])[::-1]  # the first invalid base at or behind p
    stands = (nxt - pos) >= K
    value = np.zeros(n, np.int64)
    for i in range(K):
        value = 4 * value + s[i:i + n]
    key = np.minimum(value, revcomp(value, K)) if both else value
    head = stands.copy()
    for d in range(1, K):
        same = np.zeros(n, bool)
        same[d:] = stands[:-d] & (key[:-d] == key[d:])
        head &= ~same
    p = pos - start
    cc = coordinate(anchor, p, L, K)
    b = cc // bin_size
    on = head & (b < n_bins)
    flat = np.bincount(b[on] * NK + key[on], weights=w[on], minlength=n_bins * NK)  # (exact: far below 2^53)
    counts += flat.astype(np.uint64).reshape(n_bins, NK)
    return counts


def tables_literal(codes, K, anchor, bin_size, n_bins, both):
    """the definition read position by position, for one sequence"""
    c = np.asarray(codes, np.uint8)
    L = len(c)
    counts = np.zeros((n_bins, 4 ** K), np.uint64)
    ok = [1 <= x <= 4 for x in c]

    def key_at(p):
        """the key of the word standing at p, or None"""
        if p < 0 or p + K > L or not all(ok[p:p + K]):
            return None
        val = 0
        for i in range(K):
            val = 4 * val + int(c[p + i]) - 1
        return canonical(val, K) if both else val

    for p in range(L):
        k = key_at(p)
        if k is None or any(key_at(p - d) == k for d in range(1, K)):
            continue
        cc = p if anchor == START else L - K - p if anchor == END else abs(2 * p + K - L) >> 1
        if cc // bin_size < n_bins:
            counts[cc // bin_size, k] += 1
    return counts


# ---- the summary ---------------------------------------------------------------------------------------------------------
def columns(key, K, rc=False):
    if rc:
        key = int(revcomp(key, K))
    return [(key >> (2 * (K - 1 - c))) & 3 for c in range(K)]


def related(X, Y):
    """Y laid on X at some offset in -2 .. 2: no clashing column and at least 4 equal ones"""
    for o in range(-2, 3):
        same, clash = 0, False
        for c in range(len(X)):
            cy = c - o
            if cy < 0 or cy >= len(Y):
                continue
            if X[c] == Y[cy]:
                same += 1
            else:
                clash = True
        if not clash and same >= 4:
            return True
    return False


def summary(counts, K, both, sf, min_count=5, max_evalue=0.01):
    """the report as a list of dicts, in order; sf(n, k, p) = log10 P(X >= k), X ~ Binomial(n, p)"""
    counts = np.asarray(counts, np.uint64)
    B = counts.shape[0]
    N = [int(x) for x in counts.sum(axis=1)]
    Cs = counts.sum(axis=0)
    Nt = sum(N)
    if Nt == 0:
        return []
    q = [float(N[b]) / float(Nt) for b in range(B)]
    log_tests = math.log10(float(B * n_keys(K, both)))
    log_max = math.log10(max_evalue)
    rep = []
    for key in np.flatnonzero(Cs).tolist():
        C = int(Cs[key])
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
        Y = [columns(d["key"], K)] + ([columns(d["key"], K, True)] if both else [])
        for h in heads:
            if abs(rep[h]["bin"] - d["bin"]) > 1:
                continue
            X = columns(rep[h]["key"], K)
            if any(related(X, y) for y in Y):
                d["family"] = h + 1
                break
        else:
            heads.append(k)
            d["family"], d["is_head"] = k + 1, 1
    return rep


def render_tsv(rep, counts, K):
    """the TSV of the CLI: numbers as --dyads formats its, and the key's counts per bin"""
    out = ["\t".join(COLUMNS)]
    for k, d in enumerate(rep):
        out.append("%d\t%s\t%d\t%d\t%d\t%d\t%.2f\t%.3f\t%.3f\t%.3f\t%d\t%d\t%d\t%s"
                   % (k + 1, word_string(d["key"], K), d["bin"], d["count"], d["total"], d["bin_positions"], d["expected"],
                      d["count"] / d["expected"], d["log10_pvalue"], d["log10_evalue"], d["bins_significant"], d["family"], d["is_head"],
                      ",".join(str(int(x)) for x in counts[:, d["key"]])))
    return "\n".join(out) + "\n"


def period(word):
    """the smallest shift under which the word overlaps itself letter for letter"""
    return next(t for t in range(1, len(word) + 1) if word[t:] == word[:-t] or t == len(word))


# ---- inputs --------------------------------------------------------------------------------------------------------------
IUPAC = {"A": "A", "C": "C", "G": "G", "T": "T", "W": "AT", "R": "AG"}


def planted(seed, frac=0.1, n=2000, L=200, at=0.7, motif="TATAWAWR", where=60, jitter=2):
    """the scenario of the README's table: n sequences of L bases at an A+T share `at`, `motif` laid on the plus strand of a
    share `frac` of them at `where` +- `jitter` (frac = 0: the draws are made all the same, nothing is laid)"""
    rng = np.random.default_rng(seed)
    p4 = [at / 2, (1 - at) / 2, (1 - at) / 2, at / 2]
    out = []
    for _ in range(n):
        s = rng.choice(4, L, p=p4)
        lay = rng.random() < frac
        w = np.array([LETTERS.index(IUPAC[x][rng.integers(0, len(IUPAC[x]))]) for x in motif])
        p = where + rng.integers(-jitter, jitter + 1)
        if lay:
            s[p:p + len(w)] = w
        out.append((s + 1).astype(np.uint8))
    return out


def fasta_text(seqs):
    return "".join(">s%d\n%s\n" % (i, "".join("NACGT"[x] for x in c)) for i, c in enumerate(seqs))


def edge_lengths(K, S, B):
    return sorted(set(list(range(K + 2)) + [63, 64, 65, 64 + K - 1, 64 + K, S * B - 1, S * B, S * B + K, 126, 127, 128, 129]))


def random_sequences(seed, lengths, skew=False):
    """letters of the given lengths: uniform, or (skew) two letters only, so that words repeat and overlap themselves"""
    rng = np.random.default_rng(seed)
    if skew:
        return [(rng.choice(4, int(L), p=[0.48, 0.02, 0.02, 0.48]) + 1).astype(np.uint8) for L in lengths]
    return [rng.integers(1, 5, int(L)).astype(np.uint8) for L in lengths]


def many_sequences(n=100000, pool=2000, seed=8):
    """(sequences, index into the pool, the pool): n sequences of 0 .. 300 bases drawn from a pool of distinct ones, skewed
    compositions and invalid bases, so that the model runs over the pool with multiplicities"""
    rng = np.random.default_rng(seed)
    P = []
    for k in range(pool):
        L = k % 301
        c = (rng.choice(4, L, p=rng.dirichlet(np.full(4, 0.7))) + 1).astype(np.uint8)
        if k % 3 == 0 and L:
            c[rng.integers(0, L, 1 + k % 4)] = 0
        P.append(c)
    idx = rng.integers(0, pool, n)
    idx[:pool] = np.arange(pool)
    return [P[i] for i in idx], idx, P
