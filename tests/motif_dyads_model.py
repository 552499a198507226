"""numpy restatement of --dyads (include/pengk.h, "spaced dyads"): pairs of trinucleotides a fixed number
of unconstrained bases apart.  This project's own definitions, integer up to the summary, so the device must agree with
the tables bit for bit.  The numbers are NOT promised to be those of RSAT's dyad-analysis.

Per sequence, letters s[0..L) in 0..3 and validity bits v; r[p] = the consecutive valid bases from p on:
  triplet     stands at p iff r[p] >= 3; t[p] = 16 s[p] + 4 s[p+1] + s[p+2]; adds 1 to mono[t[p]]
  occurrence  for every p and g in 0..G with r[p] >= 6 + g: the dyad (a, g, b), a = t[p], b = t[p+3+g], key = 64 a + b
  strands     on both strands key = min(key, 64 rc(b) + rc(a))
  count       counts[g, key] += 1

tables    the two tables of a set of sequences (byte codes, 0 = other, A,C,G,T = 1..4)
summary   the report: candidates, binomial tail (the library's own: `sf`), E-value, order, families"""
import math

import numpy as np

MAX_GAP = 26
LETTERS = "ACGT"
COLUMNS = "rank dyad gap count positions expected enrichment log10_pvalue log10_evalue other_gaps_mean family is_head".split()


def codes_of(s):
    return np.array(["NACGT".index(x) for x in s], np.uint8)


def rc3(x):
    return 16 * (3 - (x & 3)) + 4 * (3 - ((x >> 2) & 3)) + (3 - (x >> 4))


RC3 = np.array([rc3(x) for x in range(64)], np.int64)
RC6 = np.array([64 * RC3[k & 63] + RC3[k >> 6] for k in range(4096)], np.int64)


def key_of(a, b):
    """the key of the dyad of two triplets given as strings"""
    t = lambda w: 16 * LETTERS.index(w[0]) + 4 * LETTERS.index(w[1]) + LETTERS.index(w[2])
    return 64 * t(a) + t(b)


def canonical(key):
    return min(int(key), int(RC6[key]))


def dyad_string(key, g):
    a, b = key >> 6, key & 63
    w = lambda x: LETTERS[x >> 4] + LETTERS[(x >> 2) & 3] + LETTERS[x & 3]
    return w(a) + "n" * g + w(b)


# ---- the tables ----------------------------------------------------------------------------------------------------------
def tables(seqs, max_gap, both, weights=None):
    """(counts (max_gap + 1) x 4096 uint64, mono 64 uint64) of the sequences; weights: how many times each one counts.
    The sequences are laid end to end with one invalid base between them, which cuts every span as a sequence's end does."""
    assert 0 <= max_gap <= MAX_GAP
    counts = np.zeros((max_gap + 1, 4096), np.uint64)
    mono = np.zeros(64, np.uint64)
    parts, wts = [], []
    for i, c in enumerate(seqs):
        c = np.asarray(c, np.uint8)
        parts += [c, np.zeros(1, np.uint8)]
        wts.append(np.full(len(c) + 1, 1 if weights is None else int(weights[i]), np.int64))
    if not parts:
        return counts, mono
    c = np.concatenate(parts)
    w = np.concatenate(wts)
    n = len(c)
    v = (c >= 1) & (c <= 4)
    s = np.zeros(n + 40, np.int64)
    s[:n] = np.where(v, c.astype(np.int64) - 1, 0)
    pos = np.arange(n)
    nxt = np.minimum.accumulate(np.where(v, n, pos)[::-1])[::-1]  # the first invalid base at or behind p
    r = nxt - pos
    t = 16 * s[:-2] + 4 * s[1:-1] + s[2:]
    st = r >= 3
    mono += np.bincount(t[:n][st], weights=w[st], minlength=64).astype(np.uint64)
    for g in range(max_gap + 1):
        p = pos[r >= 6 + g]
        key = 64 * t[p] + t[p + 3 + g]
        if both:
            key = np.minimum(key, RC6[key])
        counts[g] += np.bincount(key, weights=w[p], minlength=4096).astype(np.uint64)  # (exact: far below 2^53)
    return counts, mono


def tables_literal(codes, max_gap, both):
    """the definition read position by position, for one sequence"""
    c = np.asarray(codes, np.uint8)
    L = len(c)
    counts = np.zeros((max_gap + 1, 4096), np.uint64)
    mono = np.zeros(64, np.uint64)
    ok = [1 <= x <= 4 for x in c]
    t = lambda p: 16 * (int(c[p]) - 1) + 4 * (int(c[p + 1]) - 1) + (int(c[p + 2]) - 1)
    for p in range(L):
        r = 0
        while p + r < L and ok[p + r]:
            r += 1
        if r >= 3:
            mono[t(p)] += 1
        for g in range(max_gap + 1):
            if r >= 6 + g:
                key = 64 * t(p) + t(p + 3 + g)
                counts[g, canonical(key) if both else key] += 1
    return counts, mono


# ---- the summary ---------------------------------------------------------------------------------------------------------
def frequencies(mono, both):
    m = np.asarray(mono, np.uint64)
    M = int(m.sum())
    if both:
        return np.array([float(int(m[x]) + int(m[RC3[x]])) / (2.0 * float(M)) for x in range(64)], np.float64)
    return np.array([float(int(m[x])) / float(M) for x in range(64)], np.float64)


def columns(key, g, rc=False):
    """the dyad as letters 0..3 and 4 for n"""
    if rc:
        key = int(RC6[key])
    a, b = key >> 6, key & 63
    tri = lambda x: [x >> 4, (x >> 2) & 3, x & 3]
    return tri(a) + [4] * g + tri(b)


def related(X, Y):
    for o in range(-2, 3):
        same, clash = 0, False
        for c in range(len(X)):
            cy = c - o
            if cy < 0 or cy >= len(Y) or X[c] == 4 or Y[cy] == 4:
                continue
            if X[c] == Y[cy]:
                same += 1
            else:
                clash = True
        if not clash and same >= 4:
            return True
    return False


def summary(counts, mono, both, sf, min_count=5, max_evalue=0.01):
    """the report as a list of dicts, in order; sf(n, k, p) = log10 P(X >= k), X ~ Binomial(n, p)"""
    counts = np.asarray(counts, np.uint64)
    G = counts.shape[0] - 1
    if int(np.asarray(mono, np.uint64).sum()) == 0:
        return []
    f = frequencies(mono, both)
    log_tests = math.log10(float((G + 1) * (2080 if both else 4096)))
    log_max = math.log10(max_evalue)
    rep = []
    for g in range(G + 1):
        T = int(counts[g].sum())
        for key in np.flatnonzero(counts[g]).tolist():
            c = int(counts[g, key])
            if c < min_count:
                continue
            p = float(f[key >> 6]) * float(f[key & 63])
            if both and int(RC6[key]) != key:
                p *= 2.0
            expected = float(T) * p
            if not float(c) > expected:
                continue
            lp = sf(T, c, p)
            le = lp + log_tests
            if not le <= log_max:
                continue
            other = sum(int(counts[h, key]) for h in range(G + 1) if h != g)
            rep.append(dict(gap=g, key=key, count=c, positions=T, p=p, expected=expected, log10_pvalue=lp, log10_evalue=le,
                            other_gaps_mean=float(other) / float(G) if G else 0.0, family=0, is_head=0))
    rep.sort(key=lambda d: (d["log10_evalue"], d["gap"], d["key"]))
    heads = []
    for k, d in enumerate(rep):
        Y = [columns(d["key"], d["gap"])] + ([columns(d["key"], d["gap"], True)] if both else [])
        for h in heads:
            X = columns(rep[h]["key"], rep[h]["gap"])
            if any(related(X, y) for y in Y):
                d["family"] = h + 1
                break
        else:
            heads.append(k)
            d["family"], d["is_head"] = k + 1, 1
    return rep


def render_tsv(rep):
    """the TSV of the CLI: numbers as --spacing formats its"""
    out = ["\t".join(COLUMNS)]
    for k, d in enumerate(rep):
        out.append("%d\t%s\t%d\t%d\t%d\t%.2f\t%.3f\t%.3f\t%.3f\t%.2f\t%d\t%d"
                   % (k + 1, dyad_string(d["key"], d["gap"]), d["gap"], d["count"], d["positions"], d["expected"],
                      d["count"] / d["expected"], d["log10_pvalue"], d["log10_evalue"], d["other_gaps_mean"], d["family"], d["is_head"]))
    return "\n".join(out) + "\n"


# ---- inputs --------------------------------------------------------------------------------------------------------------
def revcomp_codes(w):
    return (3 - np.asarray(w))[::-1]


def planted(seed, a="CGG", g=11, b="CCG", frac=0.3, n=2000, L=100):
    """the scenarios of the README's table: n uniform sequences of L bases, the dyad a n{g} b laid into a share `frac` of
    them on either strand (frac = 0: the draw is made all the same, nothing is laid)"""
    rng = np.random.default_rng(seed)
    A, B = codes_of(a).astype(np.int64) - 1, codes_of(b).astype(np.int64) - 1
    out = []
    for _ in range(n):
        s = rng.integers(0, 4, L)
        if rng.random() < frac:
            w = np.concatenate([A, rng.integers(0, 4, g), B])
            if rng.random() < 0.5:
                w = revcomp_codes(w)
            p = rng.integers(0, L - len(w) + 1)
            s[p:p + len(w)] = w
        out.append((s + 1).astype(np.uint8))
    return out


def fasta_text(seqs):
    return "".join(">s%d\n%s\n" % (i, "".join("NACGT"[x] for x in c)) for i, c in enumerate(seqs))


def edge_lengths(G):
    return sorted(set(list(range(8)) + [6 + G - 1, 6 + G, 6 + G + 1, 31, 32, 33, 63, 64, 65]))


def random_sequences(seed, lengths):
    """uniform letters of the given lengths"""
    rng = np.random.default_rng(seed)
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
