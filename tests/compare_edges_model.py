"""Constructed inputs for the kernels of csrc/compare.hip at their value edges, and the exact references they are compared
with (tests/test_compare_edges_cpu.py holds every case to its class, tests/test_gpu_compare_edges.py only compares).  No
device here.

Why exact: take a null with N = 2^k and an overlap of n columns with k n <= 52.  Every pmf entry, every product, every
partial sum of the convolution and every suffix sum is then a multiple of 2^-(k n) that is at most 1, so a double holds
it exactly: the result is the same in any summation order, with or without fused multiply-adds.  The device and
motif_compare_model.NullTails must equal integer arithmetic bit for bit, and two candidates tie on p exactly when their
integer counts tie.

References
  ExactTails     the counts of the null in int64: per (i0, n) the suffix sums of the integer convolution of the
                 histograms, the denominator N^n and the smallest sum.  The expected double is 1.0 for S <= the smallest
                 sum, else count / N^n, and the quotient is asserted to be exact (count 2^52 is a multiple of N^n).
  exact_table    ExactTails in the order of pengk_test_compare_tails; tail_slice(w, i0, n) is where (i0, n) lies in it.
  delta_table    the closed form for histograms with all mass in one bin per row: 1 up to the sum of the bins, 0 above.

Histograms (for the hook)                                                   databases (for the real entries)
  dyadic (k, w) in DYADIC, three variants each                                dyadic_database: N = 64 both, N = 64 plus,
  deltas, w = 64, N = 1 and 2^32, five bin patterns                                            N = 256 both
  one count at the top, w = 64, N = 2^16 and 2^32                             all_ones_database: every column uniform
  realistic, w = 64, N = 140 000
"""
import functools
import math

import numpy as np

import motif_compare_model as mc

BINS = mc.BINS
MAX_LEN = mc.MAX_LEN


# ---- the order of the table -------------------------------------------------------------------------------------------
def tails_before(n):
    """the doubles of tail(i0, 1) .. tail(i0, n - 1): sum over n' < n of 256 n' + 1"""
    return 128 * (n - 1) * n + (n - 1)


def table_size(w):
    return sum(tails_before(w - i0 + 1) for i0 in range(w))


def tail_slice(w, i0, n):
    """where tail(i0, n), 256 n + 1 doubles, lies in the table of a query of width w (pengk_test_compare_tails)"""
    assert 0 <= i0 and 1 <= n and i0 + n <= w <= MAX_LEN
    a = sum(tails_before(w - i + 1) for i in range(i0)) + tails_before(n)
    return slice(a, a + 256 * n + 1)


def table_of(w, tail):
    """the flat table from tail(i0, n) -> array"""
    out = np.empty(table_size(w), np.float64)
    for i0 in range(w):
        for n in range(1, w - i0 + 1):
            out[tail_slice(w, i0, n)] = tail(i0, n)
    return out


# ---- exact reference ----------------------------------------------------------------------------------------------------
def int_convolve(cur, col):
    """np.convolve(cur, col) on int64; a column with few non-empty bins is added shift by shift (the same integers)"""
    nz = np.flatnonzero(col)
    if len(nz) > 16:
        return np.convolve(cur, col)
    out = np.zeros(len(cur) + len(col) - 1, np.int64)
    for u in nz:
        out[u:u + len(cur)] += cur * col[u]
    return out


class ExactTails:
    """tail(i0, n) = (count, D, vmin): count[S] = the tuples (v_i0, .., v_i0+n-1), weighted by their histogram counts, with
    sum >= S (int64; np.convolve, then the suffix sums), D = N^n and vmin = the smallest sum with a count.  Chains are
    built when first asked for, as NullTails'."""

    def __init__(self, h):
        h = np.asarray(h, np.uint64)
        self.w = len(h)
        self.N = int(h[0].sum())
        assert self.N > 0 and all(int(r.sum()) == self.N for r in h)
        self.h = h.astype(np.int64)
        self.smin = [int(np.flatnonzero(r)[0]) for r in h]
        self._chain = {}

    def tail(self, i0, n):
        assert 0 <= i0 and 1 <= n and i0 + n <= self.w
        assert self.N ** n <= 2 ** 62, "the counts of this overlap do not fit an int64"
        ch = self._chain.setdefault(i0, {"cur": None, "tails": []})
        while len(ch["tails"]) < n:
            k = len(ch["tails"])
            ch["cur"] = self.h[i0].copy() if k == 0 else int_convolve(ch["cur"], self.h[i0 + k])
            assert ch["cur"].dtype == np.int64 and int(ch["cur"].sum()) == self.N ** (k + 1)
            ch["tails"].append((np.cumsum(ch["cur"][::-1])[::-1], self.N ** (k + 1), sum(self.smin[i0:i0 + k + 1])))
        return ch["tails"][n - 1]

    def expected(self, i0, n):
        """the doubles of tail(i0, n); asserts that every quotient is exact"""
        count, D, vmin = self.tail(i0, n)
        r = D // math.gcd(D, 2 ** 52)  # count 2^52 % D == 0  <=>  count % (D / gcd(D, 2^52)) == 0
        assert count[0] == D and not np.any(count % r), (i0, n)
        assert int(count.max()) <= 2 ** 53 and (D <= 2 ** 53 or D & (D - 1) == 0)  # (both operands are doubles)
        out = count.astype(np.float64) / float(D)
        assert np.all(out[:vmin + 1] == 1.0)
        return out


def exact_table(h):
    ex = ExactTails(h)
    return table_of(ex.w, ex.expected)


def null_table(h):
    """the yardstick's table (motif_compare_model.NullTails) in the same order"""
    nt = mc.NullTails(h)
    return table_of(nt.w, nt.tail)


def delta_bins(h):
    h = np.asarray(h)
    assert np.all(np.count_nonzero(h, axis=1) == 1)
    return [int(np.flatnonzero(r)[0]) for r in h]


def delta_table(h):
    """all mass in one bin per row: tail(i0, n)[S] is 1 for S <= the sum of the bins and 0 above, whatever N"""
    b = delta_bins(h)
    return table_of(len(b), lambda i0, n: (np.arange(256 * n + 1) <= sum(b[i0:i0 + n])).astype(np.float64))


# ---- histograms ------------------------------------------------------------------------------------------------------------
DYADIC = ((1, 52), (2, 26), (4, 13), (6, 8), (13, 4), (26, 2), (32, 1))
VARIANTS = ("random", "ends", "lifted")


def composition(rng, total, parts):
    """`parts` positive integers that sum to `total`"""
    cuts = np.sort(rng.integers(0, total - parts + 1, size=parts - 1, dtype=np.int64))
    return np.diff(np.concatenate([[0], cuts, [total - parts]])) + 1


def dyadic_histogram(k, w, variant):
    """w rows that sum to N = 2^k, each with up to min(2^k, 40) non-empty bins at random places.  `ends`: bins 0 and 256
    are always among them ((1, 52): every row is {0: 1, 256: 1}, whose top cell 2^-52 lies at v = 13 x 1024); `lifted`:
    the lowest bin of every row is above 0, so that the smallest sum grows along the chain"""
    rng = np.random.default_rng(1000 * k + w + 7 * VARIANTS.index(variant))
    N = 2 ** k
    h = np.zeros((w, BINS), np.uint64)
    for i in range(w):
        m = int(rng.integers(2 if variant == "ends" else 1, min(N, 40) + 1))
        if variant == "ends":
            bins = np.concatenate([[0, 256], rng.choice(np.arange(1, 256), size=m - 2, replace=False)])
        elif variant == "lifted":
            lo = int(rng.integers(1, 120))
            bins = rng.choice(np.arange(lo, BINS), size=m, replace=False)
        else:
            bins = rng.choice(BINS, size=m, replace=False)
        h[i, bins] = composition(rng, N, m).astype(np.uint64)
    assert np.all(h.sum(axis=1) == N)
    return h


DELTA_PATTERNS = ("all0", "all256", "all1", "all255", "mix")
DELTA_N = (1, 2 ** 32)


def delta_histogram(pattern, N):
    """w = 64, all N counts of a row in one bin (all256: v = 16384, the one value of a thread's 17th slot)"""
    if pattern == "mix":
        bins = np.random.default_rng(5).choice([0, 1, 128, 255, 256], size=MAX_LEN)
    else:
        bins = np.full(MAX_LEN, int(pattern[3:]))
    h = np.zeros((MAX_LEN, BINS), np.uint64)
    h[np.arange(MAX_LEN), bins] = N
    return h


ONE_COUNT_K = (16, 32)


def one_count_histogram(k):
    """w = 64, every row {0: 2^k - 1, 256: 1}: the top cell of (i0, n) is one chain of exact products, 2^-(k n)"""
    h = np.zeros((MAX_LEN, BINS), np.uint64)
    h[:, 0] = 2 ** k - 1
    h[:, 256] = 1
    return h


def one_count_top(k, n):
    """the top cell of every (i0, n): k = 16: 2^-1024, a denormal, at n = 64; k = 32: a denormal at n = 33, 0 from 34 on"""
    return math.ldexp(1.0, -k * n)


@functools.lru_cache(maxsize=None)
def realistic_histogram():
    """w = 64, every row the bincount of 140 000 scores floor(257 x), x from a Beta distribution of the row's own"""
    rng = np.random.default_rng(23)
    h = np.zeros((MAX_LEN, BINS), np.uint64)
    for i in range(MAX_LEN):
        a, b = rng.uniform(0.6, 6.0, size=2)
        v = np.minimum(np.floor(257.0 * rng.beta(a, b, size=140000)).astype(np.int64), 256)
        h[i] = np.bincount(v, minlength=BINS)
    return h


def yardstick_histograms():
    """non-dyadic nulls small enough for exact rationals: (N, h) with w <= 6, N = 1000 and N = 139 999"""
    rng = np.random.default_rng(29)
    out = []
    for N, w in ((1000, 6), (139999, 6), (1000, 3), (139999, 4)):
        h = np.zeros((w, BINS), np.uint64)
        for i in range(w):
            a, b = rng.uniform(0.6, 6.0, size=2)
            v = np.minimum(np.floor(257.0 * rng.beta(a, b, size=N)).astype(np.int64), 256)
            h[i] = np.bincount(v, minlength=BINS)
        out.append((N, h))
    return out


# ---- databases ---------------------------------------------------------------------------------------------------------------
# quantised columns: U is uniform, P its own letter reversal, A and its letter reversal A', B a column like no other
ALPHABET = np.array([[1024, 1024, 1024, 1024],   # U
                     [1408, 640, 640, 1408],     # P
                     [1920, 896, 768, 512],      # A
                     [512, 768, 896, 1920],      # A'
                     [768, 1792, 640, 896]],     # B
                    np.int16)
assert np.all(ALPHABET.sum(axis=1) == 4096) and np.array_equal(ALPHABET[1], ALPHABET[1][::-1])
assert np.array_equal(ALPHABET[2], ALPHABET[3][::-1])

DB_QUERY_WIDTHS = (1, 5, 13, 40, 64)
DB_OVERLAPS = (1, 5, 64)
DATABASES = {  # name: (target widths, both, seed)
    "n64_both": ((8, 7, 6, 5, 3, 2, 1), True, 3),
    "n64_plus": ((8, 8, 8, 8, 7, 7, 6, 5, 3, 2, 1, 1), False, 4),
    "n256_both": ((6,) * 16 + (5, 5, 5, 5, 4, 3, 2, 1, 1, 1), True, 5),
}


def alphabet_motif(rng, w):
    return ALPHABET[rng.integers(0, len(ALPHABET), size=w)].copy()


@functools.lru_cache(maxsize=None)
def dyadic_database(name):
    """(queries, targets, both): columns drawn from ALPHABET; N (the database's columns, in both orientations where `both`)
    is 64 or 256, and no target is wider than 52 / log2(N) columns, so that every overlap's null is exact"""
    widths, both, seed = DATABASES[name]
    rng = np.random.default_rng(seed)
    targets = [alphabet_motif(rng, w) for w in widths]
    queries = [alphabet_motif(rng, w) for w in DB_QUERY_WIDTHS]
    N = sum(widths) * (2 if both else 1)
    assert N in (64, 256) and max(widths) * int(math.log2(N)) <= 52
    return queries, targets, both


def tie_stages(al):
    """how definition 5 picks among the alignments that are bit-equal to the best p: (tied, by_overlap, by_orientation,
    by_offset) -- the number tied, and whether each stage had more than one value to choose from"""
    best = min(a["p"] for a in al)
    tied = [a for a in al if a["p"] == best]
    n = max(a["overlap"] for a in tied)
    widest = [a for a in tied if a["overlap"] == n]
    o = min(a["orientation"] for a in widest)
    same = [a for a in widest if a["orientation"] == o]
    return len(tied), len(widest) < len(tied), len(same) < len(widest), len(same) > 1


ALL_ONES_WIDTHS = (64, 10, 1)


@functools.lru_cache(maxsize=None)
def all_ones_database():
    """(queries, targets): every database column is uniform, so every query column scores one value against all of them:
    every tail is 1 and every candidate of every pair ties on p.  Queries and targets of the widths ALL_ONES_WIDTHS"""
    rng = np.random.default_rng(31)
    targets = [np.repeat(ALPHABET[:1], w, axis=0) for w in ALL_ONES_WIDTHS]
    queries = [mc.random_motif(rng, w) for w in ALL_ONES_WIDTHS]
    return queries, targets


def all_ones_record(Q, wt):
    """the record of definition 5 when every candidate has p = 1 (M = 1, both orientations): the largest overlap min(wq,
    wt), +, and the smallest offset that gives it: 0 when the target is no wider than the query, else -(wt - wq).
    (offset, orientation, overlap, score, n_offsets)"""
    wq = len(Q)
    n = min(wq, wt)
    k = 0 if wt <= wq else -(wt - wq)
    S = int(mc.column_scores(Q[max(k, 0):max(k, 0) + n], ALPHABET[:1]).sum())
    return (k, 0, n, S, 2 * (wq + wt - 1))


# ---- host-plan seams -------------------------------------------------------------------------------------------------------
CHUNK_SEAMS = (8191, 8192, 8193, 16384, 16385)


def columns_database(rng, total):
    """motifs of random widths up to 64 with `total` columns in all"""
    out = []
    while total:
        w = min(total, int(rng.integers(1, 65)))
        out.append(mc.random_motif(rng, w))
        total -= w
    return out


BATCH_QUERIES = 4097
BATCH_SAMPLE = (0, 1, 4095, 4096, 2, 3, 511, 1024, 2047, 2048, 3000, 3333, 4093, 4094)


@functools.lru_cache(maxsize=None)
def batch_case():
    """(queries, targets): 4097 queries of alternating width 1 and 2 -- one more than a batch holds -- and three targets"""
    rng = np.random.default_rng(37)
    cols = mc.random_motif(rng, 64)
    queries = [cols[rng.integers(0, 64, size=1 + q % 2)].copy() for q in range(BATCH_QUERIES)]
    targets = [mc.random_motif(rng, w) for w in (3, 1, 6)]
    return queries, targets


MIXED_WIDTHS = (64, 64, 7, 64, 3)


@functools.lru_cache(maxsize=None)
def mixed_width_case():
    """(queries, targets): the tails of widths 64, 64 and 7 fit 256 MiB, the third 64 does not: the second batch is (64, 3)"""
    rng = np.random.default_rng(41)
    need = [table_size(w) * 8 for w in MIXED_WIDTHS]
    assert sum(need[:3]) <= 256 << 20 < sum(need[:4])
    return [mc.random_motif(rng, w) for w in MIXED_WIDTHS], mc.decoys(rng, 12)
