"""numpy restatement of --compare (include/pengk.h, "motif comparison"): quantised columns, the
integer column score, the alignments of a query with a target, the null of an overlap built over the whole database, the
best alignment of a pair, the match statistics and the TSV.  The yardstick of csrc/compare.hip and host/motif_compare.cpp;
nothing here is Tomtom's arithmetic.

A motif is a (w x 4) int16 array of quantised columns; a database is a list of them."""
import numpy as np

MAX_LEN = 64
SCALE = 4096
BINS = 257
NEAR_TIE = 1e-8  # a runner-up within this relative distance of the best p, and not bit-equal to it, is a near tie


# ---- 1. quantised columns ----------------------------------------------------------------------------------------------
def quantize(rows):
    """rows (w x 4 doubles, any positive scale) -> X (w x 4 int16): floor(4096 p / sum(p) + 0.5), the sum taken left to right"""
    p = np.asarray(rows, np.float64).reshape(-1, 4)
    s = ((p[:, 0] + p[:, 1]) + p[:, 2]) + p[:, 3]
    assert len(p) >= 1 and len(p) <= MAX_LEN and np.all(p >= 0) and np.all(s > 0) and np.all(np.isfinite(s))
    return np.floor(4096.0 * (p / s[:, None]) + 0.5).astype(np.int16)


def revcomp(X):
    """column order and letter order reversed"""
    return np.ascontiguousarray(np.asarray(X)[::-1, ::-1])


# ---- 2. column score ---------------------------------------------------------------------------------------------------
def column_scores(Q, T):
    """s[i, j] of every column i of Q against every column j of T: max(0, 256 - (d >> 17)), d the squared distance.
    (Columns that quantize made have d <= 2^25, so the clamp only meets columns a caller made up.)"""
    q = np.asarray(Q, np.int64).reshape(-1, 1, 4)
    t = np.asarray(T, np.int64).reshape(1, -1, 4)
    d = ((q - t) ** 2).sum(axis=2)
    return np.maximum(0, 256 - (d >> 17))


# ---- 4. null -------------------------------------------------------------------------------------------------------------
def null_histograms(Q, targets, both):
    """h[i, v] (w x 257 uint64): the (target, orientation, column) triples of the database that score v against column i.
    Reversing the column order moves no count, so the other orientation is the letter-reversed columns."""
    cols = np.concatenate([np.asarray(t, np.int16).reshape(-1, 4) for t in targets])
    if both:
        cols = np.concatenate([cols, cols[:, ::-1]])
    Q = np.asarray(Q, np.int16).reshape(-1, 4)
    h = np.zeros((len(Q), BINS), np.uint64)
    for i in range(len(Q)):
        h[i] = np.bincount(column_scores(Q[i:i + 1], cols)[0], minlength=BINS)
    return h


class NullTails:
    """tail(i0, n)[S] = P(sum of the scores of query columns [i0, i0 + n) >= S) under the null histograms h of one query:
    pmf_i = h_i / N, the n pmfs convolved in double, the suffix sums clamped to 1 and set to 1 up to the smallest sum the
    null can give (where P is 1 whatever the rounding).  Chains are built when first asked for."""

    def __init__(self, h):
        h = np.asarray(h, np.uint64)
        self.w = len(h)
        self.N = int(h[0].sum())
        assert self.N > 0 and all(int(r.sum()) == self.N for r in h)
        self.pmf = h.astype(np.float64) / float(self.N)
        self.smin = [int(np.flatnonzero(r)[0]) for r in h]
        self._chain = {}

    def tail(self, i0, n):
        assert 0 <= i0 and 1 <= n and i0 + n <= self.w
        ch = self._chain.setdefault(i0, {"cur": None, "tails": []})
        while len(ch["tails"]) < n:
            k = len(ch["tails"])
            ch["cur"] = self.pmf[i0].copy() if k == 0 else np.convolve(ch["cur"], self.pmf[i0 + k])
            t = np.minimum(np.cumsum(ch["cur"][::-1])[::-1], 1.0)
            t[:sum(self.smin[i0:i0 + k + 1]) + 1] = 1.0
            ch["tails"].append(t)
        return ch["tails"][n - 1]


# ---- 3., 5. alignments -------------------------------------------------------------------------------------------------
def n_offsets(wq, wt, both, M):
    m = min(M, wq, wt)
    return (2 if both else 1) * (wq + wt - 2 * m + 1)


def alignments(Q, T, both, M, tails):
    """every (o, k) of the pair in the order + before -, k ascending: a list of dicts orientation (0 = +, 1 = -), offset,
    overlap, score, p"""
    Q, T = np.asarray(Q, np.int16).reshape(-1, 4), np.asarray(T, np.int16).reshape(-1, 4)
    wq, wt = len(Q), len(T)
    m = min(M, wq, wt)
    out = []
    for o in range(2 if both else 1):
        s = column_scores(Q, revcomp(T) if o else T)
        for k in range(-(wt - m), wq - m + 1):
            i0, j0 = max(k, 0), max(-k, 0)
            n = min(wq - i0, wt - j0)
            S = int(s.diagonal(-k).sum())  # (the overlap is the whole diagonal: i0 or j0 is 0)
            out.append({"orientation": o, "offset": k, "overlap": n, "score": S, "p": float(tails.tail(i0, n)[S])})
    assert len(out) == n_offsets(wq, wt, both, M)
    return out


def rank_key(a):
    """definition 5: the smallest p, then the larger overlap, + before -, the smaller offset"""
    return (a["p"], -a["overlap"], a["orientation"], a["offset"])


def best_alignment(al):
    """(best, near): the alignment of definition 5 and the alignments of its near-tie band (not bit-equal to the best p, but
    within a relative NEAR_TIE of it)"""
    best = min(al, key=rank_key)
    near = [a for a in al if a["p"] != best["p"] and a["p"] - best["p"] <= NEAR_TIE * best["p"]]
    return best, near


# ---- 6. match statistics ---------------------------------------------------------------------------------------------
def summary(p_offset, n_off):
    """(p_match, evalue, qvalue) of one query's T targets: p_match = -expm1(n_offsets log1p(-p_offset)), 1 where p_offset is
    1; evalue = p_match T; qvalue: Benjamini-Hochberg over the T targets -- in ascending p_match (database order on ties)
    q_(r) = min over r' >= r of p_(r') T / r', at most 1"""
    p = np.asarray(p_offset, np.float64)
    n = np.asarray(n_off, np.float64)
    T = len(p)
    pm = np.ones(T, np.float64)
    lt = p < 1.0
    pm[lt] = -np.expm1(n[lt] * np.log1p(-p[lt]))
    ev = pm * float(T)
    order = np.argsort(pm, kind="stable")
    raw = pm[order] * float(T) / np.arange(1, T + 1, dtype=np.float64)
    qs = np.minimum(np.minimum.accumulate(raw[::-1])[::-1], 1.0)
    q = np.empty(T, np.float64)
    q[order] = qs
    return pm, ev, q


# ---- a whole query -------------------------------------------------------------------------------------------------------
def compare_query(Q, targets, both, M, h=None, only=None):
    """one query against a database: a dict of arrays over the targets (offset, orientation, overlap, score, n_offsets,
    p_offset, p_value, e_value, q_value), `near` (per target: the near-tie band of its best alignment), `all` (per target:
    every alignment) and `tails`.  only: the targets to align (the null is the whole database's all the same); the match
    statistics are then left out"""
    if h is None:
        h = null_histograms(Q, targets, both)
    tails = NullTails(h)
    T = len(targets)
    rec = {k: np.zeros(T, np.int32) for k in ("offset", "orientation", "overlap", "score", "n_offsets")}
    rec["p_offset"] = np.ones(T, np.float64)
    near, every = [None] * T, [None] * T
    for t in (range(T) if only is None else only):
        al = alignments(Q, targets[t], both, M, tails)
        b, nr = best_alignment(al)
        for k in ("offset", "orientation", "overlap", "score"):
            rec[k][t] = b[k]
        rec["n_offsets"][t] = len(al)
        rec["p_offset"][t] = b["p"]
        near[t], every[t] = nr, al
    if only is None:
        rec["p_value"], rec["e_value"], rec["q_value"] = summary(rec["p_offset"], rec["n_offsets"])
    rec["near"], rec["all"], rec["tails"] = near, every, tails
    return rec


# ---- 7. output -----------------------------------------------------------------------------------------------------------
HEADER = "motif\tiupac\ttarget\ttarget_width\toffset\torientation\toverlap\tscore\tn_offsets\tp_offset\tp_value\te_value\tq_value\n"


def render(queries, iupacs, targets, names, both, M=5, E=1.0):
    """the TSV of --compare: per query (1-based, in the order given) the targets by p_value ascending, then database order;
    only lines with e_value <= E"""
    out = [HEADER]
    for m, Q in enumerate(queries):
        r = compare_query(Q, targets, both, M)
        for t in np.argsort(r["p_value"], kind="stable"):
            if not r["e_value"][t] <= E:
                continue
            out.append("%d\t%s\t%s\t%d\t%d\t%s\t%d\t%d\t%d\t%.6e\t%.6e\t%.6e\t%.6e\n" % (
                m + 1, iupacs[m], names[t], len(targets[t]), r["offset"][t], "-" if r["orientation"][t] else "+", r["overlap"][t],
                r["score"][t], r["n_offsets"][t], r["p_offset"][t], r["p_value"][t], r["e_value"][t], r["q_value"][t]))
    return "".join(out)


# ---- databases of the tests ----------------------------------------------------------------------------------------------
WORDS = (("MARE", "TGCTGASTCAGCA"), ("AP1", "TGASTCA"), ("CRE", "TGACGTCA"), ("EBOX", "CACGTG"), ("GATA", "AGATAA"))


def word_rows(word):
    """0.94 on the letter, 0.02 elsewhere; S = 0.47 C / G, 0.03 A / T"""
    rows = []
    for c in word:
        if c == "S":
            rows.append([0.03, 0.47, 0.47, 0.03])
        else:
            r = [0.02] * 4
            r["ACGT".index(c)] = 0.94
            rows.append(r)
    return np.array(rows, np.float64)


def dirichlet_rows(rng, w, alpha=0.3):
    r = rng.dirichlet([alpha] * 4, size=w)
    return np.maximum(r, 1e-12)  # (a row never sums to zero)


def planted_database(n_decoys=200, seed=2024):
    """(names, rows): n_decoys decoys with Dirichlet(0.3) columns and widths 6..19, then the five word motifs"""
    rng = np.random.default_rng(seed)
    names, rows = [], []
    for d in range(n_decoys):
        w = int(rng.integers(6, 20))
        names.append("decoy%03d" % d)
        rows.append(dirichlet_rows(rng, w))
    for name, word in WORDS:
        names.append(name)
        rows.append(word_rows(word))
    return names, rows


def write_meme(path, names, rows, crlf=False):
    nl = "\r\n" if crlf else "\n"
    with open(path, "w", newline="") as f:
        f.write("MEME version 4" + nl + nl + "ALPHABET= ACGT" + nl + nl)
        for name, r in zip(names, rows):
            f.write("MOTIF %s" % name + nl + "letter-probability matrix: alength= 4 w= %d nsites= 20 E= 0" % len(r) + nl)
            for row in r:
                f.write(" ".join("%.17g" % v for v in row) + nl)
            f.write(nl)


# ---- the cases of tests/test_gpu_motif_compare.py (built here so that the CPU module can count their near ties) ----------
ALIGN_WIDTHS = (1, 4, 5, 6, 13, 63, 64)
ALIGN_OVERLAPS = (1, 5, 64)


def random_motif(rng, w):
    return quantize(dirichlet_rows(rng, w))


def decoys(rng, n, lo=6, hi=19):
    return [random_motif(rng, int(rng.integers(lo, hi + 1))) for _ in range(n)]


def alignment_case():
    """(queries, targets): one query and one target of every width of ALIGN_WIDTHS, and 40 decoys behind the targets so
    that the null is not the pair's own"""
    rng = np.random.default_rng(7)
    queries = [random_motif(rng, w) for w in ALIGN_WIDTHS]
    targets = [random_motif(rng, w) for w in ALIGN_WIDTHS] + decoys(rng, 40)
    return queries, targets


CONSTRUCTED = ("palindrome", "revcomp", "wide", "core", "twin_a", "twin_b")


def constructed_case():
    """(queries, targets, names): query 0 a random motif of width 12, query 1 the middle of the palindrome.  Targets by
    name: a palindrome (its own reverse complement), query 0's reverse complement, query 0 between flanks of 4 and 2
    columns (offset -4), columns 3..10 of query 0 (offset +3), the same random motif twice; then 30 decoys"""
    rng = np.random.default_rng(11)
    q0 = random_motif(rng, 12)
    half = random_motif(rng, 7)
    pal = np.concatenate([half, revcomp(half)])
    assert np.array_equal(pal, revcomp(pal))
    twin = random_motif(rng, 9)
    targets = [pal, revcomp(q0), np.concatenate([random_motif(rng, 4), q0, random_motif(rng, 2)]), q0[3:11].copy(), twin,
               twin.copy()] + decoys(rng, 30)
    names = list(CONSTRUCTED) + ["decoy%02d" % i for i in range(30)]
    return [q0, pal[3:12].copy()], targets, names


def self_match_case():
    """(queries, targets): three motifs of width 64 -- more than one batch of pengk_compare_motifs -- and a database of 60
    decoys with query 0 itself at its end"""
    rng = np.random.default_rng(13)
    queries = [random_motif(rng, 64) for _ in range(3)]
    return queries, decoys(rng, 60) + [queries[0].copy()]


def spread_columns(step=0.05, hi=0.5, dist=0.1):
    """columns on a grid of the simplex, no entry above hi, every one at least dist (a score below 256: 0.0884 and more) from
    every other, from every other's letter-reversed column and from its own"""
    pts = []
    k = int(round(1 / step))
    for a in range(k + 1):
        for b in range(k + 1 - a):
            for c in range(k + 1 - a - b):
                x = np.array([a, b, c, k - a - b - c]) * step
                if x.max() > hi + 1e-9 or np.linalg.norm(x - x[::-1]) < dist:
                    continue
                if all(np.linalg.norm(x - y) >= dist and np.linalg.norm(x - y[::-1]) >= dist for y in pts):
                    pts.append(x)
    return np.array(pts)


def corner_rows(rng, w):
    """columns with 0.7 and more on one letter: none scores 256 against a column of spread_columns"""
    r = rng.dirichlet([0.3] * 4, size=w) * 0.3
    r[np.arange(w), rng.integers(0, 4, size=w)] += 0.7
    return r


def large_case():
    """(query, targets, checked): a database of about 70 000 columns with the query (width 64) at index 100, and the
    targets whose records the GPU test holds to the model.  The query's columns score 256 against themselves alone among
    the 140 000 columns of both orientations, so the p_offset of its self-match, about 1e-329, underflows"""
    rng = np.random.default_rng(17)
    targets = [quantize(corner_rows(rng, int(rng.integers(6, 20)))) for _ in range(5600)]
    q = quantize(spread_columns()[:64])
    assert len(q) == 64
    targets[100] = q.copy()
    return q, targets, list(range(90, 110))


def near_tie_share(rec, checked):
    return sum(1 for t in checked if rec["near"][t]) / float(len(checked))
