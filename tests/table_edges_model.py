"""Constructed inputs for the table-space kernels (background model, pattern-space sweep, seed compaction, IUPAC
aggregation, similarity grid) and their expected values from the oracle (oracle/oracle.py).  It adds no semantics of its
own: include/pengk.h is the specification, the oracle the reference.  Everything here is deterministic; nothing comes from
a count over sequences, so that the tables can hold what natural data never does -- counts at 5 / 6, at the expected
count rounded down and up, at 2^24 +- 1 (where (float)n starts rounding), at the top of the 32-bit bin, background
products that reach the denormals and zero, ltot beyond 2^32.

tests/test_table_edges_cpu.py asserts on the oracle's side alone that the cases below really hold those classes;
tests/test_gpu_table_edges.py compares the device with them."""
import numpy as np

from oracle import oracle as po

U32_MAX = 2 ** 32 - 1
LTOTS = (1000, 2 ** 24 + 1, 2_500_000_000, 20_000_000_000)
# the values every class of pattern meets, whatever the table; four more per table come from its own expected counts
FIXED_EDGES = (0, 1, 5, 6, 7, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 31, 2 ** 32 - 2, U32_MAX)
N_EDGES = len(FIXED_EDGES) + 4  # 15: odd, and at most the 16 patterns of W = 2


# ---- pattern ids ---------------------------------------------------------------------------------------------------
def revcomp_ids(W):
    """rc(x) of every pattern id x < 4^W (uint32): digits reversed and complemented, by swaps of bit groups"""
    x = np.arange(4 ** W, dtype=np.uint32)
    x ^= np.uint32(4 ** W - 1)  # complement: 3 - digit
    for s, m in ((2, 0x33333333), (4, 0x0F0F0F0F), (8, 0x00FF00FF)):
        x = ((x >> np.uint32(s)) & np.uint32(m)) | ((x & np.uint32(m)) << np.uint32(s))
    x = (x >> np.uint32(16)) | (x << np.uint32(16))
    return x >> np.uint32(32 - 2 * W)


def own_twin_tile_mask(W):
    """patterns of the tiles the twin-tile kernel evaluates pattern by pattern (W >= 12): the middle W - 6 digits are
    their own reverse complement"""
    mid = np.arange(4 ** (W - 6), dtype=np.uint32)
    own = revcomp_ids(W - 6) == mid
    x = np.arange(4 ** W, dtype=np.uint32)
    return own[(x >> np.uint32(6)) & np.uint32(4 ** (W - 6) - 1)]


def _hash(x):
    """a cheap integer hash (the 32-bit finalizer of MurmurHash3) of uint32 values"""
    h = x.astype(np.uint32)
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


# ---- count tables --------------------------------------------------------------------------------------------------
def mu_edges(mu):
    """four counts derived from a table's expected counts: the median and the 99th percentile, rounded down and up (+1
    where mu is an integer) -- a hundredth and a half of the patterns expect at least that many, so (float)n > mu falls
    both ways, with n > 5 wherever the table's expected counts reach 6 at all"""
    m = np.asarray(mu, np.float64)
    m = m[np.isfinite(m)]
    out = []
    for q in (np.quantile(m, 0.99), np.median(m)) if m.size else (0.0, 0.0):
        lo = int(min(max(np.floor(q), 0), U32_MAX))
        out += [lo, min(lo + 1, U32_MAX)]
    return tuple(out)


def edge_counts(W, derived=(2, 3, 4, 100), mirrored=False, salt=0):
    """uint32[4^W]: within every run of N_EDGES consecutive ids every edge value occurs once, the run's rotation being a
    hash of its index -- so W = 2 holds them all, and every class of pattern (pair tiles, own-twin tiles, palindromes,
    both halves of a twin pair) meets every edge.  As built, twins differ; mirrored: c[rc(x)] = c[x] for x < rc(x)."""
    assert len(derived) == N_EDGES - len(FIXED_EDGES)
    edges = np.array(FIXED_EDGES + tuple(derived), np.uint64).astype(np.uint32)
    x = np.arange(4 ** W, dtype=np.uint32)
    rot = _hash(x // np.uint32(N_EDGES) + np.uint32(salt * 0x9E3779B1 & 0xFFFFFFFF)) % np.uint32(N_EDGES)
    c = edges[(x % np.uint32(N_EDGES) + rot) % np.uint32(N_EDGES)]
    if mirrored:
        r = revcomp_ids(W)
        c = np.where(x < r, c, c[r])
    return np.ascontiguousarray(c, np.uint32)


# ---- background counters and V tables ----------------------------------------------------------------------------------
def _counter_set(kind):
    """84 counters n[0] (4) | n[1] (16) | n[2] (64) with the structure real ones have (a context occurs at least as often
    as its extensions together)"""
    t = np.arange(64, dtype=np.uint32)
    n2 = (_hash(t + np.uint32(977)) % np.uint32(1900) + np.uint32(40)).astype(np.int64).reshape(4, 4, 4)
    if kind == "no_T":  # a letter that never occurs
        n2[3, :, :] = 0
        n2[:, 3, :] = 0
        n2[:, :, 3] = 0
    if kind == "no_context":  # contexts that never occur: n_ab = 0, every letter present
        for a, b in ((1, 2), (3, 0), (2, 2)):
            n2[a, b, :] = 0
            n2[:, a, b] = 0
    n1 = n2.sum(axis=2)
    n1 = np.where(n1 > 0, n1 + 1, 0)
    n0 = n1.sum(axis=1)
    n0 = np.where(n0 > 0, n0 + 1, 0)
    n = np.concatenate([n0, n1.reshape(-1), n2.reshape(-1)]).astype(np.int64)
    if kind == "above_2_24":
        n = n * 9000        # counters up to 1.7e7 .. 3e8, their sum below 2^31: the reference's `int` still holds them
    if kind == "above_2_31":
        n = n * 3_000_011   # counters beyond 2^31: the 64-bit semantics the product documents (po.bg_V(..., wide=True))
    return n


COUNTER_KINDS = ("natural", "no_T", "no_context", "above_2_24", "above_2_31")
ALPHAS = ((1.0, 1.0, 1.0), (0.5, 2.0, 10.0), (1e-3, 1e-3, 1e-3))


def natural_counters():
    codes, offs = po.synth(3, 0, 2000, 150)
    return po.bg_counts(codes, offs, 2)


def counter_sets():
    """name -> (int64[84], wide): wide = compare with the 64-bit counter semantics"""
    out = {"natural": (natural_counters(), False)}
    for kind in COUNTER_KINDS[1:]:
        out[kind] = (_counter_set(kind), kind == "above_2_31")
    return out


def bg_model_cases():
    """(name, counters int64[84], K, alpha, expected V float32[84]); entries beyond order K are 0"""
    cases = []
    for name, (n, wide) in counter_sets().items():
        for alpha in ALPHAS:
            for K in (0, 1, 2):
                used = sum(4 ** (k + 1) for k in range(K + 1))
                V = np.zeros(84, np.float32)
                V[:used] = po.bg_V(n[:used], K, alpha, wide=wide)
                cases.append(("%s_K%d_a%g" % (name, K, alpha[1]), n, K, alpha, V))
    return cases


def hand_made_V():
    """V (c): rows that still sum to 1 (as far as float32 lets them) but hold entries of 1e-4 .. 1e-6 and exact zeros, so
    that products of 14 factors cover normal, denormal and zero"""
    rows = np.array([[1 - 1.11e-4, 1e-4, 1e-5, 1e-6],
                     [0.5, 0.5, 0.0, 0.0],
                     [0.25, 0.25, 0.25, 0.25],
                     [1e-6, 1e-5, 0.7 - 1.1e-5, 0.3],
                     [0.0, 1e-4, 0.9999, 0.0],
                     [0.3, 0.2, 0.4999, 1e-4]], np.float64)
    V = np.zeros(84, np.float64)
    V[0:4] = (1e-4, 0.55, 0.4498, 1e-4)  # A and T both rare: a pattern AND its reverse complement can be tiny
    for c in range(4):
        V[4 + 4 * c:8 + 4 * c] = np.roll(rows[(c + 1) % 6], c)
    for c in range(16):
        V[20 + 4 * c:24 + 4 * c] = np.roll(rows[(5 * c + 2) % 6], c // 4)
    V[80:84] = (0.4999, 0.3, 0.2, 1e-4)  # context TT -> T stays tiny: T-rich patterns reach the denormals at order 2 as well
    return V.astype(np.float32)


_V = {}


def sweep_V(kind):
    """the three V tables the sweeps run on: "a" natural counters, "b" constructed counters (a letter that never occurs,
    alpha 1e-3: conditional probabilities down to 1e-8), "c" hand-made"""
    if kind not in _V:
        if kind == "a":
            _V[kind] = po.bg_V(natural_counters(), 2)
        elif kind == "b":
            _V[kind] = po.bg_V(_counter_set("no_T"), 2, ALPHAS[2])
        else:
            _V[kind] = hand_made_V()
    return _V[kind]


# ---- sweep cases -----------------------------------------------------------------------------------------------------
def legal_orders(W):
    return [(k, mk) for mk in range(min(2, W - 1) + 1) for k in range(mk + 1)]


def small_sweep_cases(W, both):
    """W <= 10: the full cross product (V kind, ltot, k, max_k, mirrored)"""
    return [(v, lt, k, mk, mir) for v in "abc" for lt in LTOTS for (k, mk) in legal_orders(W) for mir in (False, True)]


# W = 12 and 14: chosen so that under each kernel (the twin-tile kernel: both strands, sweep_pairs = 1; the per-pattern
# kernel: both strands with sweep_pairs = 0, and the plus strand) every V kind, every ltot, k < max_k and both table
# forms occur.  The both-strand cases run under both kernels; cases are ordered by V so that the oracle's probability
# tables are built once per (V, strand mode).
BIG_BOTH = (("a", LTOTS[2], 1, 2, True), ("b", LTOTS[1], 0, 1, False), ("c", LTOTS[3], 2, 2, False), ("c", LTOTS[0], 0, 2, True))
BIG_PLUS = (("a", LTOTS[1], 2, 2, False), ("b", LTOTS[0], 1, 1, True), ("c", LTOTS[3], 0, 1, False), ("c", LTOTS[2], 1, 2, True))


# W = 14 (an oracle sweep over 2^28 patterns takes a minute): what only W = 14 can show -- products of 14 factors, the
# three-level tables -- on V "c" and "a"; V "b" and the other two ltot are W = 12's, under the same two kernels.
BIG14_BOTH = (("a", LTOTS[2], 0, 1, True), ("c", LTOTS[3], 2, 2, False))
BIG14_PLUS = (("a", LTOTS[0], 0, 0, False), ("c", LTOTS[1], 1, 2, False))


def big_sweep_cases(W, both):
    if W == 14:
        return list(BIG14_BOTH if both else BIG14_PLUS)
    return list(BIG_BOTH if both else BIG_PLUS)


def sweep_cases(W, both):
    return small_sweep_cases(W, both) if W <= 10 else big_sweep_cases(W, both)


def sweep_tag(W, both, case):
    """the unique name of a sweep case (the key of its entry in tests/golden/edges_tables_w*.npz)"""
    v, lt, k, mk, mir = case
    return "sweep/W%d/%s/V%s/ltot%d/k%d/maxk%d/%s" % (W, "both" if both else "plus", v, lt, k, mk, "mirrored" if mir else "as_built")


_bgp = {"key": None, "orders": {}}


def oracle_bgprob(W, vkind, both, order):
    """po.bgprob, kept for the (W, V, strand mode) in use only (a table is 1 GiB at W = 14)"""
    key = (W, vkind, bool(both))
    if _bgp["key"] != key:
        _bgp["key"], _bgp["orders"] = key, {}
    if order not in _bgp["orders"]:
        _bgp["orders"][order] = po.bgprob(W, order, sweep_V(vkind), both)
    return _bgp["orders"][order]


def sweep_case(W, both, case):
    """dict of one case: V, ltot, k, max_k, counts (uint32) and the oracle's bgprob[0..max_k], expected, logp, z"""
    vkind, ltot, k, max_k, mirrored = case
    po.set_threads(16)
    try:
        bgp = [oracle_bgprob(W, vkind, both, o) for o in range(max_k + 1)]
        mu = bgp[k] * np.float32(ltot)
        step = max(1, mu.size // (1 << 20))  # (the derived edges need a typical and a large mu, not the exact extremes)
        counts = edge_counts(W, mu_edges(mu[::step]), mirrored, salt=W)
        del mu
        e, lp, z = po.stats(W, counts.astype(np.uint64), bgp[k], ltot)
    finally:
        po.set_threads(1)
    return dict(W=W, both=both, V=sweep_V(vkind), vkind=vkind, ltot=ltot, k=k, max_k=max_k, mirrored=mirrored, counts=counts,
                bgp=bgp, expected=e, logp=lp, z=z)


def count_classes(c):
    """name -> bool mask of the branches of pattern_statistics (csrc/stats.hip) a pattern of the case takes"""
    n, mu = c["counts"], c["expected"]
    fn = n.astype(np.float32)
    return {"n == 0": n == 0, "0 < n <= 5": (n > 0) & (n <= 5), "n > 5, (float)n <= mu": (n > 5) & (fn <= mu),
            "n > 5, (float)n > mu": (n > 5) & (fn > mu), "n == 2^32 - 1": n == U32_MAX}


# ---- seed candidates ---------------------------------------------------------------------------------------------------
def seed_z(W, thresholds=(10.0, 0.0)):
    """float32[4^W] holding, hashed over the ids: each threshold, one ulp below and above it, +-inf, -0.0, NaN of both
    signs, the smallest denormals and a few ordinary values"""
    f = np.float32
    vals = [f(3.5), f(-5.0), f(1e30), f(np.inf), f(-np.inf), f(-0.0), f(0.0), np.nextafter(f(0), f(1)), np.nextafter(f(0), f(-1))]
    for t in thresholds:
        vals += [f(t), np.nextafter(f(t), f(-np.inf)), np.nextafter(f(t), f(np.inf))]
    bits = np.array(vals, np.float32).view(np.uint32)
    bits = np.concatenate([bits, np.array([0x7FC00000, 0xFFC00000], np.uint32)])  # NaN, -NaN
    x = np.arange(4 ** W, dtype=np.uint32)
    return np.ascontiguousarray(bits[_hash(x ^ np.uint32(0x5BD1E995)) % np.uint32(len(bits))]).view(np.float32)


SEED_THRESHOLDS = ((10.0, 3), (0.0, 0), (-np.inf, 1), (10.0, U32_MAX), (-np.inf, U32_MAX), (-np.inf, 2 ** 32 + 5), (0.0, 2 ** 32 + 5))


def seed_expected(z, counts, z_thr, count_thr):
    """the header's sentence: ids with z >= z_threshold and count >= count_threshold (NaN is not >= anything)"""
    with np.errstate(invalid="ignore"):
        return (z >= np.float32(z_thr)) & (counts.astype(np.uint64) >= np.uint64(count_thr))


# ---- IUPAC ids ---------------------------------------------------------------------------------------------------------
def kmer_iupac_id(x, W):
    """the IUPAC id of the single k-mer x (letters A, C, G, T = 0..3 in both encodings)"""
    return sum(((int(x) >> (2 * i)) & 3) * 11 ** i for i in range(W))


def iupac_ids(W, both, counts, expected):
    """(names, ids uint64) for W = 10 / 12: all-N, exactly 8192 and 16384 members (the first just fits one workgroup's LDS,
    the second is the smallest power of four beyond it), the limit's other neighbours, their own reverse complements, more
    members than any but all-N, and single-k-mer patterns for every value the count table holds -- one anywhere, one where the
    expected count lies closest below the count (z-score at most 2 above a count of 5); small and large mixed."""
    assert W in (10, 12)
    fill = lambda n: "ACGTACGT"[:n]  # noqa: E731
    half = "SWSWSW"[:W // 2]
    inner = "SWSW"[:W // 2 - 2]
    named = [("all_N", "N" * W),
             ("members_8192", "N" * 6 + "S" + fill(W - 7)),
             ("members_16384", "N" * 7 + fill(W - 7)),
             ("members_16384_spread", {10: "NSNWNRNYNA", 12: "NSNWNANCNGNT"}[W]),
             ("members_4096", "N" * 6 + fill(W - 6)),
             ("members_32768", "N" * 7 + "K" + fill(W - 8)),
             ("own_rc_SW", half + half[::-1]),
             ("own_rc_N", "NN" + inner + inner[::-1] + "NN"),
             ("half_of_all", "N" * (W - 1) + "R"),
             ("two_letter_all", "MKRYSWMKRYSW"[:W])]
    names, ids = [], []
    singles = []
    r = revcomp_ids(W)
    x = np.arange(4 ** W, dtype=np.uint32)
    canon = (x <= r) if both else np.ones(4 ** W, bool)
    for v in np.unique(counts):
        at = np.flatnonzero((counts == v) & canon)
        if at.size:
            singles.append(("kmer_count_%d" % int(v), kmer_iupac_id(at[at.size // 3], W)))
            gap = np.float64(v) - expected[at].astype(np.float64)
            if (gap > 0).any():
                singles.append(("kmer_count_%d_near_mu" % int(v), kmer_iupac_id(at[np.argmin(np.where(gap > 0, gap, np.inf))], W)))
    big = [(nm, po.iupac_id(s)) for nm, s in named]
    for nm, s in named:
        assert len(s) == W, (nm, s)
    # interleave: large, small, small, large ...
    while big or singles:
        for src in (big, singles, singles):
            if src:
                nm, i = src.pop(0)
                names.append(nm)
                ids.append(i)
    return names, np.array(ids, np.uint64)


def iupac_members(iupac, W):
    n = 1
    for i in range(W):
        n *= (1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 4)[(int(iupac) // 11 ** i) % 11]
    return n


def iupac_case(W, both, vkind):
    """counts (mirrored under both strands, as callers hand them over), bgp / expected of the sweep case (V, ltot of
    LTOTS[2], k = max_k = 2), the ids and the oracle's rows"""
    c = sweep_case(W, both, (vkind, LTOTS[2], 2, 2, bool(both)))
    names, ids = iupac_ids(W, both, c["counts"], c["expected"])
    c64 = c["counts"].astype(np.uint64)
    want = [po.iupac_aggregate(int(i), W, both, c64, c["bgp"][2], c["expected"]) for i in ids]
    return dict(W=W, both=both, counts=c["counts"], bgp=c["bgp"][2], expected=c["expected"], names=names, ids=ids, want=want)


# ---- motif sets for the similarity grid ----------------------------------------------------------------------------------
MOTIF_LENGTHS = (1, 3, 5, 6, 7, 7, 10, 14, 15, 33, 33, 63, 64, 64)
MAX_MOTIF_LEN = 64
SIM_BG = np.array([0.27, 0.23, 0.21, 0.29], np.float32)


def motif_set():
    """(pwm, comp, lens, sites): 14 motifs of 1 .. 64 columns -- shorter than the 6 overlapping columns a shift needs,
    two pairs of equal length, two of equal site count, rows from Dirichlet(0.3) and Dirichlet(0.05), one of one-hot
    rows (entries exactly 0 and 1); comp = the reverse-complement PWM"""
    rng = np.random.default_rng(2024)
    n = len(MOTIF_LENGTHS)
    lens = np.array(MOTIF_LENGTHS, np.int32)
    pw = np.zeros((n, MAX_MOTIF_LEN, 4), np.float32)
    cp = np.zeros((n, MAX_MOTIF_LEN, 4), np.float32)
    for i in range(n):
        m = rng.dirichlet(np.full(4, 0.3 if i % 2 == 0 else 0.05), size=lens[i]).astype(np.float32)
        if i == n - 1:
            m = np.eye(4, dtype=np.float32)[rng.integers(0, 4, size=lens[i])]
        pw[i, :lens[i]] = m
        cp[i, :lens[i]] = m[::-1, ::-1]
    sites = rng.integers(10, 5000, size=n).astype(np.uint64)
    sites[9] = sites[10]   # equal site counts, equal lengths: the second of the pair is complemented
    sites[2] = sites[12]   # equal site counts, different lengths: the SHORTER motif is complemented
    return pw, cp, lens, sites


def pair_list(n, first_new=0):
    """the order of pengk_motif_similarity's output: j = first_new .. n-1, then i = 0 .. j-1"""
    return [(i, j) for j in range(first_new, n) for i in range(j)]


def n_shift_pairs(li, lj, both):
    """(orientation, shift) pairs of a motif pair: shifts MIN_MERGE_OVERLAP - short .. long - MIN_MERGE_OVERLAP"""
    return (2 if both else 1) * max(li + lj - 2 * 6 + 1, 0)


def fp64_S(p1, c1, s1, p2, c2, s2, both, bg):
    """numpy restatement of the kernel's formula (csrc/similarity.hip): calculate_S in fp64, rounded to float once"""
    eps = np.float64(np.float32(1e-4))
    big, small = (p1, c1, s1), (p2, c2, s2)
    if len(p1) < len(p2):
        big, small = small, big
    lb, ls = len(big[0]), len(small[0])
    y = bg.astype(np.float64) + eps

    def xlgx(v):
        return v * np.log2(v)

    def dbg(m):
        return (xlgx(m) + xlgx(y) - (m + y) * np.log2(0.5 * (m + y))).sum()

    best = -np.inf
    for orient in range(2 if both else 1):
        pb, ps = big[0], small[0]
        if orient == 1:
            if big[2] < small[2]:
                pb = big[1]
            else:
                ps = small[1]
        pb = pb.astype(np.float64) + eps
        ps = ps.astype(np.float64) + eps
        for shift in range(6 - ls, lb - 6 + 1):
            off_s, off_b = -min(shift, 0), max(shift, 0)
            ov = min(lb - off_b, ls - off_s)
            a, b = pb[off_b:off_b + ov], ps[off_s:off_s + ov]
            d = (xlgx(a) + xlgx(b) - (a + b) * np.log2(0.5 * (a + b))).sum()
            best = max(best, 0.5 * (dbg(a) + dbg(b)) - d)
    return np.float32(best)


_exact = {}


def exact_grid(both):
    """_exact_S of every pair of motif_set(), in pair_list order (plain Python: computed once per process)"""
    if both not in _exact:
        pw, cp, lens, sites = motif_set()
        _exact[both] = np.array([_exact_S(pw[i, :lens[i]], cp[i, :lens[i]], sites[i], pw[j, :lens[j]], cp[j, :lens[j]],
                                          sites[j], both, SIM_BG) for i, j in pair_list(len(lens))], np.float32)
    return _exact[both]


def _exact_S(p1, c1, s1, p2, c2, s2, both, bg):
    """IUPACPattern::calculate_S restated with its float32 running sums (src/iupac_pattern.cpp:538-615)."""
    f32, f64 = np.float32, np.float64
    eps = f32(1e-4)

    def term(x, y):
        mean = f32(f32(f32(x + y) + f32(2) * eps) / f32(2))
        return (f64(f32(x + eps)) * np.log2(f64(f32(x + eps))) + f64(f32(y + eps)) * np.log2(f64(f32(y + eps)))
                - f64(f32(f32(2) * mean)) * np.log2(f64(mean)))

    def d(a, b, oa, ob, n):
        acc = f32(0)
        for i in range(n):
            for k in range(4):
                acc = f32(f64(acc) + term(a[oa + i][k], b[ob + i][k]))
        return acc

    def dbg(a, oa, n):
        acc = f32(0)
        for i in range(n):
            for k in range(4):
                acc = f32(f64(acc) + term(a[oa + i][k], bg[k]))
        return acc

    big, small = (p1, c1, s1), (p2, c2, s2)
    if len(p1) < len(p2):
        big, small = small, big
    lb, ls = len(big[0]), len(small[0])
    best = -np.inf
    for orient in range(2 if both else 1):
        pb, ps = big[0], small[0]
        if orient == 1:
            if big[2] < small[2]:
                pb = big[1]
            else:
                ps = small[1]
        for shift in range(6 - ls, lb - 6 + 1):
            off_s, off_b = -min(shift, 0), max(shift, 0)
            ov = min(lb - off_b, ls - off_s)
            sc = f32(0.5 * f64(f32(dbg(pb, off_b, ov) + dbg(ps, off_s, ov))) - f64(d(pb, ps, off_b, off_s, ov)))
            if sc > best:
                best = sc
    return best
