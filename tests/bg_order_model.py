"""The Markov null of order K <= 5 for the sweep (include/pengk.h, "a Markov null of order 3 .. 5 for the sweep";
DESIGN.md 29): the three entries' definitions in numpy -- on top of the oracle's Markov probabilities and statistics
(oracle.bgprob, oracle.stats) -- the constructed cases and the scenario of the README's table.  The definitions are this
project's own; the reference's model stops at order 2, so nothing here goes into oracle/.

    counters   for every sequence, every position p and k in 0..K with p >= k: the (k+1)-mer ending at p counts in
               bg[at_k + y] iff all of its bases are valid; y in BaMM order (older base more significant),
               at_k = (4^(k+1) - 4) / 3.
    model      calculateV continued: V_k[y] = (n_k[y] + a_k prior) / (n_{k-1}[y / 4] + a_k), prior = V_{k-1}[y mod 4^k] or 1/4,
               rows of four divided by their sum; float32, every operation rounded on its own.
    sweep      slot max_k of bgprob: the product over i of V_c[x_{i-c} .. x_i], c = min(i, K), float32 in position order
               from 1.0f * v0, p[x] + p[rc x] under both strands (a palindrome once); the slots below: the plain sweep's."""
import numpy as np

import control_stats_model as cm
import table_edges_model as tm
from oracle import oracle as po

MAX_K = 5


def at(k):
    return (4 ** (k + 1) - 4) // 3


def size(K):
    return at(K + 1)


# ---- entry 1: the counters --------------------------------------------------------------------------------------------------
def bg_count(seqs, K, all_valid=False):
    """uint64[size(K)] of byte-code sequences (1..4 = A,C,G,T, else invalid; all_valid: an invalid base counts as a valid
    A, which is what the layout's words hold for it)"""
    bg = np.zeros(size(K), np.uint64)
    L = np.array([len(c) for c in seqs], np.int64)
    if L.sum() == 0:
        return bg
    c = np.concatenate([np.asarray(x, np.int64).reshape(-1) for x in seqs])
    start = np.repeat(np.cumsum(L) - L, L)
    pos = np.arange(len(c)) - start
    good = (c >= 1) & (c <= 4)
    ok = np.ones(len(c), bool) if all_valid else good
    x = np.where(good, c - 1, 0)
    has, y = ok.copy(), x.copy()
    for k in range(K + 1):
        if k:
            has = has & np.roll(ok, k) & (pos >= k)
            y = y + np.roll(x, k) * 4 ** k
        bg[at(k):at(k + 1)] += np.bincount(y[has], minlength=4 ** (k + 1)).astype(np.uint64)
    return bg


# ---- entry 2: the model -----------------------------------------------------------------------------------------------------
def model(counts, K, alpha, interpolate=True):
    """float32[size(K)]; alpha: K + 1 floats"""
    f = np.float32
    n = np.asarray(counts, np.uint64)
    a = np.asarray(alpha, f)
    V = np.zeros(size(K), f)
    V[:4] = (n[:4].astype(f) + a[0] * f(0.25)) / (f(n[:4].sum()) + a[0])
    for k in range(1, K + 1):
        ny, yk = 4 ** (k + 1), 4 ** k
        y = np.arange(ny)
        prior = V[at(k - 1) + y % yk] if interpolate else np.full(ny, 0.25, f)
        with np.errstate(divide="ignore", invalid="ignore"):
            v = (n[at(k) + y].astype(f) + a[k] * prior) / (n[at(k - 1) + y // 4].astype(f) + a[k])
            rows = v.reshape(-1, 4)
            factor = ((f(0.0) + rows[:, 0]) + rows[:, 1] + rows[:, 2]) + rows[:, 3]
            V[at(k):at(k + 1)] = (rows / factor[:, None]).reshape(-1)
    return V


# ---- entry 3: the sweep -----------------------------------------------------------------------------------------------------
def order_prob(W, K, VK, both):
    """float32[4^W]: the order-K probability of every pattern, strand-aggregated when both"""
    VK = np.asarray(VK, np.float32)
    x = np.arange(4 ** W, dtype=np.int64)
    word = x & 3
    p = np.float32(1.0) * VK[word]
    for i in range(1, W):
        c = min(i, K)
        word = ((word << 2) | ((x >> (2 * i)) & 3)) & (4 ** (c + 1) - 1)
        p = p * VK[at(c) + word]
    if both:
        r = tm.revcomp_ids(W)
        p = np.where(r != x, p + p[r], p)
    return p.astype(np.float32)


def sweep(W, both, k, max_k, V, K, VK, counts, ltot, ctrl=None, Lc=0, a=0.0):
    """(bgprob[0..max_k], expected, logp, z) of pengk_pattern_stats_order"""
    m = [po.bgprob(W, o, V, both) for o in range(max_k)] + [order_prob(W, K, VK, both)]
    if ctrl is not None:
        m = [cm.control_null(t, ctrl, Lc, a) for t in m]
    e, lp, z = po.stats(W, np.asarray(counts).astype(np.uint64), m[k], int(ltot))
    return m, e, lp, z


# ---- constructed tables -----------------------------------------------------------------------------------------------------
COUNTER_KINDS = ("random", "zero_contexts", "one_hot_contexts", "near_2_24")
V_KINDS = ("uniform", "dirichlet", "zero_conditional", "one_hot_row", "denormal")


def counters(kind, K, seed=0):
    """uint64[size(K)] counters that are consistent downwards (order k - 1 is the sum over the oldest base of order k, as on
    a long sequence), of the kind named"""
    rng = np.random.default_rng(100 + seed)
    top = rng.integers(1, 2000, 4 ** (K + 1)).astype(np.uint64)
    if kind == "zero_contexts":          # whole rows of four without a count, in every order
        top.reshape(-1, 4)[rng.random(4 ** K) < 0.3] = 0
        top[:4 ** K] = 0
    elif kind == "one_hot_contexts":     # rows with one letter only
        rows = top.reshape(-1, 4)
        keep = rng.integers(0, 4, len(rows))
        hot = rng.random(len(rows)) < 0.5
        mask = np.zeros_like(rows, bool)
        mask[np.arange(len(rows)), keep] = True
        rows[hot[:, None] & ~mask] = 0
    elif kind == "near_2_24":            # where float32 stops holding every integer
        top = (np.uint64(2 ** 24 - 3) + rng.integers(0, 7, 4 ** (K + 1)).astype(np.uint64))
    out = np.zeros(size(K), np.uint64)
    out[at(K):] = top
    for k in range(K - 1, -1, -1):
        out[at(k):at(k + 1)] = out[at(k + 1):at(k + 2)].reshape(4, -1).sum(axis=0)
    return out


def alphas(K, n=0):
    return ((1.0,) * (K + 1), (0.5, 2.0, 10.0, 1.0, 3.0, 0.25)[:K + 1], (1e-3,) * (K + 1))[n % 3]


def sweep_VK(kind, K, seed=0):
    """float32[size(K)] tables of orders 0 .. K of the kind named: every one a model of some counters but for the entries
    set by hand"""
    rng = np.random.default_rng(200 + seed)
    if kind == "uniform":
        return np.full(size(K), 0.25, np.float32)
    V = np.concatenate([rng.dirichlet([2.0] * 4, 4 ** k).astype(np.float32).reshape(-1) for k in range(K + 1)])
    if kind == "zero_conditional":
        V[rng.random(len(V)) < 0.1] = 0.0
        V[at(K)] = 0.0
    elif kind == "one_hot_row":
        for k in range(K + 1):
            rows = V[at(k):at(k + 1)].reshape(-1, 4)
            rows[::3] = 0.0
            rows[::3, k % 4] = 1.0
    elif kind == "denormal":
        V[::7] = np.float32(1e-40)
        V[at(K) + 1] = np.float32(1e-45)
    return V


SWEEP_KS = (0, 2, 3, 4, 5)


def small_cases(W, both):
    """W <= 10: (K, V kind, ltot, k, max_k, mirrored input, control?, Lc, a, mirrored control).  Every legal (k, max_k) meets
    every K of SWEEP_KS, with and without a control in turn (five orders: the turn shifts from one (k, max_k) to the next);
    the V kinds, ltot, the control's total and pseudocount and the table forms rotate."""
    out = []
    n = 0
    for i, (k, mk) in enumerate(tm.legal_orders(W)):
        for K in SWEEP_KS:
            totals = cm.control_totals(W)
            out.append((K, V_KINDS[(n + i) % 5], tm.LTOTS[n % 4], k, mk, n % 4 < 2, n % 2 == 1, totals[n % 5], cm.PSEUDOCOUNTS[n % 3],
                        bool(both) and n % 3 == 0))
            n += 1
    return out


def big_case(W=12):
    """the one W = 12 case, both strands: K = 5, mirrored input, un-mirrored control, k < max_k"""
    return (5, "dirichlet", tm.LTOTS[2], 1, 2, True, True, cm.lc_odd(W), 1.0, False)


_low = {}


def _low_slots(W, both, max_k):
    """the plain sweep's tables of orders below max_k for the run's own model (kind "a" of tests/table_edges_model.py)"""
    for o in range(max_k):
        if (W, bool(both), o) not in _low:
            _low[(W, bool(both), o)] = po.bgprob(W, o, tm.sweep_V("a"), both)
    return [_low[(W, bool(both), o)] for o in range(max_k)]


def case(W, both, spec):
    """dict of one case: inputs and the model's bgprob[0..max_k], expected, logp, z"""
    K, kind, ltot, k, max_k, mirrored, control, Lc, a, ctrl_mirrored = spec
    po.set_threads(16)
    try:
        VK = sweep_VK(kind, K, seed=W)
        plain = _low_slots(W, both, max_k) + [order_prob(W, K, VK, both)]
        mu = plain[k] * np.float32(ltot)
        step = max(1, mu.size // (1 << 20))
        counts = tm.edge_counts(W, tm.mu_edges(mu[::step]), mirrored, salt=W + 3)
        ctrl = cm.control_table(W, plain, k, Lc, a, ctrl_mirrored, salt=W + 1) if control else None
        m = [cm.control_null(t, ctrl, Lc, a) for t in plain] if control else plain
        e, lp, z = po.stats(W, counts.astype(np.uint64), m[k], int(ltot))
    finally:
        po.set_threads(1)
    return dict(W=W, both=both, K=K, kind=kind, V=tm.sweep_V("a"), VK=VK, ltot=ltot, k=k, max_k=max_k, mirrored=mirrored,
                counts=counts, ctrl=ctrl, Lc=Lc, a=a if control else 0.0, ctrl_mirrored=ctrl_mirrored, bgp=m, expected=e, logp=lp,
                z=z)


# ---- the scenario of the README's table --------------------------------------------------------------------------------------
MOTIF = "TGACTCAGCA"
N_SEQ, SEQ_LEN, CHAIN_ORDER, FRACTION = 20_000, 100, 4, 0.05


def chain(seed, n=N_SEQ, planted=False):
    """n sequences of SEQ_LEN bp (byte codes 1..4) from a random order-4 chain.  rng = np.random.default_rng(seed), the calls
    in this order: rng.dirichlet([8, 8, 8, 8], 256) (the conditionals of the 256 contexts, context = the four bases behind,
    older base more significant); rng.integers(0, 4, (n, 4)) (the first four bases); then for every position 4 .. 99 ONE
    rng.random(n), the base of sequence i being the number of the context's cumulative probabilities (float64 cumsum, the
    first three) that are <= the draw.  planted: then rng.random(n) < FRACTION picks the sequences and
    rng.integers(0, SEQ_LEN - 10 + 1, n) the places where MOTIF is written over them."""
    rng = np.random.default_rng(seed)
    T = rng.dirichlet([8.0] * 4, 4 ** CHAIN_ORDER)
    cum = np.cumsum(T, axis=1)[:, :3]
    s = np.zeros((n, SEQ_LEN), np.int64)
    s[:, :CHAIN_ORDER] = rng.integers(0, 4, (n, CHAIN_ORDER))
    ctx = np.zeros(n, np.int64)
    for j in range(CHAIN_ORDER):
        ctx = ctx * 4 + s[:, j]
    for t in range(CHAIN_ORDER, SEQ_LEN):
        u = rng.random(n)
        b = (cum[ctx] <= u[:, None]).sum(axis=1)
        s[:, t] = b
        ctx = (ctx * 4 + b) % 4 ** CHAIN_ORDER
    codes = (s + 1).astype(np.uint8)
    if planted:
        has = rng.random(n) < FRACTION
        where = rng.integers(0, SEQ_LEN - len(MOTIF) + 1, n)
        for i in np.flatnonzero(has):
            codes[i, where[i]:where[i] + len(MOTIF)] = cm.encode(MOTIF)
    return [codes[i] for i in range(n)]


def _flatten(seqs):
    offs = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    return (np.concatenate(seqs).astype(np.uint8) if len(seqs) else np.zeros(0, np.uint8)), offs


def shares_6mer(word):
    """does `word` hold a 6-mer of MOTIF or of its reverse complement?"""
    return cm.shares_6mer(word, MOTIF)


# ---- what the CLI does ------------------------------------------------------------------------------------------------------
REPORT_HEADER = "order\tcontexts\tcontexts_seen\tmin_count\tmedian_count\n"


def cli_model(model_set, K, alpha_high=1.0):
    """(counters, VK) of --high-order-background K over the model's source set as it was read: alpha 1 at orders 0 .. 2 (the
    run's default), alpha_high above, interpolated"""
    n = bg_count(model_set, K)
    return n, model(n, K, (1.0, 1.0, 1.0)[:min(K, 2) + 1] + (alpha_high,) * max(0, K - 2))


def contexts(n, k):
    """the counts of the contexts of order k: the k-mers, i.e. the counters of order k - 1; order 0 has one, every base"""
    return np.array([n[:4].sum()], np.uint64) if k == 0 else n[at(k - 1):at(k)]


def report(n, K):
    """the --high-order-report TSV: one line per order; the median is the lower one (sorted ascending, place (n - 1) / 2)"""
    out = [REPORT_HEADER]
    for k in range(K + 1):
        c = np.sort(contexts(n, k))
        out.append("%d\t%d\t%d\t%d\t%d\n" % (k, len(c), np.count_nonzero(c), int(c[0]), int(c[(len(c) - 1) // 2])))
    return "".join(out)


def stdout_line(n, K, alpha_high=1.0):
    return "high-order background: order %d, alpha %g, %d model bases, %d of %d contexts seen" % (
        K, alpha_high, int(n[:4].sum()), np.count_nonzero(contexts(n, K)), 4 ** K)


def cli_sweep(counted, model_set, W, K, both=True, alpha_high=1.0, ctrl=None, Lc=0, a=0.0):
    """(counts, expected, z, VK) as the CLI computes them at k = max_k = 2: the oracle's counts of `counted`, the one model
    and the order-K model of `model_set`"""
    counts, ltot = po.count(*_flatten(counted), W, both)
    n, VK = cli_model(model_set, K, alpha_high)
    V = po.bg_V(po.bg_counts(*_flatten(model_set), 2), 2)
    _, e, _, z = sweep(W, both, 2, 2, V, K, VK, counts, ltot, ctrl, Lc, a)
    return counts, e, z, VK


def order_z(seqs, W, K, alpha_high=1.0, both=True):
    """(counts, z) of the sweep as --high-order-background K computes it on an input that is its own background set"""
    counts, _, z, _ = cli_sweep(seqs, seqs, W, K, both, alpha_high)
    return counts, z


def seeds(seqs, W, K):
    """(seed words, largest z among words that share a 6-mer with MOTIF and have count >= 3): what the oracle selects on both
    strands with its default thresholds (z >= 10, count >= 3, neighbours filtered) under the order-K null"""
    counts, z = order_z(seqs, W, K)
    names = [po.kmer_str(int(x), W) for x in po.select(W, z, counts, 10.0, 3, False, True)]
    with_motif = [float(z[x]) for x in np.flatnonzero(counts >= 3) if shares_6mer(po.kmer_str(int(x), W))]
    return names, (max(with_motif) if with_motif else float("nan"))
