"""The GC-stratified null of the sweep (--stratified-background; include/pengk.h, "a GC-stratified null for the sweep";
INTEGRATION.md 7s): the two device entries' definitions in numpy -- on top of the oracle's model, Markov
probabilities and statistics (oracle.bg_V, oracle.bgprob, oracle.stats) and the stratum rule of tests/motif_match_model.py --
the constructed cases, the CLI's report and the scenario of the README's table.  The definitions are this project's own;
the reference has no such mode, so nothing here goes into oracle/.

    counters   for every sequence of stratum s < n_strata, every position p and k in 0..2 with p >= k: the (k+1)-mer ending
               at p counts in bg[s][at_k + y] iff all of its bases are valid; y in BaMM order (older base more significant),
               at_k = 0 / 4 / 20.  windows[s]: the positions with W consecutive valid bases from p on.
    mixture    m_o[x] = (float)( (sum_s (double) w_s (double) p_{s,o}[x]) / (double) sum_s w_s ), the sum in fp64 in ascending
               s over w_s > 0, one division, one rounding; with a control q_o = (float) fmax((double) m_o, share)."""
import numpy as np

import control_stats_model as cm
import motif_match_model as mm
import table_edges_model as tm
from oracle import oracle as po

NONE = mm.NONE
MAX_STRATA = 16
AT = (0, 4, 20)


# ---- entry 1: the counters --------------------------------------------------------------------------------------------------
def gc_strata(seqs, G, all_valid=False):
    """the stratum of every sequence: pengk_seq_strata with gc_bins = G, use_length = 0 (uint16; 0xFFFF without a valid base)"""
    return mm.strata(seqs, G, False, all_valid)[0]


def bg_count(seqs, stratum, n_strata, W, all_valid=False):
    """(bg uint64[n_strata, 84], windows uint64[n_strata]) of byte-code sequences (1..4 = A,C,G,T, else invalid; all_valid:
    an invalid base counts as a valid A, which is what the layout's words hold for it)"""
    bg = np.zeros((n_strata, 84), np.uint64)
    win = np.zeros(n_strata, np.uint64)
    L = np.array([len(c) for c in seqs], np.int64)
    if L.sum() == 0:
        return bg, win
    c = np.concatenate([np.asarray(x, np.int64).reshape(-1) for x in seqs])
    sid = np.repeat(np.arange(len(seqs)), L)
    start = np.repeat(np.cumsum(L) - L, L)
    end = start + np.repeat(L, L)
    pos = np.arange(len(c)) - start
    ok = np.ones(len(c), bool) if all_valid else (c >= 1) & (c <= 4)
    x = np.where((c >= 1) & (c <= 4), c - 1, 0)
    st = np.asarray(stratum, np.int64)[sid]
    use = st < n_strata
    x1, ok1 = np.roll(x, 1), np.roll(ok, 1)
    x2, ok2 = np.roll(x, 2), np.roll(ok, 2)
    flat = bg.reshape(-1)
    for k, (has, y) in enumerate(((use & ok, x), (use & ok & ok1 & (pos >= 1), 4 * x1 + x),
                                   (use & ok & ok1 & ok2 & (pos >= 2), 16 * x2 + 4 * x1 + x))):
        flat += np.bincount(st[has] * 84 + AT[k] + y[has], minlength=flat.size).astype(np.uint64)
    cs = np.concatenate([[0], np.cumsum(ok)])
    p = np.arange(len(c))
    stands = use & (p + W <= end)
    stands[stands] = cs[p[stands] + W] - cs[p[stands]] == W
    win += np.bincount(st[stands], minlength=n_strata).astype(np.uint64)
    return bg, win


# ---- entry 2: the mixture ---------------------------------------------------------------------------------------------------
def mixture(tables, windows):
    """tables: per stratum the float32 table p_s of one order; -> m float32"""
    w = [int(v) for v in windows]
    assert any(w)
    acc = None
    for p, ws in zip(tables, w):
        if ws:
            term = np.float64(ws) * np.asarray(p, np.float32).astype(np.float64)
            acc = term if acc is None else acc + term
    return (acc / np.float64(sum(w))).astype(np.float32)


def sweep(W, counts, ltot, p, windows, k, ctrl=None, Lc=0, a=0.0):
    """p[s][o]: the Markov table of stratum s and order o <= max_k -> (bgprob[0..max_k], expected, logp, z)"""
    max_k = len(p[0]) - 1
    m = [mixture([ps[o] for ps in p], windows) for o in range(max_k + 1)]
    if ctrl is not None:
        m = [cm.control_null(t, ctrl, Lc, a) for t in m]
    e, lp, z = po.stats(W, np.asarray(counts).astype(np.uint64), m[k], int(ltot))
    return m, e, lp, z


def markov_tables(W, Vs, both, max_k, windows=None):
    """p[s][o] = oracle.bgprob(W, o, V_s, both); strata without a window are not evaluated (None)"""
    return [[po.bgprob(W, o, V, both) for o in range(max_k + 1)] if windows is None or int(windows[s]) else [None] * (max_k + 1)
            for s, V in enumerate(Vs)]


# ---- constructed cases for entry 2 ------------------------------------------------------------------------------------------
WEIGHTS = (0, 1, 2 ** 40, 3_000_017)
N_STRATA = (1, 2, 3, 16)


def stratum_V(S):
    """S V tables: the three kinds of tests/table_edges_model.py in turn, from the fourth on the natural one with rows rolled
    -- different models, every one a legal V"""
    out = []
    for s in range(S):
        V = tm.sweep_V("abc"[s % 3]).copy()
        if s >= 3:
            r = s // 3
            V[0:4] = np.roll(V[0:4], r)
            V[4:20] = np.roll(V[4:20].reshape(4, 4), r, axis=1).reshape(-1)
            V[20:84] = np.roll(V[20:84].reshape(16, 4), r, axis=1).reshape(-1)
        out.append(V)
    return np.ascontiguousarray(np.stack(out), np.float32)


def weights(S, n):
    """S weights among WEIGHTS, rotated by n, at least one of them non-zero; n % 5 == 4: exactly one non-zero"""
    w = [WEIGHTS[(n + 3 * s) % 4] for s in range(S)]
    if n % 5 == 4:
        w = [0] * S
        w[n % S] = WEIGHTS[1 + n % 3]
    if not any(w):
        w[-1] = WEIGHTS[3]
    return np.array(w, np.uint64)


def small_cases(W, both):
    """W <= 10: (S, weights, ltot, k, max_k, mirrored input, control?, Lc, a, mirrored control).  Every legal (k, max_k)
    meets every S of N_STRATA (W < 10; W = 10: two of them in turn), with and without a control; the weights, ltot, the
    control's total and pseudocount and the table forms rotate."""
    out = []
    n = 0
    for i, (k, mk) in enumerate(tm.legal_orders(W)):
        for S in (N_STRATA if W < 10 else (N_STRATA[i % 4], N_STRATA[(i + 2) % 4])):
            for control in (False, True):
                totals = cm.control_totals(W)
                out.append((S, weights(S, n), tm.LTOTS[n % 4], k, mk, n % 4 < 2, control, totals[n % 5], cm.PSEUDOCOUNTS[n % 3],
                            bool(both) and n % 3 == 0))
                n += 1
    return out


def big_case(W=12):
    """the one W = 12 case, both strands: three strata, mirrored input, un-mirrored control, k < max_k"""
    return (3, np.array([2 ** 40, 0, 3_000_017], np.uint64), tm.LTOTS[2], 1, 2, True, True, cm.lc_odd(W), 1.0, False)


_tables = {"key": None, "p": None}


def _markov(W, both, S):
    """p[s][o] for stratum_V(S) at max_k = min(2, W - 1), kept for the (W, strand mode, S) in use"""
    key = (W, bool(both), S)
    if _tables["key"] != key:
        _tables["key"], _tables["p"] = key, markov_tables(W, stratum_V(S), both, min(2, W - 1))
    return _tables["p"]


def case(W, both, spec):
    """dict of one case: inputs and the model's bgprob[0..max_k], expected, logp, z"""
    S, w, ltot, k, max_k, mirrored, control, Lc, a, ctrl_mirrored = spec
    po.set_threads(16)
    try:
        p = [ps[:max_k + 1] for ps in _markov(W, both, S)]
        plain = [mixture([ps[o] for ps in p], w) for o in range(max_k + 1)]
        mu = plain[k] * np.float32(ltot)
        step = max(1, mu.size // (1 << 20))
        counts = tm.edge_counts(W, tm.mu_edges(mu[::step]), mirrored, salt=W + 3)
        ctrl = cm.control_table(W, plain, k, Lc, a, ctrl_mirrored, salt=W + 1) if control else None
        m, e, lp, z = sweep(W, counts, ltot, p, w, k, ctrl, Lc, a)
    finally:
        po.set_threads(1)
    return dict(W=W, both=both, S=S, V=stratum_V(S), windows=w, ltot=ltot, k=k, max_k=max_k, mirrored=mirrored, counts=counts,
                ctrl=ctrl, Lc=Lc, a=a if control else 0.0, ctrl_mirrored=ctrl_mirrored, plain=plain, bgp=m, expected=e, logp=lp, z=z)


# ---- what the CLI does ------------------------------------------------------------------------------------------------------
DEFAULT_BINS, DEFAULT_MIN_BASES = 10, 10_000
REPORT_HEADER = "stratum\tgc_lo\tgc_hi\tinput_sequences\tinput_windows\tmodel_bases\tmodel_used\tp_A\tp_C\tp_G\tp_T\n"


def stratified(counted, model_set, W, G=DEFAULT_BINS, min_bases=DEFAULT_MIN_BASES, order=2, alpha=(1.0, 1.0, 1.0), global_V=None,
               strata_of=None):
    """counted: the sequences round 1 counts (byte codes); model_set: the model's source set M.  -> dict: V (G x 84), windows,
    input_sequences, model_bases, own (bool per stratum).  A stratum whose order-0 counters over M sum below min_bases takes
    global_V (default: the oracle's model of all of M).  strata_of: the same sequences as they were read, where `counted`
    holds them behind a mask -- a sequence's stratum is its own, its windows are what is left of it."""
    s_in = gc_strata(counted if strata_of is None else strata_of, G)
    _, windows = bg_count(counted, s_in, G, W)
    bg, _ = bg_count(model_set, gc_strata(model_set, G), G, W)
    if global_V is None:
        global_V = po.bg_V(po.bg_counts(*_flatten(model_set), 2), order, alpha)
    global_V = np.concatenate([global_V, np.zeros(84 - len(global_V), np.float32)])
    bases = bg[:, :4].sum(axis=1)
    own = bases >= np.uint64(min_bases)
    used = sum(4 ** (o + 1) for o in range(order + 1))
    V = np.zeros((G, 84), np.float32)
    for s in range(G):
        if own[s]:
            V[s, :used] = po.bg_V(bg[s, :used].astype(np.int64), order, alpha, wide=True)
        else:
            V[s] = global_V
    return dict(V=V, windows=windows, input_sequences=np.bincount(s_in[s_in < G].astype(np.int64), minlength=G), model_bases=bases,
                own=own, G=G)


def _flatten(seqs):
    offs = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    return (np.concatenate(seqs).astype(np.uint8) if len(seqs) else np.zeros(0, np.uint8)), offs


def report(st):
    """the --stratified-report TSV: one line per stratum, the GC range with three decimals, the order-0 probabilities of the
    model the stratum uses with six"""
    G = st["G"]
    out = [REPORT_HEADER]
    for s in range(G):
        out.append("%d\t%.3f\t%.3f\t%d\t%d\t%d\t%s\t%.6f\t%.6f\t%.6f\t%.6f\n" % (
            s, s / G, (s + 1) / G, int(st["input_sequences"][s]), int(st["windows"][s]), int(st["model_bases"][s]),
            "own" if st["own"][s] else "global", *[float(v) for v in st["V"][s, :4]]))
    return "".join(out)


def stratified_z(counted, model_set, W, both=True, order=2, G=DEFAULT_BINS, min_bases=DEFAULT_MIN_BASES):
    """(counts, z, expected) of the sweep under the stratified null, as the CLI computes them at k = max_k = order"""
    st = stratified(counted, model_set, W, G, min_bases, order)
    counts, ltot = po.count(*_flatten(counted), W, both)
    p = markov_tables(W, st["V"], both, order, st["windows"])
    _, e, _, z = sweep(W, counts, ltot, p, st["windows"], order)
    return counts, z, e


# ---- the scenario of the README's table --------------------------------------------------------------------------------------
MOTIF = "TGACTCAGCA"
N_SEQ, SEQ_LEN, GC_LOW, GC_HIGH, FRACTION = 20_000, 100, 0.30, 0.70, 0.05


def mixed(seed, n=N_SEQ, planted=False, gc=(GC_LOW, GC_HIGH)):
    """n sequences of 100 bp (byte codes), sequence i drawn base by base at gc[i % 2]: one rng.choice(4, 100, p=...) per
    sequence; planted: MOTIF then written over FRACTION of them at a uniform position (drawn after all sequences)"""
    rng = np.random.default_rng(seed)
    seqs = [mm.draw(rng, 1, SEQ_LEN, gc[i % 2])[0] for i in range(n)]
    if planted:
        has = rng.random(n) < FRACTION
        at = rng.integers(0, SEQ_LEN - len(MOTIF) + 1, n)
        for i in np.flatnonzero(has):
            seqs[i][at[i]:at[i] + len(MOTIF)] = cm.encode(MOTIF)
    return seqs


def gc_fraction(word):
    return sum(ch in "CG" for ch in word) / len(word)


def seeds(seqs, W=8, G=DEFAULT_BINS):
    """(Markov seeds, stratified seeds, largest z with count >= 3 under either): k-mer strings the oracle selects on both
    strands at order 2 with its default thresholds (z >= 10, count >= 3, neighbours filtered)"""
    codes, offs = _flatten(seqs)
    counts, ltot = po.count(codes, offs, W, True)
    V = po.bg_V(po.bg_counts(codes, offs, 2), 2)
    _, _, z0 = po.stats(W, counts, po.bgprob(W, 2, V, True), ltot)
    _, z1, _ = stratified_z(seqs, seqs, W, True, 2, G)
    names = lambda z: [po.kmer_str(int(x), W) for x in po.select(W, z, counts, 10.0, 3, False, True)]  # noqa: E731
    top = lambda z: float(z[counts >= 3].max())  # noqa: E731
    return names(z0), names(z1), (top(z0), top(z1))
