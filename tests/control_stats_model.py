"""The sweep held to a control set's counts (pengk_pattern_stats_control, --discriminative): the definition in numpy on
top of the oracle's Markov probabilities and statistics (oracle.bgprob, oracle.stats), and the constructed cases the
device is compared on.  The definition is this project's own; the reference has no
such mode, so nothing here goes into oracle/.

    q_o[x] = (float) fmax( (double) p_o[x], ((double) c[x] + a) / (double) Lc )        (Lc == 0: q_o[x] = p_o[x])

p_o: the strand-aggregated Markov probability of order o, the bits pengk_pattern_stats writes; c: the control's count
table; Lc: the control's window total; a >= 0: the pseudocount.  Sum and quotient in fp64, ONE rounding to float32.
bgprob[o] = q_o; expected, log-p and z come from q_k, the input's ltot and the input's counts through the oracle's
statistics, unchanged.

tests/test_control_stats_cpu.py asserts that the cases hold the classes they are built for, and that the definition
does what it is for on a planted scenario; tests/test_gpu_control_stats.py compares the device with it."""
import numpy as np

import table_edges_model as tm
from oracle import oracle as po

U32_MAX = 2 ** 32 - 1
PSEUDOCOUNTS = (0.0, 0.5, 1.0)


# ---- the definition --------------------------------------------------------------------------------------------------
def control_share(ctrl, Lc, a):
    """(c + a) / Lc in fp64, per pattern; None when the control is empty"""
    if int(Lc) == 0:
        return None
    return (np.asarray(ctrl).astype(np.float64) + np.float64(a)) / np.float64(int(Lc))


def control_null(p, ctrl, Lc, a):
    """q of one order: float32[4^W]"""
    share = control_share(ctrl, Lc, a)
    p = np.asarray(p, np.float32)
    if share is None:
        return p.copy()
    return np.maximum(p.astype(np.float64), share).astype(np.float32)


def sweep(W, counts, ltot, p, k, ctrl, Lc, a):
    """p: the Markov tables of orders 0..max_k -> (q[0..max_k], expected, logp, z)"""
    q = [control_null(po_, ctrl, Lc, a) for po_ in p]
    e, lp, z = po.stats(W, np.asarray(counts).astype(np.uint64), q[k], int(ltot))
    return q, e, lp, z


# ---- constructed control tables ----------------------------------------------------------------------------------------
# The class of a pattern follows from its id the way the count edges of table_edges_model do (every run of N_CLASSES
# consecutive ids holds every class once, rotated by a hash of the run), with another salt: count edges and control
# classes meet in every combination, and every kind of pattern -- palindromes, both halves of a twin pair, pair tiles and
# own-twin tiles of the twin-tile kernel -- meets every class.
CLASSES = ("c = 0", "c = 1", "c = 2^32 - 1",
           "share == p_k", "p_k Lc rounded down", "p_k Lc rounded up",
           "one float ulp below p_k", "one float ulp above p_k",
           "between p_0 and p_max_k", "share == p_0", "p_max_k Lc rounded up")
N_CLASSES = len(CLASSES)


def lc_exact(W):
    """a power of two at which p Lc - a is an integer below 2^32 for the typical p of a pattern length (p ~ 4^-W with 24
    bits): the control totals at which (c + a) / Lc == p_o can hold in fp64"""
    return 2 ** (2 * W + 24)


def lc_odd(W):
    """of the same size but three times a power of two: p Lc falls on integers and on halves, so that rounding it down and
    up gives shares within a float ulp below and above p as well as equal to it"""
    return 3 * 2 ** (2 * W + 22)


def pattern_class(W, salt=0):
    x = np.arange(4 ** W, dtype=np.uint32)
    rot = tm._hash(x // np.uint32(N_CLASSES) + np.uint32((salt * 0x9E3779B1 + 0x7F4A7C15) & 0xFFFFFFFF)) % np.uint32(N_CLASSES)
    return ((x % np.uint32(N_CLASSES) + rot) % np.uint32(N_CLASSES)).astype(np.int64)


def _clip(v):
    return np.clip(np.nan_to_num(v, nan=0.0, posinf=float(U32_MAX)), 0, U32_MAX).astype(np.uint64).astype(np.uint32)


def control_table(W, p, k, Lc, a, mirrored=False, salt=0):
    """uint32[4^W] for the Markov tables p[0..max_k]: every pattern's control count by its class.  The targets are met
    where the numbers allow it (Lc = 0 or 1 leaves c = 0 / 1 for every derived class; the classes are counted by
    class_masks, not assumed).  As built, twins differ; mirrored: c[rc(x)] = c[x] for x < rc(x)."""
    cls = pattern_class(W, salt)
    L = np.float64(int(Lc))
    a = np.float64(a)
    c = np.zeros(4 ** W, np.uint32)
    c[cls == 1] = 1
    c[cls == 2] = U32_MAX
    f64 = lambda t, at: np.asarray(t, np.float32)[at].astype(np.float64)  # noqa: E731
    below = lambda t, at: np.nextafter(np.asarray(t, np.float32)[at], np.float32(-np.inf)).astype(np.float64)  # noqa: E731
    above = lambda t, at: np.nextafter(np.asarray(t, np.float32)[at], np.float32(np.inf)).astype(np.float64)  # noqa: E731
    for j, target in ((3, lambda at: np.rint(f64(p[k], at) * L - a)),
                      (4, lambda at: np.floor(f64(p[k], at) * L - a)),
                      (5, lambda at: np.ceil(f64(p[k], at) * L - a)),
                      (6, lambda at: np.ceil(below(p[k], at) * L - a)),
                      (7, lambda at: np.floor(above(p[k], at) * L - a)),
                      (8, lambda at: np.rint(0.5 * (f64(p[0], at) + f64(p[-1], at)) * L - a)),
                      (9, lambda at: np.rint(f64(p[0], at) * L - a)),
                      (10, lambda at: np.ceil(f64(p[-1], at) * L - a))):
        at = np.flatnonzero(cls == j)
        c[at] = _clip(target(at))
    if mirrored:
        x = np.arange(4 ** W, dtype=np.uint32)
        r = tm.revcomp_ids(W)
        c = np.where(x < r, c, c[r])
    return np.ascontiguousarray(c, np.uint32)


def class_masks(p, k, ctrl, Lc, a):
    """name -> bool mask: what a case really holds, from the definition alone"""
    share = control_share(ctrl, Lc, a)
    if share is None:
        share = np.full(len(ctrl), -np.inf)
    p64 = [np.asarray(t, np.float32).astype(np.float64) for t in p]
    f32 = np.asarray(p[k], np.float32)
    q = [control_null(t, ctrl, Lc, a) for t in p]
    s32 = share.astype(np.float32)
    return {
        "c = 0": ctrl == 0, "c = 1": ctrl == 1, "c = 2^32 - 1": ctrl == U32_MAX,
        "share == p_k in fp64": share == p64[k],
        "share == p_0 in fp64": share == p64[0],
        "share below p_k by less than a float ulp": (share < p64[k]) & (s32 == f32),
        "share above p_k by less than a float ulp": (share > p64[k]) & (s32 == f32),
        "share rounds one float ulp below p_k": s32 == np.nextafter(f32, np.float32(-np.inf)),
        "share rounds one float ulp above p_k": s32 == np.nextafter(f32, np.float32(np.inf)),
        "control wins at order k": share > p64[k],
        "Markov wins at order k": share < p64[k],
        "Markov wins at order 0, control at order max_k": (share <= p64[0]) & (share > p64[-1]),
        "control wins at order 0, Markov at order max_k": (share > p64[0]) & (share <= p64[-1]),
        "q_k differs from p_k": q[k].view(np.uint32) != f32.view(np.uint32),
    }


def palindromes(W):
    return tm.revcomp_ids(W) == np.arange(4 ** W, dtype=np.uint32)


# ---- cases -------------------------------------------------------------------------------------------------------------
def control_totals(W):
    return (0, 1, 2 ** 40, lc_exact(W), 3_000_017)


def small_cases(W, both):
    """W <= 10: (vkind, ltot, k, max_k, mirrored input, Lc, a, mirrored control).  Every legal (k, max_k) meets every
    control total (W < 10) or two of them in turn (W = 10); the pseudocount, the V kind, the input's ltot and the two table forms rotate, so that over a pattern
    length and strand setting each value of each meets each control total."""
    out = []
    n = 0
    totals = control_totals(W)
    for i, (k, mk) in enumerate(tm.legal_orders(W)):
        # (W = 10: a million patterns a case -- two totals per (k, max_k), every total three times or twice over the six)
        for j, Lc in enumerate(totals if W < 10 else (totals[(2 * i) % 5], totals[(2 * i + 1) % 5])):
            a = PSEUDOCOUNTS[(n + j // 3) % 3]
            out.append(("ac"[n % 2], tm.LTOTS[n % 4], k, mk, n % 4 < 2, Lc, a, bool(both) and n % 3 == 0))
            n += 1
    return out


def big_case(W=12):
    """the one W = 12 case, both strands: mirrored input (what callers hand over), un-mirrored control -- twins with the
    same and with different control counts -- at a total where equality and both neighbours occur, k < max_k"""
    return ("a", tm.LTOTS[2], 1, 2, True, lc_odd(W), 1.0, False)


def case(W, both, spec):
    """dict of one case: inputs, and the model's bgprob[0..max_k] (q), expected, logp, z; `p` the Markov tables"""
    vkind, ltot, k, max_k, mirrored, Lc, a, ctrl_mirrored = spec
    po.set_threads(16)
    try:
        p = [tm.oracle_bgprob(W, vkind, both, o) for o in range(max_k + 1)]
        mu = p[k] * np.float32(ltot)
        step = max(1, mu.size // (1 << 20))
        counts = tm.edge_counts(W, tm.mu_edges(mu[::step]), mirrored, salt=W + 1)
        del mu
        ctrl = control_table(W, p, k, Lc, a, ctrl_mirrored, salt=W)
        q, e, lp, z = sweep(W, counts, ltot, p, k, ctrl, Lc, a)
    finally:
        po.set_threads(1)
    return dict(W=W, both=both, V=tm.sweep_V(vkind), vkind=vkind, ltot=ltot, k=k, max_k=max_k, mirrored=mirrored, counts=counts,
                ctrl=ctrl, Lc=Lc, a=a, ctrl_mirrored=ctrl_mirrored, p=p, bgp=q, expected=e, logp=lp, z=z)


def own_table_case(W, both):
    """a control equal to the input's own table (c = counts, Lc = ltot, a = 1): the expected count is at least n + 1
    wherever the table's count is positive -- nothing is enriched against itself"""
    vkind, ltot, k, max_k = "a", tm.LTOTS[0], min(2, W - 1), min(2, W - 1)
    p = [tm.oracle_bgprob(W, vkind, both, o) for o in range(max_k + 1)]
    counts = tm.edge_counts(W, tm.mu_edges(p[k] * np.float32(ltot)), bool(both), salt=W + 2)
    q, e, lp, z = sweep(W, counts, ltot, p, k, counts, ltot, 1.0)
    return dict(W=W, both=both, V=tm.sweep_V(vkind), vkind=vkind, ltot=ltot, k=k, max_k=max_k, mirrored=bool(both), counts=counts,
                ctrl=counts, Lc=ltot, a=1.0, ctrl_mirrored=bool(both), p=p, bgp=q, expected=e, logp=lp, z=z)


# ---- the planted scenario ----------------------------------------------------------------------------------------------
U_MOTIF = "GGCTGGAGTG"   # in 30 % of the input AND of the control: a contaminant
T_MOTIF = "TGACTCAGCA"   # in 30 % of the input only: the motif
N_SEQ, SEQ_LEN, FRACTION = 2000, 100, 0.3


def encode(s):
    return np.array(["ACGT".index(ch) + 1 for ch in s], np.uint8)


def revcomp_str(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def planted(seed):
    """(input codes, control codes, offsets): 2000 x 100 bp uniform random each (codes 1..4 = A, C, G, T); U planted in
    30 % of both at a uniform position, then T in 30 % of the input (over a planted U where the two meet)"""
    rng = np.random.default_rng(seed)
    sets = []
    for which in ("input", "control"):
        s = rng.integers(1, 5, (N_SEQ, SEQ_LEN)).astype(np.uint8)
        has_u = rng.random(N_SEQ) < FRACTION
        at_u = rng.integers(0, SEQ_LEN - len(U_MOTIF) + 1, N_SEQ)
        for i in np.flatnonzero(has_u):
            s[i, at_u[i]:at_u[i] + len(U_MOTIF)] = encode(U_MOTIF)
        if which == "input":
            has_t = rng.random(N_SEQ) < FRACTION
            at_t = rng.integers(0, SEQ_LEN - len(T_MOTIF) + 1, N_SEQ)
            for i in np.flatnonzero(has_t):
                s[i, at_t[i]:at_t[i] + len(T_MOTIF)] = encode(T_MOTIF)
        sets.append(s.reshape(-1))
    offs = np.arange(N_SEQ + 1, dtype=np.int64) * SEQ_LEN
    return sets[0], sets[1], offs


def shares_6mer(word, motif):
    """does `word` hold a 6-mer of `motif` or of its reverse complement?"""
    subs = {m[i:i + 6] for m in (motif, revcomp_str(motif)) for i in range(len(m) - 5)}
    return any(word[i:i + 6] in subs for i in range(len(word) - 5))


def planted_seeds(seed, W, order=2, a=1.0):
    """the seeds (k-mer strings) the oracle selects on the planted scenario, both strands, default thresholds, under the
    Markov null (model trained on the control, as the CLI trains it on --background-sequences) and under the control's
    counts as a second null; and the largest z of a U-sharing k-mer with count >= 3 under the latter"""
    inp, ctl, offs = planted(seed)
    V = po.bg_V(po.bg_counts(ctl, offs, 2), 2)
    counts, ltot = po.count(inp, offs, W, True)
    ctrl, Lc = po.count(ctl, offs, W, True)
    p = [po.bgprob(W, o, V, True) for o in range(order + 1)]
    _, _, z0 = po.stats(W, counts, p[order], ltot)
    _, _, _, z1 = sweep(W, counts, ltot, p, order, ctrl, Lc, a)
    names = lambda z: [po.kmer_str(int(x), W) for x in po.select(W, z, counts, 10.0, 3, False, True)]  # noqa: E731
    cand = np.flatnonzero(counts >= 3)
    u_z = [float(z1[x]) for x in cand if shares_6mer(po.kmer_str(int(x), W), U_MOTIF)]
    return names(z0), names(z1), (max(u_z) if u_z else float("-inf"))
