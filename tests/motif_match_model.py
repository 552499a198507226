"""numpy restatement of the control matching (--score-negatives control; include/pengk.h, "a control set matched to the
input"): the stratum of a sequence (half-octave length bin x GC bin), the quotas per stratum, the evenly
spaced selection by stable rank, the report the CLI writes, and the scenario of the README's table.  Everything is
integer, so the device must agree with it bit for bit."""
import numpy as np

NONE = 0xFFFF
N_STRATA = 256


# ---- strata ------------------------------------------------------------------------------------------------------------------
def length_bin(L):
    """clamp(2 floor(log2 L) + (the bit of L below its top bit) - 10, 0, 15), L >= 1"""
    l = int(L).bit_length() - 1
    sub = (int(L) >> (l - 1)) & 1 if l else 0
    return min(15, max(0, 2 * l + sub - 10))


def stratum_of(codes, G, use_length, all_valid=False):
    """one sequence of byte codes (1..4 = A,C,G,T, else invalid; all_valid: an invalid base counts as a valid A)"""
    c = np.asarray(codes)
    n = len(c) if all_valid else int(((c >= 1) & (c <= 4)).sum())
    if n == 0:
        return NONE
    gc = int(((c == 2) | (c == 3)).sum())
    g = min(G - 1, (gc * G) // n)
    return (length_bin(len(c)) if use_length else 0) * G + g


def strata(seqs, G=10, use_length=True, all_valid=False):
    """(stratum per sequence as uint16, the 256 counts as uint64): stratum_of for all sequences at once"""
    L = np.array([len(c) for c in seqs], np.int64)
    c = np.concatenate([np.asarray(x, np.int64).reshape(-1) for x in seqs] + [np.zeros(0, np.int64)])
    ends = np.cumsum(L)
    def per_sequence(mask):
        cs = np.concatenate([[0], np.cumsum(mask)])
        return cs[ends] - cs[ends - L]
    n = L.copy() if all_valid else per_sequence((c >= 1) & (c <= 4))
    gc = per_sequence((c == 2) | (c == 3))
    g = np.minimum(G - 1, (gc * G) // np.maximum(n, 1))
    l = np.frexp(np.maximum(L, 1).astype(np.float64))[1].astype(np.int64) - 1  # floor(log2 L), exact below 2^53
    h = 2 * l + np.where(l > 0, (L >> np.maximum(l - 1, 0)) & 1, 0) - 10
    lb = np.clip(h, 0, 15) if use_length else 0
    s = np.where(n > 0, lb * G + g, NONE).astype(np.uint16)
    return s, histogram(s)


def histogram(s):
    s = np.asarray(s, np.int64)
    return np.bincount(s[s < N_STRATA], minlength=N_STRATA).astype(np.uint64)


def length_range(lb):
    """[lo, hi] of the lengths of bin lb (hi None: no upper end)"""
    def first(h):  # the smallest L with 2 l + sub = h
        return (2 + (h & 1)) << ((h >> 1) - 1) if h >= 2 else 1
    lo = 1 if lb == 0 else first(lb + 10)
    return lo, (None if lb == 15 else first(lb + 11) - 1)


# ---- quotas ------------------------------------------------------------------------------------------------------------------
def quotas(h_in, h_ctrl, ratio=1):
    """(quota per stratum, shortfall), Python integers underneath"""
    q = [min(int(c), ratio * int(a)) for a, c in zip(h_in, h_ctrl)]
    return np.array(q, np.uint64), sum(ratio * int(a) - x for a, x in zip(h_in, q))


# ---- selection ---------------------------------------------------------------------------------------------------------------
def kept_rank(r, q, c):
    return ((r + 1) * q) // c > (r * q) // c


def select(s, count, quota, rank0=None):
    """the indices (ascending) of the kept entries of s: entry i of stratum t < 256 has the rank r = rank0[t] + the entries
    before it with the same stratum and is kept iff kept_rank(r, quota[t], count[t])"""
    s = np.asarray(s, np.int64)
    keep = np.zeros(len(s), bool)
    for t in np.unique(s[s < N_STRATA]):
        at = np.flatnonzero(s == t)
        q, c = int(quota[t]), int(count[t])
        r0 = int(rank0[t]) if rank0 is not None else 0
        if c == 0:
            continue
        if (r0 + len(at) + 1) * max(q, 1) < 2 ** 62:
            r = np.arange(len(at), dtype=np.int64) + r0
            keep[at] = (r < c) & (((r + 1) * q) // c > (r * q) // c)
        else:  # Python integers
            keep[at] = [x < c and kept_rank(x, q, c) for x in range(r0, r0 + len(at))]
    return np.flatnonzero(keep)


# ---- the report --------------------------------------------------------------------------------------------------------------
REPORT_HEADER = "length_min\tlength_max\tgc_min\tgc_max\tinput\tcontrol\tkept\n"


def report(h_in, h_ctrl, quota, G, use_length):
    """the --control-match-report TSV: one line per stratum with an input or a control sequence, strata ascending; GC bin g
    of G covers [g / G, (g + 1) / G) (the last one up to 1), printed with three decimals; without length matching the
    length range is 1 .. inf"""
    out = [REPORT_HEADER]
    for t in range(N_STRATA):
        if not (int(h_in[t]) or int(h_ctrl[t])):
            continue
        lb, g = divmod(t, G)
        lo, hi = length_range(lb) if use_length else (1, None)
        out.append("%d\t%s\t%.3f\t%.3f\t%d\t%d\t%d\n" % (lo, "inf" if hi is None else str(hi), g / G, (g + 1) / G, int(h_in[t]),
                                                         int(h_ctrl[t]), int(quota[t])))
    return "".join(out)


# ---- the scenario of the README's table --------------------------------------------------------------------------------------
GC_RICH_8MER = "GCCGCGGC"


def draw(rng, n, length, gc):
    """n sequences of byte codes (A,C,G,T = 1..4), every base C or G with probability gc"""
    p = [(1 - gc) / 2, gc / 2, gc / 2, (1 - gc) / 2]
    return [rng.choice(4, size=int(L), p=p).astype(np.uint8) + 1 for L in np.broadcast_to(length, n)]


def scenario(seed, n_in=2000, n_ctrl=6000):
    """(input, control): the input n_in x 100 bp at 60 % GC with nothing planted; the control n_ctrl sequences, every one
    at 30 % or 60 % GC and of 100 or 300 bp with equal chances, in random order"""
    rng = np.random.default_rng(seed)
    pos = draw(rng, n_in, 100, 0.60)
    gcs = np.where(rng.random(n_ctrl) < 0.5, 0.30, 0.60)
    lens = np.where(rng.random(n_ctrl) < 0.5, 100, 300)
    ctrl = [draw(rng, 1, L, g)[0] for L, g in zip(lens, gcs)]
    return pos, ctrl


# ---- the scenario of the match modes -----------------------------------------------------------------------------------------
EDGE_LENGTHS = [30, 47, 48, 6143, 6144, 7000]  # length bins 0, 0 | 1, 14 | 15, 15: both ends of the half-octave scale
EDGE_SEED = 98  # (the edge sequences have a generator of their own: scenario(seed) stays what it is)

# (name, the CLI's flags, match by GC, match by length, G, ratio)
MODES = [
    ("default", [], True, True, 10, 1),
    ("gc4_r3", ["--control-match", "gc", "--control-match-gc-bins", "4", "--control-ratio", "3"], True, False, 4, 3),
    ("length_r2", ["--control-match", "length", "--control-ratio", "2"], False, True, 1, 2),
    ("both16_r3", ["--control-match-gc-bins", "16", "--control-ratio", "3"], True, True, 16, 3),
    ("gc1", ["--control-match", "gc", "--control-match-gc-bins", "1"], True, False, 1, 1),
]


def mode_scenario(seed):
    """(input, control): scenario(seed) and, behind it, sequences of the lengths at which the length bins begin and end
    (EDGE_LENGTHS) at 60 % GC -- three of each in the input, then two of each in the control"""
    pos, ctrl = scenario(seed)
    rng = np.random.default_rng(EDGE_SEED + seed)
    pos = pos + [c for L in EDGE_LENGTHS for c in draw(rng, 3, L, 0.60)]
    ctrl = ctrl + [c for L in EDGE_LENGTHS for c in draw(rng, 2, L, 0.60)]
    return pos, ctrl


def match(pos, ctrl, gc=True, length=True, G=10, ratio=1):
    """what the CLI does with one mode: a dict of h_in, h_ctrl, quota, short, kept (indices into ctrl) and in_use.
    Without GC matching there is one GC bin, whatever --control-match-gc-bins says."""
    G = G if gc else 1
    _, h_in = strata(pos, G, length)
    s_ctrl, h_ctrl = strata(ctrl, G, length)
    quota, short = quotas(h_in, h_ctrl, ratio)
    return dict(h_in=h_in, h_ctrl=h_ctrl, quota=quota, short=short, kept=select(s_ctrl, h_ctrl, quota),
                in_use=int((h_in > 0).sum()), G=G, use_length=length, ratio=ratio)


def stdout_line(name, m, n_ctrl):
    """the CLI's line on stdout for the mode `name` ("gc,length", "gc" or "length") and the result m of match()"""
    return "control negatives: matched by %s (%d GC bin%s, ratio %d): %d strat%s in use, kept %d of %d control sequences, shortfall %d" % (
        name, m["G"], "" if m["G"] == 1 else "s", m["ratio"], m["in_use"], "um" if m["in_use"] == 1 else "a", len(m["kept"]),
        n_ctrl, m["short"])


def front_loaded(ctrl, h_in, G=10, use_length=True):
    """(the control reordered, n): the n sequences of a stratum the input uses first, the others behind them, each group
    in its old order.  Read by several ranks (byte ranges), the later ranks' shards then hold nothing to keep."""
    s, _ = strata(ctrl, G, use_length)
    used = (s < N_STRATA) & (np.asarray(h_in)[np.minimum(s, N_STRATA - 1)] > 0)
    order = np.concatenate([np.flatnonzero(used), np.flatnonzero(~used)])
    return [ctrl[i] for i in order], int(used.sum())


def word_pwm(word, p=0.85):
    """a PWM (w x 4) with probability p on the word's letter of every column"""
    out = np.full((len(word), 4), (1 - p) / 3)
    for j, ch in enumerate(word):
        out[j, "ACGT".index(ch)] = p
    return out
