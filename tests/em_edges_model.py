"""Constructed inputs that put the EM kernels (csrc/em.hip, em_serial.h, em_fused.hip, em_legacy.hip, seqsum.h) at their
value edges -- pure numpy; shared by tests/test_em_edges_cpu.py (which asserts that the cases are what they claim to be,
with the oracle alone) and tests/test_gpu_em_edges.py (which runs them on the device against the oracle).

Every builder returns a list of dicts: W, counts (uint32[4^W]), bg (float32[4^W]), pwms (float32[n, W, 4]), saturation,
threshold, max_iter, tag -- and, for class G, `ladder` (its name), `form` ("pow2" / "mant"), `division`, `inequality`,
`shadowed`, and `rungs` (per PWM the ladder position, None for a PWM that is not a rung).  PWM rows need not sum to 1:
neither the kernels nor the reference (src/peng.cpp:104-144, 180-197) require it.

Class G, the guard ladders.  With PWM entries 2^e (product 2^P in every k-mer), a constant background 2^B and a
saturation 2^S, the ranges lean_ranges_ok derives are exact: p in [2^(P-1), 2^(P+1)], odds in [2^(P-B-2), 2^(P-B+2)],
t_hi = 2^(S-(P-B)+3), c s in [2^(S-1), 2^(S+33)], 1 + t in [1, 2^(S-(P-B)+4)].  The four inequalities of lean_div_ok
(I1: eb_hi <= 251, I2: ea_lo >= 25, I3: ea_hi - eb_lo <= 94, I4: ea_lo - eb_hi >= -123) then read
    pr / bg        I1  B <= 124       I2  P >= -101      I3  P - B <= 93           I4  P - B >= -122
    s / odds       I1  P - B <= 122   I2  S >= -102      I3  S - (P - B) <= 92     I4  S - (P - B) >= -121
    c s / (1 + t)  I1  S - (P - B) <= 120   I2  S >= -101   I3  S <= 61            I4  P - B >= -118  (t_hi >= 1)
Four of the twelve are implied by another one (`shadowed`: D1-I4 by D3-I4, D2-I1 by D1-I3, D2-I2 by D3-I2, D3-I1 by
D2-I3): their ladders straddle the inequality all the same, on the plain side of the guard as a whole.  Each ladder
moves ONE quantity a binade at a time -- the exponent of one PWM column (all rungs in one call, one PWM per rung), the
exponent of the background table, or the saturation (one call per rung) -- three rungs on the failing side, four on the
passing side; in the "mant" form every PWM entry, the two background values and the saturation carry random 23-bit
mantissas on the same exponents, the ladder is placed where the restated guard's inequality flips for them.

Oracle time at W = 12 (one thread, this suite's build of oracle/peng_oracle.cpp): 0.70 s per PWM-iteration; the W = 12
selection is 33 PWM-iterations (w12_budget)."""
import numpy as np

from oracle import oracle as po

FLT_MAX = np.float32(3.4028234663852886e38)
WS = (2, 4, 6, 8, 10, 12)


# ---- the guard, restated ---------------------------------------------------------------------------------------------
def _bits(x):
    return int(np.float32(x).view(np.uint32))


def _fin(x):
    """normal, finite, positive"""
    return ((_bits(x) - 0x00800000) & 0xFFFFFFFF) < 0x7F000000


def lean_div_detail(a_lo, a_hi, b_lo, b_hi):
    """(fin, I1, I2, I3, I4) of lean_div_ok, each evaluated on its own"""
    fin = all(_fin(v) for v in (a_lo, a_hi, b_lo, b_hi)) and not (a_lo > a_hi) and not (b_lo > b_hi)
    ea_lo, ea_hi, eb_lo, eb_hi = (_bits(v) >> 23 & 0x1FF for v in (a_lo, a_hi, b_lo, b_hi))
    return (fin, eb_hi <= 251, ea_lo >= 25, ea_hi - eb_lo <= 94, ea_lo - eb_hi >= -123)


def bg_range(bg):
    """{min, max} of a background table the way em_bg_range_kernel takes them: of the float BITS"""
    b = np.ascontiguousarray(bg, np.float32).view(np.uint32)
    return np.array([b.min(), b.max()], np.uint32).view(np.float32)


def lean_ranges_detail(pwm, bg_lo, bg_hi, saturation):
    """The pieces of lean_ranges_ok: {"positive", "background", 1: (fin, I1..I4), 2: ..., 3: ...} in float32."""
    f = np.float32
    pwm = np.asarray(pwm, f)
    s = f(saturation)
    out = {"positive": bool((pwm > 0).all()), "background": _bits(bg_hi) <= 0x7F7FFFFF and bool(s > 0)}
    if not out["positive"]:
        return out
    with np.errstate(all="ignore"):
        p_lo = p_hi = f(1.0)
        for p in range(pwm.shape[0]):
            p_lo = f(p_lo * pwm[p].min())
            p_hi = f(p_hi * pwm[p].max())
        p_lo, p_hi = f(p_lo * f(0.5)), f(p_hi * f(2.0))
        b_lo, b_hi = f(bg_lo), f(bg_hi)
        out[1] = lean_div_detail(p_lo, p_hi, b_lo, b_hi)
        o_lo, o_hi = f(f(p_lo / b_hi) * f(0.5)), f(f(p_hi / b_lo) * f(2.0))
        out[2] = lean_div_detail(s, s, o_lo, o_hi)
        t_hi = f(f(s / o_lo) * f(2.0))
        out[3] = lean_div_detail(f(s * f(0.5)), f(s * f(8589934592.0)), f(1.0), f(f(f(1.0) + t_hi) * f(2.0)))
    return out


def lean_ranges_ok(pwm, bg_lo, bg_hi, saturation):
    """A plain float32 restatement of lean_ranges_ok / lean_div_ok (csrc/em_serial.h:131-160): may the workgroups of this
    PWM run the three divisions of a weight without range scaling?

    A COVERAGE CERTIFICATE ONLY.  It places the ladders of class G and lets tests/test_em_edges_cpu.py prove that every
    ladder has cases on both sides of its inequality; no assertion about the device depends on it -- those compare with
    the oracle alone, whichever side of the guard a case lies on."""
    d = lean_ranges_detail(pwm, bg_lo, bg_hi, saturation)
    return d["positive"] and d["background"] and all(all(d[k]) for k in (1, 2, 3))


# ---- common pieces ---------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng([977] + [int(k) for k in key])


def small_counts(W, salt=0):
    """random small integers, a third of the entries zero"""
    rng = _rng(1, W, salt)
    c = rng.integers(1, 8, 4 ** W).astype(np.uint32)
    c[rng.random(4 ** W) < 1.0 / 3.0] = 0
    return c


def healthy_bg(W, salt=0):
    return (_rng(2, W, salt).uniform(0.5, 1.5, 4 ** W) * 4.0 ** -W).astype(np.float32)


def healthy_pwms(W, n, salt=0, conc=2.0):
    return _rng(3, W, salt).dirichlet(np.full(4, conc), size=(n, W)).astype(np.float32)


def _case(W, counts, bg, pwms, saturation, threshold, max_iter, tag, **more):
    c = dict(W=W, counts=np.ascontiguousarray(counts, np.uint32), bg=np.ascontiguousarray(bg, np.float32),
             pwms=np.ascontiguousarray(pwms, np.float32).reshape(-1, W, 4), saturation=float(np.float32(saturation)),
             threshold=float(threshold), max_iter=int(max_iter), tag=tag)
    assert c["counts"].shape == c["bg"].shape == (4 ** W,)
    c.update(more)
    return c


def digit(x, p):
    return (int(x) >> (2 * p)) & 3


# ---- class G ---------------------------------------------------------------------------------------------------------
# name: (division, inequality, what moves, P, B, S at the crossing's passing side (powers of two), shadowed by)
LADDERS = {
    "D1-I1": (1, 1, "B", 84, 124, 13, None),
    "D1-I2": (1, 2, "P", -101, 0, -40, None),
    "D1-I3": (1, 3, "P", 33, -60, 0, None),
    "D1-I4": (1, 4, "P", -62, 60, -40, "D3-I4"),
    "D2-I1": (2, 1, "P", 62, -60, 0, "D1-I3"),
    "D2-I2": (2, 2, "S", -8, 0, -102, "D3-I2"),
    "D2-I3": (2, 3, "P", -52, 0, 40, None),
    "D2-I4": (2, 4, "P", 61, 0, -60, None),
    "D3-I1": (3, 1, "P", -80, 0, 40, "D2-I3"),
    "D3-I2": (3, 2, "S", -8, 0, -101, None),
    "D3-I3": (3, 3, "S", -8, 0, 61, None),
    "D3-I4": (3, 4, "P", -58, 60, -40, None),
}
W12_LADDERS = ("D1-I2", "D2-I3", "D3-I4")  # one per division
FAIL_RUNGS, PASS_RUNGS = 3, 4
MORE_FAIL_RUNGS = {}  # ladder: rungs on the failing side, where three do not reach a rung that a too generous guard turns red


def fail_rungs(name):
    return MORE_FAIL_RUNGS.get(name, FAIL_RUNGS)


def _column_exponents(W, P):
    e = np.full(W, P // W, np.int64)
    e[:P - int(e.sum())] += 1
    return e


def _ladder_parts(name, W, form):
    """the unscaled PWM mantissas, the two background mantissas, the saturation's mantissa"""
    if form == "pow2":
        return np.ones((W, 4)), (1.0, 1.0), 1.0
    rng = _rng(4, W, sorted(LADDERS).index(name))
    m = 1.0 + rng.integers(0, 1 << 23, (W, 4)) / float(1 << 23)
    b = 1.0 + rng.integers(0, 1 << 23, 2) / float(1 << 23)
    return m, (float(b.min()), float(b.max())), 1.0 + int(rng.integers(0, 1 << 23)) / float(1 << 23)


def _ladder_point(name, W, form, k):
    """rung k of a ladder (k counts binades of the moving quantity from the nominal crossing): (pwm, b_lo, b_hi, s)"""
    div, ineq, moves, P, B, S, _ = LADDERS[name]
    m, (mb_lo, mb_hi), ms = _ladder_parts(name, W, form)
    e = _column_exponents(W, P)
    if moves == "P":
        e[0] += k
    elif moves == "B":
        B += k
    else:
        S += k
    with np.errstate(over="ignore"):  # (the far rungs of the search may pass 2^128)
        pwm = np.ldexp(m, e[:, None]).astype(np.float32)
        return pwm, np.float32(np.ldexp(mb_lo, B)), np.float32(np.ldexp(mb_hi, B)), np.float32(np.ldexp(ms, S))


def ladder_rungs(name, W, form):
    """[(k, position)]: the 3 + 4 rungs around the place where the ladder's inequality flips, position < 0 on the failing
    side (-1 next to the edge), >= 0 on the passing side"""
    div, ineq = LADDERS[name][:2]
    holds = {}
    for k in range(-24, 25):
        pwm, b_lo, b_hi, s = _ladder_point(name, W, form, k)
        holds[k] = lean_ranges_detail(pwm, b_lo, b_hi, s)[div][ineq]
    flips = [k for k in range(-24, 24) if holds[k] != holds[k + 1]]
    assert len(flips) == 1, (name, W, form, flips)
    k0 = flips[0]
    if holds[k0]:  # passing below the edge (an upper bound on the moving quantity)
        return [(k0 + 1 + j, -1 - j) for j in range(fail_rungs(name))][::-1] + [(k0 - j, j) for j in range(PASS_RUNGS)]
    return [(k0 - j, -1 - j) for j in range(fail_rungs(name))][::-1] + [(k0 + 1 + j, j) for j in range(PASS_RUNGS)]


def _ladder_bg(W, b_lo, b_hi, salt):
    if b_lo == b_hi:
        return np.full(4 ** W, b_lo, np.float32)
    return np.where(_rng(5, W, salt).random(4 ** W) < 0.5, b_lo, b_hi).astype(np.float32)


def guard_ladder(name, W, form, max_iter=1):
    div, ineq, moves, _, _, _, shadowed = LADDERS[name]
    rungs = ladder_rungs(name, W, form)
    more = dict(ladder=name, form=form, division=div, inequality=ineq, shadowed=shadowed, cls="G")
    counts = small_counts(W)
    tag = "G/%s/%s/W%d" % (name, form, W)
    if moves == "P":  # one call: a PWM per rung, and two ordinary PWMs behind them (a group of eight and a remainder)
        pts = [_ladder_point(name, W, form, k) for k, _ in rungs]
        extra = 2 if W < 12 else 0  # (W = 12: the rungs alone, for the oracle's sake)
        pwms = np.stack([p[0] for p in pts] + list(healthy_pwms(W, extra, salt=div * 10 + ineq)))
        _, b_lo, b_hi, s = pts[0]
        return [_case(W, counts, _ladder_bg(W, b_lo, b_hi, div * 10 + ineq), pwms, s, 0.0, max_iter, tag,
                      rungs=[pos for _, pos in rungs] + [None] * extra, **more)]
    out = []
    for k, pos in rungs:  # one call per rung: the rung's PWM and a second one three binades further down
        pwm, b_lo, b_hi, s = _ladder_point(name, W, form, k)
        second = pwm.copy()
        second[W - 1] *= np.float32(0.125)
        out.append(_case(W, counts, _ladder_bg(W, b_lo, b_hi, div * 10 + ineq), np.stack([pwm, second]), s, 0.0, max_iter,
                         "%s/rung%+d" % (tag, pos), rungs=[pos, None], **more))
    return out


def class_G(W):
    names = sorted(LADDERS) if W < 12 else W12_LADDERS
    forms = ("pow2", "mant") if W in (8, 10) else ("pow2",)
    return [c for name in names for form in forms for c in guard_ladder(name, W, form)]


# ---- class F ---------------------------------------------------------------------------------------------------------
F_KINDS = ("bg_zero", "bg_negative", "bg_inf", "bg_nan", "count_max")
F_MATCHING, F_ELSEWHERE = (2, 8), (6,)  # PWMs with a zero entry under / beside the defect's k-mer


def f_placements(W):
    """the k-mers a defect is put on: first block of its chains, last block, the two sides of a span boundary"""
    NP = 4 ** W
    out = [("first_block", 5 % NP), ("last_block", NP - 3)]
    if W >= 8:
        out += [("span_end", 16383), ("span_start", 16384)]
    return out


def flagged_case(W, kind, place, x):
    """One defect in k-mer x of an otherwise healthy table, nine PWMs: 2 and 8 have a ZERO entry in a column under x (so
    x is zero-over-something for them), 6 has one beside x (zero over a positive background entry, weight 0, in a
    quarter of the table); the other six are ordinary."""
    counts, bg = small_counts(W, 1), healthy_bg(W, 1)
    counts[x] = 5
    saturation = 1e4
    if kind == "bg_zero":        # positive over zero: c s (finite); zero over zero: NaN
        bg[x] = 0.0
    elif kind == "bg_negative":  # 1 + s / odds < 0: a negative weight
        bg[x] = -bg[x]
    elif kind == "bg_inf":       # odds 0, weight 0
        bg[x] = np.inf
    elif kind == "bg_nan":
        bg[x] = np.nan
    elif kind == "count_max":    # c s = +inf
        counts[x] = 0xFFFFFFFF
        saturation = 2.0 ** 100
    else:
        raise ValueError(kind)
    pwms = healthy_pwms(W, 9, salt=7)
    p0 = W // 2
    for i in F_MATCHING:
        pwms[i, p0, digit(x, p0)] = 0.0
    for i in F_ELSEWHERE:
        pwms[i, p0, (digit(x, p0) + 1) & 3] = 0.0
    # (two iterations, so that the second consumes what the first made; one at W = 12, for the oracle's sake)
    return _case(W, counts, bg, pwms, saturation, 0.0, 2 if W < 12 else 1, "F/%s/%s/W%d" % (kind, place, W), cls="F", kind=kind,
                 x=int(x))


def class_F(W):
    places = f_placements(W)
    out = []
    for kind in F_KINDS:
        if W == 12:    # one case: the span boundary
            chosen = [places[2]] if kind == "bg_zero" else []
        else:
            chosen = places
        out += [flagged_case(W, kind, name, x) for name, x in chosen]
    return out


# ---- class S ---------------------------------------------------------------------------------------------------------
def ramp_counts(W, doublings=30):
    """a count table whose running sums pass a power of two every few blocks of every chain, `doublings` times"""
    x = np.arange(4 ** W, dtype=np.float64)
    period = 4 ** W / (doublings + 10.0) if W <= 10 else 16 * 16384.0
    return np.floor(2.0 ** np.minimum(x / period, float(doublings))).astype(np.uint32)


def overflow_case(W, max_iter):
    """(c): uniform PWM 2^-2 (and an ordinary one), background 2^-111, saturation 2^100: a weight is c 2^(111 - 2W) to
    within a few per cent; counts of about 2^20 where digit p0 is a0 make cell (p0, a0) -- 4^(W-1) terms -- reach twice
    FLT_MAX, i.e. +inf about half-way through its chain; every other cell holds a quarter of those k-mers and ends near
    FLT_MAX / 2."""
    p0, a0 = W // 2, 2
    x = np.arange(4 ** W)
    rng = _rng(6, W)
    big = ((x >> (2 * p0)) & 3) == a0
    counts = np.where(big, (1 << 20) + rng.integers(0, 1 << 10, 4 ** W), rng.integers(0, 8, 4 ** W)).astype(np.uint32)
    pwms = np.stack([np.full((W, 4), 0.25, np.float32), healthy_pwms(W, 1, salt=11, conc=200.0)[0]])
    return _case(W, counts, np.full(4 ** W, 2.0 ** -111, np.float32), pwms, 2.0 ** 100, 0.0, max_iter, "S/c/W%d" % W, cls="S",
                 kind="c", cell=(p0, a0))


def giant_case(W, max_iter):
    """(e): a table of ones with one count of 2^31 in the last block of its chains"""
    counts = np.ones(4 ** W, np.uint32)
    counts[4 ** W - 2] = 1 << 31
    return _case(W, counts, healthy_bg(W, 3), healthy_pwms(W, 3 if W < 12 else 1, salt=13), 1e4, 0.0, max_iter, "S/e/W%d" % W,
                 cls="S", kind="e")


def nan_row_case(W, threshold, max_iter, tag):
    """(b): no k-mer occurs: every cell sums to 0, every row is 0 / 0"""
    return _case(W, np.zeros(4 ** W, np.uint32), healthy_bg(W, 3), healthy_pwms(W, 2, salt=14), 1e4, threshold, max_iter, tag,
                 cls="S", kind="b")


def class_S(W):
    if W == 12:
        return [overflow_case(W, 1), giant_case(W, 1)]
    NP = 4 ** W
    x = np.arange(NP)
    out = []
    p0, a0 = W // 2, 1
    counts = small_counts(W, 2)
    counts[((x >> (2 * p0)) & 3) == a0] = 0  # (a): one cell sums to exactly 0; the second iteration meets the zero entry
    out.append(_case(W, counts, healthy_bg(W, 3), healthy_pwms(W, 3, salt=15), 1e4, 0.0, 2, "S/a/W%d" % W, cls="S", kind="a",
                     cell=(p0, a0)))
    out.append(nan_row_case(W, 0.0, 2, "S/b/W%d" % W))
    out.append(overflow_case(W, 2))
    # (d): every weight denormal -- through a denormal c s (saturation 2^-145), and through denormal odds
    # (products 2^-130 over a background of 2^10, saturation 2^-50: c s / (1 + s / odds) = c 2^-140)
    out.append(_case(W, small_counts(W, 3), healthy_bg(W, 3), healthy_pwms(W, 2, salt=16), 2.0 ** -145, 0.0, 2, "S/d1/W%d" % W,
                     cls="S", kind="d"))
    tiny = np.ldexp(np.ones((W, 4)), _column_exponents(W, -130)[:, None]).astype(np.float32)
    mant = (tiny * (1.0 + _rng(7, W).integers(0, 1 << 23, (W, 4)) / float(1 << 23))).astype(np.float32)
    out.append(_case(W, small_counts(W, 3), np.full(NP, 1024.0, np.float32), np.stack([tiny, mant]), 2.0 ** -50, 0.0, 1,
                     "S/d2/W%d" % W, cls="S", kind="d"))
    out.append(giant_case(W, 2))
    for s in (1.0, 2.0 ** 40):  # (f)
        out.append(_case(W, ramp_counts(W), healthy_bg(W, 4), healthy_pwms(W, 3, salt=17, conc=40.0), s, 0.0, 2,
                         "S/f/s=%g/W%d" % (s, W), cls="S", kind="f"))
    return out


# ---- class T ---------------------------------------------------------------------------------------------------------
T_K, T_MAX_ITER = 2, 4
T_THRESHOLDS = ("equal", "below", "above", "+inf", "-0.0", "nan")


def stopping_base(W):
    return small_counts(W, 5), healthy_bg(W, 5), healthy_pwms(W, 2, salt=19)


def class_T(W):
    """The reference loops while !(change <= threshold || it >= max_iter) (src/peng.cpp:104): thresholds at, one ulp below
    and one ulp above the oracle's change of PWM 0 after iteration T_K; +inf (no iteration), -0.0 and NaN (nothing stops
    the loop but max_iter); and a NaN change (class S (b)) under an ordinary threshold."""
    counts, bg, pwms = stopping_base(W)
    ch = np.float32(po.em(W, counts.astype(np.uint64), bg, pwms[0], 1e4, 0.0, T_K, mode=0, final_norm=False)[2])
    thr = {"equal": ch, "below": np.nextafter(ch, np.float32(0)), "above": np.nextafter(ch, np.float32(np.inf)),
           "+inf": np.float32(np.inf), "-0.0": np.float32(-0.0), "nan": np.float32(np.nan)}
    out = [_case(W, counts, bg, pwms, 1e4, thr[name], T_MAX_ITER, "T/%s/W%d" % (name, W), cls="T", kind=name, change_k=float(ch))
           for name in T_THRESHOLDS]
    out.append(nan_row_case(W, 0.08, T_MAX_ITER, "T/nan_change/W%d" % W))
    out[-1].update(cls="T", kind="nan_change")
    return out


# ---- the selection per W ---------------------------------------------------------------------------------------------
def classes(W):
    """the classes run at W (the issue's shapes): everything at 8 and 10; G (powers of two) and F at 2, 4, 6; a thinned
    G, F and S (c, e) at 12"""
    return ("G", "F", "S", "T") if W in (8, 10) else ("G", "F", "S") if W == 12 else ("G", "F")


def cases(W, cls):
    return {"G": class_G, "F": class_F, "S": class_S, "T": class_T}[cls](W)


def pwm_iterations(cs):
    """an upper bound of the oracle's work for a list of cases"""
    return sum(len(c["pwms"]) * max(c["max_iter"], 0) for c in cs)


def w12_budget():
    return sum(pwm_iterations(cases(12, cls)) for cls in classes(12))


# ---- the domain of the throughput mode (em_fast = 1) -----------------------------------------------------------------
def products(c, i):
    """the float32 product of PWM i over its columns for every k-mer, in the reference's order"""
    W = c["W"]
    x = np.arange(4 ** W)
    pr = np.ones(4 ** W, np.float32)
    with np.errstate(all="ignore"):
        for p in range(W):
            pr = pr * c["pwms"][i][p][(x >> (2 * p)) & 3]
    return pr


def fast_mode_domain(c, i):
    """include/pengk.h, mode 1: for every k-mer with a count, c s prod >= 2^-126 and prod + s bg < 2^126 -- for the PWM a
    case starts from.  Decided from ranges where those settle it (float products of positive operands are monotone: the
    products of the column minima and maxima bound every k-mer's product), k-mer by k-mer otherwise; at W = 12 from the
    ranges alone (sufficient, not necessary: 16 M products per PWM are the oracle's cost over again)."""
    f = np.float32
    lo, hi = f(2.0 ** -126), f(2.0 ** 126)
    pw = c["pwms"][i]
    live = c["counts"] > 0
    if not live.any() or not (pw > 0).all() or not (c["bg"][live] > 0).all():
        return False
    s = f(c["saturation"])
    with np.errstate(all="ignore"):
        p_lo = p_hi = f(1.0)
        for p in range(c["W"]):
            p_lo, p_hi = f(p_lo * pw[p].min()), f(p_hi * pw[p].max())
        if f(f(f(c["counts"][live].min()) * s) * p_lo) >= lo and f(f(s * c["bg"][live].max()) + p_hi) < hi:
            return True
        if c["W"] > 10:
            return False
        pr = products(c, i)[live]
        return bool(((c["counts"][live].astype(f) * s * pr >= lo) & (s * c["bg"][live] + pr < hi)).all())
