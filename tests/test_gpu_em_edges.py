"""The EM kernels (csrc/em.hip, em_serial.h, em_fused.hip, em_legacy.hip, seqsum.h) on the CONSTRUCTED cases of
tests/em_edges_model.py -- the lean division's guard a binade at a time across each of its inequalities, PWMs that get
flagged, cell sums that are zero, infinite, denormal or dominated by one term, the stopping rule at equality and at NaN
-- against the oracle (oracle.em, mode 0: the reference's left-to-right float32 sums, src/peng.cpp:104-144,180-197;
mode 1 for the fp64 modes).  Tables go to the device as built; no sequences are attached, no count runs.
tests/test_em_edges_cpu.py asserts that the cases are what they claim to be.

Bars, the project's own (tests/test_gpu_parity.py, tests/test_gpu_table_edges.py).  Serial mode (em_fast = 2): PWMs and
`change` bit for bit, infinities exactly, NaN in position (x86 and gfx950 give 0 / 0 different sign bits), iteration
counts equal -- for em_lean_div 1 and 0 and for every generation of pengk_test_em_generation the W has, each against
the oracle.  em_fast = 0 and 1: within BASELINE.json's 1e-5 relative of oracle mode 1 on the cases that are finite
everywhere (em_fast = 1: inside the domain include/pengk.h states for it), iteration counts equal where the oracle's
change is not within 1e-5 relative of the threshold; on the flagged and the overflowing cases em_fast = 0 alone, NaN and
infinities in position.

And directly against the COMPILED REFERENCE (tests/golden/edges_em_w*.npz, tests/golden/make_edge_golden.py): what the
device returned in the runs above, after the model's final normalisation (edge_fixtures.final_normalisation: the extra
row division of the constructor the reference returns its PWM through), against the reference's PWM, and h_iters
against the reference's count where the fixture identifies one (edge_fixtures.em_reference_iterations).  em_fast = 2:
bit for bit.  em_fast = 0 and 1 add terms the reference's way but sum them in fp64; include/pengk.h gives them 1e-5
relative to the exact sums and says that "the reference's own serial float32 sums are off by up to 2.6e-4 relative from
the exact ones".  On these tables the reference is further off than that (S/e/W12, one term of 2^31 among 4^12 ones:
8.1e-3; F/bg_zero/span_end/W12: 2.1e-3; up to 2.4e-4 at W <= 10), so no single figure can stand for its error.  The bar
against the reference's float32 PWM is therefore, cell by cell, the modes' own 1e-5 relative PLUS the reference's own
distance from the fp64 sums of the same terms in that cell -- oracle mode 1, computed on the CPU, which
tests/test_oracle_golden.py pins; nothing measured on the device goes into it.  By the triangle inequality this holds
whenever the oracle tests above hold; it is here so that the device is compared with the reference's numbers in every
mode, and what decides about modes 0 and 1 remains the 1e-5 against oracle mode 1.  These tests read tests/golden only,
never the reference."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import edge_fixtures as ef
import em_edges_model as em
import peng_motif_amd as pk
from oracle import oracle as po
from test_gpu_table_edges import _mismatch, _ordered

pytestmark = pytest.mark.gpu

W_CLS = [(W, cls) for W in em.WS for cls in em.classes(W)]
_IDS = ["W%d-%s" % wc for wc in W_CLS]


@pytest.fixture(scope="module")
def ctx():
    c = pk.Context(0)
    yield c
    c.close()


# ---- the oracle, once per (W, class) and mode ------------------------------------------------------------------------
_ORACLE = {}


def _oracle(W, cls, mode, cs=None):
    """[per case: [(pwm, iterations, change) per PWM]]"""
    if (W, cls, mode) not in _ORACLE:
        cs = cs if cs is not None else em.cases(W, cls)
        jobs = []
        for c in cs:
            c64 = c["counts"].astype(np.uint64)
            jobs += [(c, c64, i) for i in range(len(c["pwms"]))]
        with ThreadPoolExecutor(min(12, os.cpu_count() or 1)) as pool:
            flat = list(pool.map(lambda j: po.em(W, j[1], j[0]["bg"], j[0]["pwms"][j[2]], j[0]["saturation"], j[0]["threshold"],
                                                 j[0]["max_iter"], mode=mode, final_norm=False), jobs))
        out, at = [], 0
        for c in cs:
            out.append(flat[at:at + len(c["pwms"])])
            at += len(c["pwms"])
        _ORACLE[W, cls, mode] = out
    return _ORACLE[W, cls, mode]


def _u32(v):
    return int(np.float32(v).view(np.uint32))


def _describe(c, variant, i, what, got, want, n=1):
    return ("%s differs: case %s, W = %d, %s, PWM %d of %d: device %r (0x%08x), oracle %r (0x%08x), %d apart in float order"
            " (%d values of this PWM)" % (what, c["tag"], c["W"], variant, i, len(c["pwms"]), float(got), _u32(got), float(want),
                                         _u32(want), int(abs(_ordered(np.array([got], np.float32))[0] - _ordered(np.array([want], np.float32))[0])),
                                         n))


def _compare_bits(c, variant, got, want, failures):
    """got = (pwms, iterations, change) of the device, want = [(pwm, iterations, change)] of oracle mode 0"""
    for i, (pw, it, ch) in enumerate(want):
        g, w = got[0][i].reshape(-1), np.ascontiguousarray(pw, np.float32).reshape(-1)
        bad = _mismatch(g, w)
        if bad.size:
            j = int(bad[0])
            failures.append(_describe(c, variant, i, "cell (%d, %s)" % (j >> 2, "ACGT"[j & 3]), g[j], w[j], bad.size))
        if int(got[1][i]) != it:
            failures.append("iterations differ: case %s, W = %d, %s, PWM %d: device %d, oracle %d" % (c["tag"], c["W"], variant, i, int(got[1][i]), it))
        if _mismatch(got[2][i:i + 1], np.array([ch], np.float32)).size:
            failures.append(_describe(c, variant, i, "change", got[2][i], np.float32(ch)))


def _variants(W):
    """(name, generation, em_lean_div): the library's scheme with and without the lean division, and every earlier
    generation the W has (pengk_test_em_generation: 0 the dependent additions, 1 the scan block after block, 3 the
    two-launch variant).  Below W = 10 the variants share kernels (no lean division there; at W = 8 generation 2 is the
    block-after-block scan): they cost milliseconds and stay, so that a W that gets kernels of its own is covered."""
    v = [("generation 2, lean division", 2, 1), ("generation 2, plain division", 2, 0)]
    if W >= 8:
        v += [("generation 0", 0, 1), ("generation 1", 1, 1)]
    if W >= 10:  # (em_fused.hip has a lean and a plain body of its own)
        v += [("generation 3, lean division", 3, 1), ("generation 3, plain division", 3, 0)]
    return v


def _upload(ctx, c):
    return pk.DeviceArray.from_host(ctx, c["counts"]), pk.DeviceArray.from_host(ctx, c["bg"])


def _em(ctx, c, d_counts, d_bg):
    return ctx.em(c["W"], c["pwms"], d_counts, d_bg, c["saturation"], c["threshold"], c["max_iter"])


def _report(failures):
    assert not failures, "%d mismatches, the first ones:\n%s" % (len(failures), "\n".join(failures[:8]))


# ---- serial mode -----------------------------------------------------------------------------------------------------
_SERIAL = {}


def _serial_device(ctx, W, cls, cs):
    """[per case: {variant: (pwms, iterations, change)}] as the device returned them, once per (W, class): the oracle
    test and the reference test below look at the same runs"""
    if (W, cls) not in _SERIAL:
        out = []
        ctx.set_option("em_fast", 2)
        try:
            for c in cs:
                d_counts, d_bg = _upload(ctx, c)
                got = {}
                for name, generation, lean in _variants(W):
                    ctx.test_em_generation(generation)
                    ctx.set_option("em_lean_div", lean)
                    got[name] = tuple(np.array(a, copy=True) for a in _em(ctx, c, d_counts, d_bg))
                out.append(got)
                d_counts.free()
                d_bg.free()
        finally:
            ctx.test_em_generation(2)
            ctx.set_option("em_lean_div", 1)
            ctx.set_option("em_fast", 1)
        _SERIAL[W, cls] = out
    return _SERIAL[W, cls]


@pytest.mark.parametrize("W,cls", W_CLS, ids=_IDS)
def test_serial_mode_bit_for_bit_against_the_oracle(ctx, W, cls):
    """Every case of the class, under every variant (_variants), each against oracle mode 0: PWMs, iteration counts and
    `change`."""
    failures = []
    cs = em.cases(W, cls)
    want = _oracle(W, cls, 0, cs)
    for c, w, got in zip(cs, want, _serial_device(ctx, W, cls, cs)):
        for name, _, _ in _variants(W):
            _compare_bits(c, name, got[name], w, failures)
    _report(failures)


def _fixture(W, cs):
    fix = ef.load(ef.em_file(W))
    for c in cs:
        drift = ef.inputs_match(fix, c["tag"], ef.em_inputs(c))
        assert drift is None, drift
    return fix


@pytest.mark.parametrize("W,cls", W_CLS, ids=_IDS)
def test_serial_mode_bit_for_bit_against_the_reference(ctx, W, cls):
    """The same device runs against the compiled reference's answers (the fixture): h_pwms after the final normalisation
    against the PWM the reference returned at max_iter, bit for bit (NaN in position: x86 and gfx950 give 0 / 0 different
    sign bits); h_iters against the reference's count -- the smallest cap that returns its final PWM -- where the
    fixture identifies one.  Every variant."""
    failures = []
    cs = em.cases(W, cls)
    fix = _fixture(W, cs)
    for c, got in zip(cs, _serial_device(ctx, W, cls, cs)):
        ref = ef.em_reference(fix, c)
        its = ef.em_reference_counts(fix, c)  # (-1: not identifiable; tests/test_edges_reference_cpu.py holds them to the PWMs)
        for name, _, _ in _variants(W):
            norm = ef.final_normalisation(got[name][0])
            for i in range(len(c["pwms"])):
                g, w = norm[i].reshape(-1), np.ascontiguousarray(ref[-1, i]).reshape(-1)
                bad = _mismatch(g, w)
                if bad.size:
                    j = int(bad[0])
                    failures.append(_describe(c, name, i, "cell (%d, %s)" % (j >> 2, "ACGT"[j & 3]), g[j], w[j], bad.size).replace("oracle", "reference"))
                if its[i] >= 0 and int(got[name][1][i]) != its[i]:
                    failures.append("iterations differ: case %s, W = %d, %s, PWM %d: device %d, reference %d"
                                    % (c["tag"], W, name, i, int(got[name][1][i]), its[i]))
    _report(failures)


def test_guard_ladders_with_wrong_binade_estimates(ctx):
    """Class G at W = 10 once more with em_test_skew = 2: every second block is handed a wrong binade, on weights whose
    magnitudes lie where the ladders put them (2^-118 .. 2^61)."""
    W = 10
    failures = []
    cs = em.cases(W, "G")
    want = _oracle(W, "G", 0, cs)
    ctx.set_option("em_fast", 2)
    try:
        ctx.set_option("em_test_skew", 2)
        for c, w in zip(cs, want):
            d_counts, d_bg = _upload(ctx, c)
            _compare_bits(c, "em_test_skew = 2", _em(ctx, c, d_counts, d_bg), w, failures)
            d_counts.free()
            d_bg.free()
    finally:
        ctx.set_option("em_test_skew", 0)
        ctx.set_option("em_fast", 1)
    _report(failures)


# ---- the fp64 modes --------------------------------------------------------------------------------------------------
def _finite(results):
    return all(np.isfinite(pw).all() and np.isfinite(ch) for pw, it, ch in results)


def _compare_fp64(c, mode, got, want, failures, only=None):
    for i, (pw, it, ch) in enumerate(want):
        if only is not None and not only(i):
            continue
        g, w = got[0][i].reshape(-1).astype(np.float64), np.asarray(pw, np.float64).reshape(-1)
        bad = np.flatnonzero((np.isnan(g) != np.isnan(w)) | (np.isinf(w) & (g != w)) | (np.isinf(g) & (g != w)))
        fin = np.isfinite(g) & np.isfinite(w)
        rel = np.abs(g - w) / np.maximum(np.abs(w), 1e-30)
        bad = np.union1d(bad, np.flatnonzero(fin & (rel > 1e-5)))
        if bad.size:
            j = int(bad[0])
            failures.append(_describe(c, "em_fast = %d" % mode, i, "cell (%d, %s)" % (j >> 2, "ACGT"[j & 3]), np.float32(g[j]), np.float32(w[j]),
                                      bad.size))
        dev_it = int(got[1][i])
        if dev_it != it:
            # equal counts are waived only where the stop was a close call: the oracle's change at the EARLIER of the two
            # stops (the iteration at which one of them went on and the other did not) within 1e-5 relative of the threshold
            k, thr = min(dev_it, it), c["threshold"]
            ch_k = po.em(c["W"], c["counts"].astype(np.uint64), c["bg"], c["pwms"][i], c["saturation"], -1.0, k, mode=1, final_norm=False)[2]
            if not (k > 0 and np.isfinite(ch_k) and np.isfinite(thr) and abs(ch_k - thr) <= 1e-5 * abs(thr)):
                failures.append("iterations differ: case %s, W = %d, em_fast = %d, PWM %d: device %d, oracle %d (oracle's change after "
                                "iteration %d: %r, threshold %r)" % (c["tag"], c["W"], mode, i, dev_it, it, k, ch_k, thr))


_FP64 = {}


def _fp64_device(ctx, W, cls, cs):
    """[per case: (em_fast = 0 result, em_fast = 1 result or None, inside: per PWM, in the domain of mode 1)], once per
    (W, class).  em_fast = 1 runs on the cases whose oracle results are finite everywhere and that have a PWM inside the
    mode's stated domain."""
    if (W, cls) not in _FP64:
        want0, want1 = _oracle(W, cls, 0, cs), _oracle(W, cls, 1, cs)
        out = []
        try:
            for c, w0, w1 in zip(cs, want0, want1):
                d_counts, d_bg = _upload(ctx, c)
                ctx.set_option("em_fast", 0)
                got0 = tuple(np.array(a, copy=True) for a in _em(ctx, c, d_counts, d_bg))
                got1, inside = None, [False] * len(c["pwms"])
                if _finite(w0) and _finite(w1):
                    inside = [em.fast_mode_domain(c, i) for i in range(len(c["pwms"]))]
                    if any(inside):
                        ctx.set_option("em_fast", 1)
                        got1 = tuple(np.array(a, copy=True) for a in _em(ctx, c, d_counts, d_bg))
                out.append((got0, got1, inside))
                d_counts.free()
                d_bg.free()
        finally:
            ctx.set_option("em_fast", 1)
        _FP64[W, cls] = out
    return _FP64[W, cls]


@pytest.mark.parametrize("W,cls", W_CLS, ids=_IDS)
def test_fp64_modes_against_the_oracle(ctx, W, cls):
    """em_fast = 0 (the reference's terms, fp64 tree sums) on every case: within 1e-5 relative of oracle mode 1, NaN and
    infinities in position -- the flagged and the overflowing cases included.  em_fast = 1 (one reciprocal per term) on the
    cases whose oracle results are finite everywhere, PWM by PWM inside the mode's stated domain (include/pengk.h;
    em_edges_model.fast_mode_domain)."""
    failures = []
    cs = em.cases(W, cls)
    want1 = _oracle(W, cls, 1, cs)
    for c, w1, (got0, got1, inside) in zip(cs, want1, _fp64_device(ctx, W, cls, cs)):
        _compare_fp64(c, 0, got0, w1, failures)
        if got1 is not None:
            _compare_fp64(c, 1, got1, w1, failures, only=lambda i: inside[i])
    _report(failures)


@pytest.mark.parametrize("W,cls", W_CLS, ids=_IDS)
def test_fp64_modes_against_the_reference(ctx, W, cls):
    """The same em_fast = 0 and em_fast = 1 runs (the latter on the cases and PWMs that test admits) against the
    reference's PWM from the fixture, after the final normalisation: cell by cell within 1e-5 relative plus the
    reference's own distance from oracle mode 1 in that cell (module docstring), NaN and infinities in position; h_iters
    against the reference's count where the fixture identifies one.  The counts may differ only on a close call: where
    the reference's float32 change (oracle mode 0, which the CPU tests hold to the reference bit for bit) and the fp64
    change at the earlier stop fall on different sides of the threshold -- class T's `equal`, `below`, `above` put the
    threshold within an ulp of the float32 change -- or the fp64 change is within the oracle test's 1e-5 relative of it.
    The two PWMs then belong to different iterations and are not compared."""
    failures = []
    cs = em.cases(W, cls)
    fix = _fixture(W, cs)
    want1 = _oracle(W, cls, 1, cs)
    for c, w1, (got0, got1, inside) in zip(cs, want1, _fp64_device(ctx, W, cls, cs)):
        ref = ef.em_reference(fix, c)
        its = ef.em_reference_counts(fix, c)  # (-1: not identifiable; tests/test_edges_reference_cpu.py holds them to the PWMs)
        for mode, got in ((0, got0), (1, got1)):
            if got is None:
                continue
            norm = ef.final_normalisation(got[0])
            for i in range(len(c["pwms"])):
                if mode == 1 and not inside[i]:
                    continue
                dev_it = int(got[1][i])
                if its[i] >= 0 and dev_it != its[i]:
                    k, thr = min(dev_it, int(its[i])), np.float32(c["threshold"])
                    c64 = c["counts"].astype(np.uint64)
                    ch32, ch64 = (po.em(W, c64, c["bg"], c["pwms"][i], c["saturation"], -1.0, k, mode=m, final_norm=False)[2] for m in (0, 1))
                    close = k > 0 and ((np.float32(ch32) <= thr) != (np.float32(ch64) <= thr) or
                                       (np.isfinite(ch64) and np.isfinite(thr) and abs(ch64 - thr) <= 1e-5 * abs(thr)))
                    if not close:
                        failures.append("iterations differ: case %s, W = %d, em_fast = %d, PWM %d: device %d, reference %d (after iteration %d "
                                        "the oracle's float32 change is %r, its fp64 change %r, threshold %r)"
                                        % (c["tag"], W, mode, i, dev_it, its[i], k, ch32, ch64, float(thr)))
                    continue
                if w1[i][1] != dev_it:
                    continue  # (the oracle test reports it; its PWM is another iteration's)
                g, w = norm[i].reshape(-1).astype(np.float64), ref[-1, i].reshape(-1).astype(np.float64)
                o = ef.final_normalisation(w1[i][0]).reshape(-1).astype(np.float64)
                bad = np.flatnonzero((np.isnan(g) != np.isnan(w)) | (np.isinf(w) & (g != w)) | (np.isinf(g) & (g != w)))
                fin = np.isfinite(g) & np.isfinite(w) & np.isfinite(o)
                with np.errstate(invalid="ignore"):
                    tol = 1e-5 * np.maximum(np.abs(o), 1e-30) + np.abs(w - o)
                    bad = np.union1d(bad, np.flatnonzero(fin & (np.abs(g - w) > tol)))
                if bad.size:
                    j = int(bad[0])
                    failures.append(_describe(c, "em_fast = %d" % mode, i, "cell (%d, %s)" % (j >> 2, "ACGT"[j & 3]), np.float32(g[j]),
                                              np.float32(w[j]), bad.size).replace("oracle", "reference"))
    _report(failures)


def _domain_edge_cases():
    """Four single-PWM cases at W = 8, random mantissas everywhere, next to the two edges of the mode's domain.
    Lower edge (background 1, saturation 2^-40, the PWM's product moves a binade at a time): the smallest product with
    every c s prod >= 2^-126 -- the least of them then lies in [2^-126, 2^-125) --, and the largest with every c s prod
    rounding to 0 (below 2^-150: every term 0).  Upper edge (products about 2^60, saturation 2^13, the background table moves): the
    largest table with every prod + s bg < 2^126 -- the greatest then in [2^125, 2^126) --, and the smallest whose every
    s bg is +inf (every term 0)."""
    W = 8
    f = np.float32
    rng = np.random.default_rng(8)
    mant = 1.0 + rng.integers(0, 1 << 23, (W, 4)) / float(1 << 23)
    bgm = 1.0 + rng.integers(0, 1 << 23, 4 ** W) / float(1 << 23)
    counts = em.small_counts(W)
    live = counts > 0
    low = lambda P: em._case(W, counts, np.ones(4 ** W, f), np.ldexp(mant, em._column_exponents(W, P)[:, None]), 2.0 ** -40, 0.0, 1,
                             "fast-domain/c s prod/P=%d" % P)
    csp = lambda c: (c["counts"].astype(f) * f(c["saturation"]) * em.products(c, 0))[live]
    P_in = min(P for P in range(-100, -70) if csp(low(P)).min() >= f(2.0 ** -126))
    P_out = max(P for P in range(-130, -100) if csp(low(P)).max() == 0)
    pw = np.ldexp(mant, em._column_exponents(W, 60)[:, None])
    high = lambda B: em._case(W, counts, np.ldexp(bgm, B), pw, 2.0 ** 13, 0.0, 1, "fast-domain/prod + s bg/B=%d" % B)
    with np.errstate(over="ignore"):
        top = lambda c: f(c["saturation"]) * c["bg"] + em.products(c, 0)
        B_in = max(B for B in range(100, 116) if top(high(B)).max() < f(2.0 ** 126))
        B_out = min(B for B in range(100, 116) if np.isinf(f(2.0 ** 13) * high(B)["bg"]).all())
    return [low(P_in), high(B_in)], [low(P_out), high(B_out)]


def test_throughput_mode_on_both_sides_of_its_domain(ctx):
    """include/pengk.h states where em_fast = 1 holds its 1e-5, and what it returns far outside.  Next to each edge of the
    domain (_domain_edge_cases), inside: within 1e-5 of oracle mode 1.  Outside, where the header says every term is 0:
    every row is 0 / 0 although the oracle's PWM is finite.  em_fast = 0 holds the bar on all four.  (Between the two
    points of an edge the mode loses bits gradually; the header promises nothing there and nothing is asserted.)"""
    inside, outside = _domain_edge_cases()
    failures = []
    try:
        for c, is_in in [(c, True) for c in inside] + [(c, False) for c in outside]:
            assert em.fast_mode_domain(c, 0) == is_in, c["tag"]
            want = [po.em(c["W"], c["counts"].astype(np.uint64), c["bg"], c["pwms"][0], c["saturation"], 0.0, 1, mode=1, final_norm=False)]
            assert _finite(want), c["tag"]
            d_counts, d_bg = _upload(ctx, c)
            ctx.set_option("em_fast", 0)
            _compare_fp64(c, 0, _em(ctx, c, d_counts, d_bg), want, failures)
            ctx.set_option("em_fast", 1)
            got = _em(ctx, c, d_counts, d_bg)
            if is_in:
                _compare_fp64(c, 1, got, want, failures)
            elif not np.isnan(got[0]).all():
                failures.append("case %s: em_fast = 1 was to return 0 / 0 in every cell, returned %r" % (c["tag"], got[0][0].tolist()))
            d_counts.free()
            d_bg.free()
    finally:
        ctx.set_option("em_fast", 1)
    _report(failures)


# ---- the device-resident entry point ---------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [6, 8, 10])
@pytest.mark.parametrize("mode", [2, 0, 1])
def test_em_device_equals_em_on_a_flagged_batch(ctx, W, mode):
    """pengk_em_device (what bench.py times) on a class F batch -- a zero background entry on a span boundary (W = 6:
    in the last block), nine PWMs, two of them flagged: the PWMs and `change` of pengk_em bit for bit, d_state =
    {iterations, active} per PWM as include/pengk.h documents it: pengk_em's iteration counts, and nobody active once the
    call is through (max_iterations reached).  (This one compares the two entry points with each other, in every mode;
    what pengk_em returns on these batches is compared with the oracle by the tests above.)"""
    c = [c for c in em.class_F(W) if c["kind"] == "bg_zero"][-1]
    n = len(c["pwms"])
    d_counts, d_bg = _upload(ctx, c)
    ctx.set_option("em_fast", mode)
    try:
        want = _em(ctx, c, d_counts, d_bg)
        d_pwms = pk.DeviceArray.from_host(ctx, c["pwms"])
        d_state = pk.DeviceArray.from_host(ctx, np.full((n, 2), -7, np.int32))
        d_change = pk.DeviceArray.from_host(ctx, np.full(n, np.float32(-7.0)))
        ctx.em_device(W, n, d_pwms, d_counts, d_bg, d_state, d_change, c["saturation"], c["threshold"], c["max_iter"])
        ctx.synchronize()
        got, state, change = d_pwms.to_host(), d_state.to_host(), d_change.to_host()
        for d in (d_pwms, d_state, d_change):
            d.free()
    finally:
        ctx.set_option("em_fast", 1)
        d_counts.free()
        d_bg.free()
    assert np.isnan(want[0][em.F_MATCHING[0]]).any() and np.isfinite(want[0][0]).all()
    for i in range(n):
        assert not _mismatch(got[i].reshape(-1), want[0][i].reshape(-1)).size, (c["tag"], mode, i)
    assert not _mismatch(change, want[2]).size, (c["tag"], mode)
    assert state[:, 0].tolist() == want[1].tolist() == [c["max_iter"]] * n, (c["tag"], mode, state.tolist())
    assert state[:, 1].tolist() == [0] * n, (c["tag"], mode, state.tolist())
