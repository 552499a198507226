"""pengk_pattern_stats_control (both kernels of csrc/stats.hip under the control policy) against the numpy model of
tests/control_stats_model.py, on constructed control tables -- c = 0, 1, 2^32 - 1; Lc = 0, 1, 2^40 and totals at which
(c + a) / Lc meets p_o exactly and within a float ulp on either side; a = 0, 0.5, 1; another winner at order 0 than at
order max_k; palindromes; mirrored and un-mirrored control tables; the input's own table as the control -- and once end
to end behind pengk_count.  tests/test_control_stats_cpu.py asserts that the cases hold those classes.

Bars, those of tests/test_gpu_table_edges.py: bgprob[0..max_k], expected and z bit for bit; log-p within 1 float ulp;
infinities agree exactly; NaN agrees in position."""
import numpy as np
import pytest

import control_stats_model as cm
import peng_motif_amd as pk
from oracle import oracle as po
from test_gpu_table_edges import _beyond_one_ulp, _mismatch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = pk.Context(0)
    yield c
    c.close()


def _describe(c, what, x, got, want, kernel):
    x = int(x)
    return ("%s differs: W = %d, %s, kernel %s, V %s, ltot %d, k = %d, max_k = %d, Lc = %d, a = %g, control %s, pattern %d (%s), "
            "count %d, control count %d: device %r (0x%08x), model %r (0x%08x)"
            % (what, c["W"], "both strands" if c["both"] else "plus strand", kernel, c["vkind"], c["ltot"], c["k"], c["max_k"],
               c["Lc"], c["a"], "mirrored" if c["ctrl_mirrored"] else "as built", x, po.kmer_str(x, c["W"]), int(c["counts"][x]),
               int(c["ctrl"][x]), float(got[x]), int(got[x:x + 1].view(np.uint32)[0]), float(want[x]),
               int(want[x:x + 1].view(np.uint32)[0])))


def _run_case(ctx, c, d_V, failures, kernels=(("per-pattern", 1),)):
    W, both = c["W"], c["both"]
    d_lt = pk.DeviceArray.from_host(ctx, np.array([c["ltot"]], np.uint64))
    d_c = pk.DeviceArray.from_host(ctx, c["counts"])
    d_cl = pk.DeviceArray.from_host(ctx, np.array([c["Lc"]], np.uint64))
    d_cc = d_c if c["ctrl"] is c["counts"] else pk.DeviceArray.from_host(ctx, c["ctrl"])
    for kernel, pairs in kernels:
        ctx.set_option("sweep_pairs", pairs)
        out = ctx.pattern_stats_control(W, both, c["k"], c["max_k"], d_V, d_lt, d_c, d_cc, d_cl, c["a"])
        bgp = out[0].to_host()
        for o in range(c["max_k"] + 1):
            bad = _mismatch(bgp[o], c["bgp"][o])
            if bad.size:
                failures.append(_describe(c, "bgprob[%d]" % o, bad[0], bgp[o], c["bgp"][o], kernel) + " (%d patterns)" % bad.size)
        del bgp
        for what, d, want, cmp in (("expected", out[1], c["expected"], _mismatch), ("z", out[3], c["z"], _mismatch),
                                   ("log-p", out[2], c["logp"], _beyond_one_ulp)):
            got = d.to_host()
            bad = cmp(got, want)
            if bad.size:
                failures.append(_describe(c, what, bad[0], got, want, kernel) + " (%d patterns)" % bad.size)
            del got
        for d in out:
            d.free()
    for d in {id(d): d for d in (d_lt, d_c, d_cl, d_cc)}.values():
        d.free()


@pytest.mark.parametrize("both", [False, True], ids=["plus", "both"])
@pytest.mark.parametrize("W", [4, 8, 10])
def test_control_sweep_on_constructed_tables(ctx, W, both):
    """every legal (k, max_k) over 0..2 with the control totals 0, 1, 2^40, 2^(2W + 24) and 3 000 017, the pseudocounts 0,
    0.5 and 1, natural and hand-made V (products down to the denormals and zero), count tables at every value edge,
    mirrored and un-mirrored control tables; then the input's own table as the control"""
    failures = []
    d_V = {}
    for spec in cm.small_cases(W, both):
        c = cm.case(W, both, spec)
        if spec[0] not in d_V:
            d_V[spec[0]] = pk.DeviceArray.from_host(ctx, c["V"])
        _run_case(ctx, c, d_V[spec[0]], failures)
        if len(failures) > 20:
            break
    c = cm.own_table_case(W, both)
    _run_case(ctx, c, d_V["a"], failures)
    assert not failures, "%d mismatches, the first ones:\n%s" % (len(failures), "\n".join(failures[:8]))


def test_control_sweep_at_w12_under_both_kernels(ctx):
    """W = 12, both strands: the twin-tile kernel (the twin's control count travels through LDS beside its count; a twin
    with another control count or another count is evaluated again) and the per-pattern kernel (sweep_pairs = 0) on the
    same case: mirrored input, un-mirrored control"""
    failures = []
    try:
        c = cm.case(12, True, cm.big_case(12))
        d_V = pk.DeviceArray.from_host(ctx, c["V"])
        _run_case(ctx, c, d_V, failures, kernels=(("twin-tile", 1), ("per-pattern", 0)))
    finally:
        ctx.set_option("sweep_pairs", 1)
    assert not failures, "%d mismatches, the first ones:\n%s" % (len(failures), "\n".join(failures[:8]))


def test_pseudocount_must_be_finite_and_not_negative(ctx):
    c = cm.own_table_case(4, False)
    d_V = pk.DeviceArray.from_host(ctx, c["V"])
    d_lt = pk.DeviceArray.from_host(ctx, np.array([c["ltot"]], np.uint64))
    d_c = pk.DeviceArray.from_host(ctx, c["counts"])
    for a in (-1.0, float("nan"), float("inf")):
        with pytest.raises(pk.PengkError) as e:
            ctx.pattern_stats_control(4, False, 0, 0, d_V, d_lt, d_c, d_c, d_lt, a)
        assert e.value.code == pk.ERR_ARG


@pytest.mark.parametrize("both", [False, True], ids=["plus", "both"])
def test_end_to_end_behind_the_count(ctx, both):
    """500 synthetic sequences as the input, 500 longer ones as the control (a pattern the control never shows keeps its
    Markov probability, one it shows three times does not): pengk_count, the mirror and the new entry against
    oracle.count plus the model"""
    W, K = 8, 2
    codes, offs = po.synth(11, 0, 500, 120)
    ccodes, coffs = po.synth(12, 1000, 500, 400)
    want_counts, want_ltot = po.count(codes, offs, W, both)
    want_ctrl, want_lc = po.count(ccodes, coffs, W, both)
    V = po.bg_V(po.bg_counts(ccodes, coffs, 2), 2)
    p = [po.bgprob(W, o, V, both) for o in range(K + 1)]
    q, e, lp, z = cm.sweep(W, want_counts, want_ltot, p, K, want_ctrl, want_lc, 1.0)

    def device_count(cd, of):
        ctx.upload(pk.Packed(cd, of, W))
        counts, ltot = ctx.count(both)
        if both:
            ctx.mirror(W, counts)
        return counts, ltot

    d_ctrl, d_lc = device_count(ccodes, coffs)
    d_counts, d_ltot = device_count(codes, offs)
    assert int(d_lc.to_host()[0]) == want_lc and int(d_ltot.to_host()[0]) == want_ltot
    assert np.array_equal(d_ctrl.to_host().astype(np.uint64), want_ctrl)
    assert np.array_equal(d_counts.to_host().astype(np.uint64), want_counts)
    out = ctx.pattern_stats_control(W, both, K, K, ctx.to_device(V), d_ltot, d_counts, d_ctrl, d_lc, 1.0)
    bgp = out[0].to_host()
    for o in range(K + 1):
        assert not _mismatch(bgp[o], q[o]).size, o
    assert not _mismatch(out[1].to_host(), e).size
    assert not _mismatch(out[3].to_host(), z).size
    assert not _beyond_one_ulp(out[2].to_host(), lp).size
    # and the control changes something here: it raises the expected count of some patterns, not of all
    changed = q[K] != p[K]
    assert changed.any() and not changed.all()
