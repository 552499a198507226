"""The two device entries of the Markov null of order K <= 5 (include/pengk.h, "a Markov null of order 3 .. 5 for the
sweep") against the numpy model of tests/bg_order_model.py, bit for bit.

pengk_bg_count_order, K = 0 .. 5: sequences of 0 .. 7 bases and at every length where a half, a word of the layout or a tile
of 64 positions ends; an invalid base at every position of a 70-base sequence in turn and pairs 1 .. 7 apart (every way an
order <= 5 loses its context); without input validity; the hottest bins (100 000 x 40 bases, all A); 100 000 short mixed
sequences; one sequence of 70 000 bases; a subset of the offset arrays; two calls; K = 2 against pengk_strata_bg_count with
one stratum; the argument errors.

pengk_pattern_stats_order: V tables of the kinds uniform, random Dirichlet, a zero conditional, a one-hot row and a denormal
entry, on the count edges of tests/table_edges_model.py, W = 2 .. 10 for every K in {0, 2, 3, 4, 5}, both strand settings,
every legal (k, max_k), with and without the control tables of tests/control_stats_model.py; K = 2 against
pengk_pattern_stats and pengk_pattern_stats_control themselves; W = 12 once at K = 5; sweep_pairs on and off.  Bars, those
of tests/test_gpu_table_edges.py: bgprob, expected and z bit for bit, log-p within one float ulp.

Both entries once behind the gate of tests/stream_gate.py on a caller-owned stream: right order, no host wait."""
import numpy as np
import pytest
import torch  # noqa: F401  (the gate's streams are torch's: its HIP runtime is loaded before the library's, whichever test runs first)

import bg_order_model as bm
import peng_motif_amd as pk
import motif_score_model as ms
import stream_gate as sg
import table_edges_model as tm
from oracle import oracle as po
from test_gpu_stream_order import through_the_gate
from test_gpu_table_edges import _beyond_one_ulp, _mismatch

pytestmark = pytest.mark.gpu

KS = (0, 1, 2, 3, 4, 5)


@pytest.fixture(scope="module")
def ctx():
    c = pk.Context(0)
    yield c
    c.close()


# ---- entry 1 ------------------------------------------------------------------------------------------------------------------
def check_counters(ctx, seqs, K, all_valid=False, scan=None, want=None):
    if scan is None:
        scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    got = ctx.bg_count_order(scan, K, all_valid=all_valid).to_host()
    if want is None:
        want = bm.bg_count(seqs, K, all_valid)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "K %d: counter %d: %d, the model %d (%d counters differ)" % (K, bad[0], got[bad[0]], want[bad[0]], bad.size)
    return int(want.sum())


def mixed(seed, lengths, invalid=0.0):
    """sequences of skewed and of even composition, some with invalid bases"""
    rng = np.random.default_rng(seed)
    out = []
    for i, L in enumerate(lengths):
        g = (i % 5) / 4.0
        c = (rng.choice(4, L, p=[(1 - g) / 2 * 0.9 + 0.05, g / 2 * 0.9 + 0.025, g / 2 * 0.9 + 0.025, (1 - g) / 2 * 0.9]) + 1).astype(np.uint8)
        if invalid and L:
            c[rng.random(L) < invalid] = 0
        out.append(c)
    return out


EDGE_LENGTHS = [0, 1, 2, 3, 5, 6, 7, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 130]


@pytest.mark.parametrize("K", KS)
def test_lengths_at_the_edges(ctx, K):
    seqs = mixed(1, EDGE_LENGTHS * 4) + mixed(2, EDGE_LENGTHS * 2, invalid=0.1)
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    assert check_counters(ctx, seqs, K, scan=scan) > 0
    check_counters(ctx, seqs, K, all_valid=True, scan=scan)
    for c in seqs[1:len(EDGE_LENGTHS)]:  # every length alone
        check_counters(ctx, [c], K)


@pytest.mark.parametrize("K", KS)
def test_invalid_bases_wherever_an_order_loses_its_context(ctx, K):
    base = mixed(3, [5] * 5 + [70])[5]
    seqs = []
    for p in range(70):  # one at every position in turn
        c = base.copy()
        c[p] = 0
        seqs.append(c)
    for d in range(1, 8):  # and pairs 1 .. 7 apart: at the start, across a half, a word and the tile, at the end
        for p in (0, 3, 12, 28, 30, 58, 62, 69 - d):
            c = base.copy()
            c[[p, p + d]] = 0
            seqs.append(c)
    seqs.append(np.zeros(70, np.uint8))
    check_counters(ctx, seqs, K)
    for i in (0, 5, 31, 64, 69, 70, 100, len(seqs) - 1):
        check_counters(ctx, [seqs[i]], K)


@pytest.mark.parametrize("K", KS)
def test_the_hottest_bins(ctx, K):
    """100 000 x 40 bases, all A: one counter an order takes everything"""
    n, L = 100_000, 40
    want = np.zeros(bm.size(K), np.uint64)
    for k in range(K + 1):
        want[bm.at(k)] = n * (L - k)
    check_counters(ctx, [np.ones(L, np.uint8)] * n, K, want=want)


@pytest.fixture(scope="module")
def many():
    rng = np.random.default_rng(5)
    pool = mixed(6, rng.integers(0, 80, 500).tolist(), invalid=0.02)
    idx = rng.integers(0, len(pool), 100_000)
    return [pool[i] for i in idx]


@pytest.mark.parametrize("K", KS)
def test_100000_short_mixed_sequences(ctx, many, K):
    check_counters(ctx, many, K)


@pytest.mark.parametrize("K", KS)
def test_a_subset_and_two_calls(ctx, many, K):
    seqs = many
    lay = pk.ScanLayout(*ms.flatten(seqs))
    words, valid = ctx.to_device(lay.words), ctx.to_device(lay.valid)
    n = len(seqs)
    pick = np.flatnonzero(np.random.default_rng(7).random(n) < 0.3)[::-1].copy()   # (not contiguous, and in another order)
    part = (words, valid, ctx.to_device(lay.offs[pick]), ctx.to_device(lay.lens[pick]), len(pick))
    check_counters(ctx, [seqs[i] for i in pick], K, scan=part)
    want = bm.bg_count(seqs, K)
    for cut in (1, 50_001):
        bg = ctx.to_device(np.zeros(bm.size(K), np.uint64))
        for a, b in ((0, cut), (cut, n)):
            part = (words, valid, ctx.to_device(lay.offs[a:b]), ctx.to_device(lay.lens[a:b]), b - a)
            ctx.bg_count_order(part, K, bg=bg)
        assert np.array_equal(bg.to_host(), want)


@pytest.mark.parametrize("K", KS)
def test_one_sequence_of_70000_bases(ctx, K):
    c = mixed(8, [70_000])[0]
    check_counters(ctx, [c], K)
    c[np.random.default_rng(9).integers(0, 70_000, 50)] = 0
    c[[0, 69_999, 35_001]] = 0
    assert check_counters(ctx, [c], K) > 60_000  # (order 0 alone holds 69 947 valid bases)


def test_order_two_is_the_stratified_count_with_one_stratum(ctx, many):
    seqs = many[:20_000] + mixed(10, EDGE_LENGTHS, invalid=0.2)
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    for all_valid in (False, True):
        bg, _ = ctx.strata_bg_count(scan, ctx.to_device(np.zeros(len(seqs), np.uint16)), 1, 8, all_valid=all_valid)
        assert np.array_equal(ctx.bg_count_order(scan, 2, all_valid=all_valid).to_host(), bg.to_host()[0])


def test_argument_errors_write_nothing(ctx):
    seqs = mixed(10, [40, 50])
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    bg = ctx.to_device(np.full(bm.size(5), 7, np.uint64))
    for K, n in ((-1, 2), (6, 2), (100, 2), (3, 1 << 32)):
        with pytest.raises(pk.PengkError) as e:
            ctx.bg_count_order(scan, K, bg=bg, n_seq=n)
        assert e.value.code == pk.ERR_ARG and "pengk_bg_count_order" in str(e.value), (K, n)
    ptrs = [x.ptr for x in scan[:4]]
    call = lambda w, v, o, l, n, b: pk.lib().pengk_bg_count_order(ctx.h, w, v, o, l, n, 3, b)  # noqa: E731
    assert call(None, ptrs[1], ptrs[2], ptrs[3], 2, bg.ptr) == pk.ERR_ARG
    assert call(ptrs[0], ptrs[1], None, ptrs[3], 2, bg.ptr) == pk.ERR_ARG
    assert call(ptrs[0], ptrs[1], ptrs[2], None, 2, bg.ptr) == pk.ERR_ARG
    assert call(ptrs[0], ptrs[1], ptrs[2], ptrs[3], 2, None) == pk.ERR_ARG
    assert pk.lib().pengk_bg_count_order(None, ptrs[0], ptrs[1], ptrs[2], ptrs[3], 2, 3, bg.ptr) == pk.ERR_ARG
    assert call(None, None, None, None, 0, None) == 0
    ctx.bg_count_order(scan, 5, bg=bg, n_seq=0)
    ctx.synchronize()
    assert (bg.to_host() == 7).all()
    # d_valid may be null; the table is added to, not written; a lower order touches its own counters only
    ctx.bg_count_order(scan, 5, bg=bg)
    ctx.bg_count_order(scan, 5, bg=bg, all_valid=True)
    ctx.bg_count_order(scan, 3, bg=bg)
    want = 7 + 2 * bm.bg_count(seqs, 5)
    want[:bm.size(3)] += bm.bg_count(seqs, 3)
    assert np.array_equal(bg.to_host(), want)


# ---- entry 2 ------------------------------------------------------------------------------------------------------------------
def _describe(c, what, x, got, want):
    x = int(x)
    return ("%s differs: W = %d, %s, K = %d, V kind %s, ltot %d, k = %d, max_k = %d, control %s (Lc = %d, a = %g), pattern %d (%s), "
            "count %d: device %r (0x%08x), model %r (0x%08x)"
            % (what, c["W"], "both strands" if c["both"] else "plus strand", c["K"], c["kind"], c["ltot"], c["k"], c["max_k"],
               "none" if c["ctrl"] is None else ("mirrored" if c["ctrl_mirrored"] else "as built"), c["Lc"], c["a"], x,
               po.kmer_str(x, c["W"]), int(c["counts"][x]), float(got[x]), int(got[x:x + 1].view(np.uint32)[0]), float(want[x]),
               int(want[x:x + 1].view(np.uint32)[0])))


def _run_case(ctx, c, d_V, failures, pairs=(1,)):
    W, both = c["W"], c["both"]
    d_VK = pk.DeviceArray.from_host(ctx, c["VK"])
    d_lt = pk.DeviceArray.from_host(ctx, np.array([c["ltot"]], np.uint64))
    d_c = pk.DeviceArray.from_host(ctx, c["counts"])
    d_cc = d_cl = None
    if c["ctrl"] is not None:
        d_cc = pk.DeviceArray.from_host(ctx, c["ctrl"])
        d_cl = pk.DeviceArray.from_host(ctx, np.array([c["Lc"]], np.uint64))
    first = None
    for sp in pairs:
        ctx.set_option("sweep_pairs", sp)
        out = ctx.pattern_stats_order(W, both, c["k"], c["max_k"], d_V, c["K"], d_VK, d_lt, d_c, d_cc, d_cl, c["a"])
        got = [out[0].to_host(), out[1].to_host(), out[2].to_host(), out[3].to_host()]
        for o in range(c["max_k"] + 1):
            bad = _mismatch(got[0][o], c["bgp"][o])
            if bad.size:
                failures.append(_describe(c, "bgprob[%d]" % o, bad[0], got[0][o], c["bgp"][o]) + " (%d patterns)" % bad.size)
        for what, g, want, cmp in (("expected", got[1], c["expected"], _mismatch), ("z", got[3], c["z"], _mismatch),
                                   ("log-p", got[2], c["logp"], _beyond_one_ulp)):
            bad = cmp(g, want)
            if bad.size:
                failures.append(_describe(c, what, bad[0], g, want) + " (%d patterns)" % bad.size)
        if first is None:
            first = got
        else:  # sweep_pairs changes no bit
            assert all(a.tobytes() == b.tobytes() for a, b in zip(first, got))
        for d in out:
            d.free()
    for d in (d_VK, d_lt, d_c, d_cc, d_cl):
        if d is not None:
            d.free()


@pytest.mark.parametrize("both", [False, True], ids=["plus", "both"])
@pytest.mark.parametrize("W", [2, 4, 6, 8, 10])
def test_order_sweep_on_constructed_tables(ctx, W, both):
    failures = []
    d_V = pk.DeviceArray.from_host(ctx, tm.sweep_V("a"))
    for spec in bm.small_cases(W, both):
        _run_case(ctx, bm.case(W, both, spec), d_V, failures)
        if len(failures) > 20:
            break
    assert not failures, "%d mismatches, the first ones:\n%s" % (len(failures), "\n".join(failures[:8]))


def test_order_sweep_at_w12_with_sweep_pairs_on_and_off(ctx):
    failures = []
    try:
        c = bm.case(12, True, bm.big_case(12))
        _run_case(ctx, c, pk.DeviceArray.from_host(ctx, c["V"]), failures, pairs=(1, 0))
    finally:
        ctx.set_option("sweep_pairs", 1)
    assert not failures, "%d mismatches, the first ones:\n%s" % (len(failures), "\n".join(failures[:8]))


@pytest.mark.parametrize("both", [False, True], ids=["plus", "both"])
@pytest.mark.parametrize("W", [4, 10])
def test_order_two_is_the_plain_sweep_and_the_control_sweep(ctx, W, both):
    """K = 2 with the run's own table against the device's own pengk_pattern_stats / pengk_pattern_stats_control, every bit of
    every table -- log-p included: the same code made it"""
    counts = tm.edge_counts(W, mirrored=bool(both), salt=W + 9)
    ctrl = tm.edge_counts(W, (0, 1, 2, 3), mirrored=False, salt=W + 10)
    d_c, d_cc = ctx.to_device(counts), ctx.to_device(ctrl)
    d_lt, d_cl = ctx.to_device(np.array([tm.LTOTS[1]], np.uint64)), ctx.to_device(np.array([3_000_017], np.uint64))
    for kind in "abc":
        d_V = ctx.to_device(tm.sweep_V(kind))
        for k in (0, 1, 2):
            for control in (False, True):
                if control:
                    got = ctx.pattern_stats_order(W, both, k, 2, d_V, 2, d_V, d_lt, d_c, d_cc, d_cl, 0.5)
                    want = ctx.pattern_stats_control(W, both, k, 2, d_V, d_lt, d_c, d_cc, d_cl, 0.5)
                else:
                    got = ctx.pattern_stats_order(W, both, k, 2, d_V, 2, d_V, d_lt, d_c)
                    want = ctx.pattern_stats(W, both, k, 2, d_V, d_lt, d_c)
                for name, g, t in zip(("bgprob", "expected", "logp", "z"), got, want):
                    assert g.to_host().tobytes() == t.to_host().tobytes(), (kind, k, control, name)


@pytest.mark.parametrize("K", [0, 1, 2])
def test_model_at_low_orders_is_the_devices_bg_model(ctx, K):
    """pengk_bg_model_order at K <= 2 against pengk_bg_model (the device's calculateV, which tests/test_gpu_table_edges.py pins
    to the compiled reference's and with it to BackgroundModel::modelOf) on the same counters: bit for bit"""
    for kind in tm.COUNTER_KINDS:
        n84 = np.asarray(tm._counter_set(kind), np.int64).astype(np.uint64)
        for alpha in tm.ALPHAS:
            want = ctx.bg_model(ctx.to_device(n84), K, alpha).to_host()
            got = pk.bg_model_order(n84, K, alpha[:K + 1], True)
            assert got.tobytes() == want[:bm.size(K)].tobytes(), (kind, alpha)
    n = bm.counters("random", 5, seed=3)   # and the low orders of a K = 5 model are the K = 2 model's
    assert pk.bg_model_order(n, 5, (1.0,) * 6)[:84].tobytes() == ctx.bg_model(ctx.to_device(n[:84].copy()), 2).to_host().tobytes()


def test_order_sweep_argument_errors(ctx):
    W = 4
    d_V = ctx.to_device(tm.sweep_V("a"))
    d_VK = ctx.to_device(bm.sweep_VK("dirichlet", 5))
    d_c = ctx.to_device(tm.edge_counts(W))
    d_lt = ctx.to_device(np.array([1000], np.uint64))
    bad = [dict(K=-1), dict(K=6), dict(W=3), dict(W=0), dict(W=16), dict(k=2, max_k=1), dict(max_k=3), dict(k=-1),
           dict(ctrl_counts=d_c), dict(ctrl_ltot=d_lt), dict(pseudocount=1.0),
           dict(ctrl_counts=d_c, ctrl_ltot=d_lt, pseudocount=-1.0), dict(ctrl_counts=d_c, ctrl_ltot=d_lt, pseudocount=float("nan"))]
    for kw in bad:
        a = dict(W=W, k=0, max_k=1, K=5, ctrl_counts=None, ctrl_ltot=None, pseudocount=0.0)
        a.update(kw)
        with pytest.raises(pk.PengkError) as e:
            ctx.pattern_stats_order(a["W"], True, a["k"], a["max_k"], d_V, a["K"], d_VK, d_lt, d_c, a["ctrl_counts"], a["ctrl_ltot"],
                                    a["pseudocount"])
        assert e.value.code == pk.ERR_ARG, kw
    out = ctx.pattern_stats_order(W, True, 0, 1, d_V, 5, d_VK, d_lt, d_c)
    for which in (5, 7):  # d_V, d_VK
        args = [ctx.h, W, 1, 0, 1, d_V.ptr, 5, d_VK.ptr, d_lt.ptr, d_c.ptr, None, None, 0.0] + [o.ptr for o in out]
        args[which] = None
        assert pk.lib().pengk_pattern_stats_order(*args) == pk.ERR_ARG
    ctx.synchronize()


# ---- both entries behind the gate ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gate():
    return sg.Gate(0)


@pytest.fixture(scope="module")
def gated_ctx(gate):
    sg.positive_control(gate)  # (raises when the set-up cannot see a copy that overtakes the gate)
    c = pk.Context(0)
    c.set_stream(gate.s)
    yield c
    c.close()


G_K, G_W = 5, 8


def _gated_inputs(poison):
    seqs, lay = sg.scan_layout(poison)
    V = tm.sweep_V("b" if poison else "a")
    VK = bm.sweep_VK("denormal" if poison else "dirichlet", G_K, seed=int(poison))
    counts = tm.edge_counts(G_W, mirrored=True, salt=40 + int(poison))
    ltot = np.array([tm.LTOTS[1 + int(poison)]], np.uint64)
    return seqs, V, VK, counts, ltot


def _gated_want(poison):
    seqs, V, VK, counts, ltot = _gated_inputs(poison)
    m, e, lp, z = bm.sweep(G_W, True, 2, 2, V, G_K, VK, counts, int(ltot[0]))
    return dict(bg=bm.bg_count(seqs, G_K), bgprob=np.stack(m), expected=e, logp=lp, z=z)


def test_both_entries_in_stream_order_without_host_waits(gated_ctx, gate):
    """the counters of a scan layout, then the order-K sweep on tables of its own: inputs that hold poison until the gate has
    passed, outputs copied right behind the call that wrote them, one host wait at the end"""
    ctx = gated_ctx
    ch = sg.Chain(gate)
    real, poison = _gated_inputs(False), _gated_inputs(True)
    want, other = _gated_want(False), _gated_want(True)
    assert not np.array_equal(want["bg"], other["bg"]) and want["z"].tobytes() != other["z"].tobytes()
    scan = sg.scan_buffers(ch)
    b = dict(V=ch.inp("V", real[1], poison[1]), VK=ch.inp("VK", real[2], poison[2]), counts=ch.inp("counts", real[3], poison[3]),
             ltot=ch.inp("ltot", real[4], poison[4]))
    for name, w in want.items():
        b[name] = ch.out(name, w.shape, w.dtype, added_to=name == "bg")

    def steps():
        ctx.bg_count_order(scan, G_K, bg=b["bg"])
        ch.take("bg")
        yield
        ctx.pattern_stats_order(G_W, True, 2, 2, b["V"], G_K, b["VK"], b["ltot"], b["counts"], bgprob=b["bgprob"],
                                expected=b["expected"], logp=b["logp"], z=b["z"])
        ch.take("bgprob", "expected", "logp", "z")
        yield

    def check(got):
        assert set(got) == set(want)
        sg.check_bits({"bg": got["bg"]}, want)
        for name in ("bgprob", "expected", "z"):  # (bit for bit; NaN agrees in position)
            assert not _mismatch(got[name].reshape(-1), want[name].reshape(-1)).size, name
        assert not _beyond_one_ulp(got["logp"], want["logp"]).size

    through_the_gate("bg_order", ch, steps, check, True)
