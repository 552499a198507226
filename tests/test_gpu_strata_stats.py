"""The two device entries of --stratified-background (include/pengk.h, "a GC-stratified null for the sweep") against the
numpy model of tests/strata_stats_model.py, bit for bit.

pengk_strata_bg_count: sequences of 0 .. 65 bases and at every length where a word of the layout or a tile of 64 positions
ends; an invalid base at the positions where an order loses its context, a half, a word or the sequence ends, and pairs one
and two apart; without input validity; strata that are ignored; 1 and 16 strata; the hottest bins (100 000 x 40 bases, all
A, one stratum); 100 000 short sequences over 16 strata; one sequence of 70 000 bases; a subset of the offset arrays; two
calls; the windows at W = 2 and 14; the argument errors.

pengk_pattern_stats_strata: on the V kinds and the count edges of tests/table_edges_model.py, every legal (k, max_k), both
strand settings, 1 / 2 / 3 / 16 strata, weights among 0, 1, 2^40 and 3 000 017, with and without the control tables of
tests/control_stats_model.py; one non-zero weight against pengk_pattern_stats and pengk_pattern_stats_control themselves;
W = 12 once; sweep_pairs on and off.  Bars, those of tests/test_gpu_table_edges.py: bgprob, expected and z bit for bit,
log-p within one float ulp.

Both entries once behind the gate of tests/stream_gate.py on a caller-owned stream: right order, no host wait."""
import numpy as np
import pytest
import torch  # noqa: F401  (the gate's streams are torch's: its HIP runtime is loaded before the library's, whichever test runs first)

import control_stats_model as cm
import peng_motif_amd as pk
import motif_score_model as ms
import strata_stats_model as sm
import stream_gate as sg
import table_edges_model as tm
from oracle import oracle as po
from test_gpu_stream_order import through_the_gate
from test_gpu_table_edges import _beyond_one_ulp, _mismatch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = pk.Context(0)
    yield c
    c.close()


# ---- entry 1 ------------------------------------------------------------------------------------------------------------------
def check_counters(ctx, seqs, stratum, S, W, all_valid=False, scan=None, want=None):
    if scan is None:
        scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    bg, win = ctx.strata_bg_count(scan, ctx.to_device(np.ascontiguousarray(stratum, np.uint16)), S, W, all_valid=all_valid)
    wb, ww = want if want is not None else sm.bg_count(seqs, stratum, S, W, all_valid)
    gb, gw = bg.to_host(), win.to_host()
    bad = np.argwhere(gb != wb)
    assert len(bad) == 0, "S %d W %d: stratum %d counter %d: %d, the model %d (%d counters differ)" % (
        S, W, bad[0][0], bad[0][1], gb[tuple(bad[0])], wb[tuple(bad[0])], len(bad))
    assert np.array_equal(gw, ww), "S %d W %d windows: %s, the model %s" % (S, W, gw.tolist(), ww.tolist())
    return int(wb.sum())


def skewed(seed, lengths, invalid=0.0):
    """sequences of every composition from all-AT to all-GC (so that every GC bin is met), some with invalid bases"""
    rng = np.random.default_rng(seed)
    out = []
    for k, L in enumerate(lengths):
        gc = (k % 11) / 10.0
        c = (rng.choice(4, L, p=[(1 - gc) / 2, gc / 2, gc / 2, (1 - gc) / 2]) + 1).astype(np.uint8)
        if invalid and L:
            c[rng.random(L) < invalid] = 0
        out.append(c)
    return out


EDGE_LENGTHS = [0, 1, 2, 3, 31, 32, 33, 64, 65, 15, 16, 17, 63, 127, 128, 129, 130]


@pytest.mark.parametrize("S", [1, 10, 16])
def test_lengths_at_the_edges(ctx, S):
    seqs = skewed(1, EDGE_LENGTHS * 4) + skewed(2, EDGE_LENGTHS * 2, invalid=0.1)
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    stratum = sm.gc_strata(seqs, S)
    assert S == 1 or len(set(stratum.tolist()) - {sm.NONE}) == S
    for W in (2, 8, 14):
        assert check_counters(ctx, seqs, stratum, S, W, scan=scan) > 0
        check_counters(ctx, seqs, stratum, S, W, all_valid=True, scan=scan)
    for c in seqs[1:len(EDGE_LENGTHS)]:  # every length alone
        check_counters(ctx, [c], [0], 1, 2)


def test_invalid_bases_where_a_context_a_word_or_the_sequence_ends(ctx):
    base = skewed(3, [5] * 5 + [70])[5]
    seqs = []
    for at in ([0], [1], [2], [31], [32], [69], [10, 11], [10, 12], [31, 32], [63, 64], [62, 64], [0, 1], [0, 2], [68, 69], list(range(70))):
        c = base.copy()
        c[at] = 0
        seqs.append(c)
    for p in range(70):  # and one at every position in turn
        c = base.copy()
        c[p] = 0
        seqs.append(c)
    stratum = sm.gc_strata(seqs, 4)
    assert stratum[14] == sm.NONE
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    for W in (2, 14):
        check_counters(ctx, seqs, stratum, 4, W, scan=scan)
    for i in range(15):
        check_counters(ctx, [seqs[i]], [0], 1, 6)


def test_strata_out_of_range_are_ignored(ctx):
    seqs = skewed(4, [40, 50, 60, 70, 80, 90])
    for stratum, S in (([0, 1, 2, 3, 0xFFFF, 16], 3), ([5, 0xFFFF, 15, 16, 255, 0], 16), ([1, 1, 1, 1, 1, 1], 1), ([0xFFFF] * 6, 16)):
        check_counters(ctx, seqs, stratum, S, 8)


def test_the_hottest_bins(ctx):
    """100 000 x 40 bases, all A, one stratum: three counters take everything"""
    n, L = 100_000, 40
    seqs = [np.ones(L, np.uint8)] * n
    want = np.zeros((1, 84), np.uint64)
    want[0, 0], want[0, 4], want[0, 20] = n * L, n * (L - 1), n * (L - 2)
    check_counters(ctx, seqs, np.zeros(n, np.uint16), 1, 14, want=(want, np.array([n * (L - 13)], np.uint64)))


@pytest.fixture(scope="module")
def many():
    rng = np.random.default_rng(5)
    pool = skewed(6, rng.integers(0, 80, 500).tolist(), invalid=0.02)
    idx = rng.integers(0, len(pool), 100_000)
    seqs = [pool[i] for i in idx]
    return seqs, sm.gc_strata(seqs, 16)


def test_100000_short_sequences_over_16_strata(ctx, many):
    seqs, stratum = many
    assert len(set(stratum.tolist()) - {sm.NONE}) == 16
    check_counters(ctx, seqs, stratum, 16, 8)


def test_a_subset_and_two_calls(ctx, many):
    seqs, stratum = many
    lay = pk.ScanLayout(*ms.flatten(seqs))
    words, valid = ctx.to_device(lay.words), ctx.to_device(lay.valid)
    n = len(seqs)
    pick = np.flatnonzero(np.random.default_rng(7).random(n) < 0.3)[::-1].copy()   # (not contiguous, and in another order)
    part = (words, valid, ctx.to_device(lay.offs[pick]), ctx.to_device(lay.lens[pick]), len(pick))
    check_counters(ctx, [seqs[i] for i in pick], stratum[pick], 16, 8, scan=part)
    want = sm.bg_count(seqs, stratum, 16, 10)
    for cut in (1, 50_001):
        bg, win = ctx.to_device(np.zeros((16, 84), np.uint64)), ctx.to_device(np.zeros(16, np.uint64))
        for a, b in ((0, cut), (cut, n)):
            part = (words, valid, ctx.to_device(lay.offs[a:b]), ctx.to_device(lay.lens[a:b]), b - a)
            ctx.strata_bg_count(part, ctx.to_device(stratum[a:b].copy()), 16, 10, bg=bg, windows=win)
        assert np.array_equal(bg.to_host(), want[0]) and np.array_equal(win.to_host(), want[1])


def test_one_sequence_of_70000_bases(ctx):
    c = skewed(8, [70_000])[0]
    check_counters(ctx, [c], [2], 3, 14)
    c[np.random.default_rng(9).integers(0, 70_000, 50)] = 0
    c[[0, 69_999, 35_001]] = 0
    assert check_counters(ctx, [c], [0], 1, 2) > 200_000


def test_argument_errors_write_nothing(ctx):
    seqs = skewed(10, [40, 50])
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    st = ctx.to_device(np.zeros(2, np.uint16))
    bg, win = ctx.to_device(np.full((16, 84), 7, np.uint64)), ctx.to_device(np.full(16, 7, np.uint64))
    for S, W, n in ((0, 8, 2), (17, 8, 2), (-1, 8, 2), (4, 7, 2), (4, 0, 2), (4, 16, 2), (4, -2, 2), (4, 8, 1 << 32)):
        with pytest.raises(pk.PengkError) as e:
            ctx.strata_bg_count(scan, st, S, W, bg=bg, windows=win, n_seq=n)
        assert e.value.code == pk.ERR_ARG and "pengk_strata_bg_count" in str(e.value), (S, W, n)
    ptrs = [x.ptr for x in scan[:4]]
    call = lambda w, v, o, l, n, s, b, wi: pk.lib().pengk_strata_bg_count(ctx.h, w, v, o, l, n, s, 4, 8, b, wi)  # noqa: E731
    assert call(None, ptrs[1], ptrs[2], ptrs[3], 2, st.ptr, bg.ptr, win.ptr) == pk.ERR_ARG
    assert call(ptrs[0], ptrs[1], None, ptrs[3], 2, st.ptr, bg.ptr, win.ptr) == pk.ERR_ARG
    assert call(ptrs[0], ptrs[1], ptrs[2], None, 2, st.ptr, bg.ptr, win.ptr) == pk.ERR_ARG
    assert call(ptrs[0], ptrs[1], ptrs[2], ptrs[3], 2, None, bg.ptr, win.ptr) == pk.ERR_ARG
    assert call(ptrs[0], ptrs[1], ptrs[2], ptrs[3], 2, st.ptr, None, win.ptr) == pk.ERR_ARG
    assert call(None, None, None, None, 0, None, None, None) == 0
    ctx.strata_bg_count(scan, st, 4, 8, bg=bg, windows=win, n_seq=0)
    ctx.synchronize()
    assert (bg.to_host() == 7).all() and (win.to_host() == 7).all()
    # d_valid and d_windows may be null; the tables are added to, not written
    want, ww = sm.bg_count(seqs, [0, 0], 16, 8)
    ctx.strata_bg_count(scan, st, 16, 8, bg=bg, want_windows=False)
    ctx.strata_bg_count(scan, st, 16, 8, bg=bg, windows=win, all_valid=True)
    assert np.array_equal(bg.to_host(), 7 + 2 * want) and np.array_equal(win.to_host(), 7 + ww)


# ---- entry 2 ------------------------------------------------------------------------------------------------------------------
def _describe(c, what, x, got, want):
    x = int(x)
    return ("%s differs: W = %d, %s, %d strata, weights %s, ltot %d, k = %d, max_k = %d, control %s (Lc = %d, a = %g), pattern %d (%s), "
            "count %d: device %r (0x%08x), model %r (0x%08x)"
            % (what, c["W"], "both strands" if c["both"] else "plus strand", c["S"], c["windows"].tolist(), c["ltot"], c["k"],
               c["max_k"], "none" if c["ctrl"] is None else ("mirrored" if c["ctrl_mirrored"] else "as built"), c["Lc"], c["a"], x,
               po.kmer_str(x, c["W"]), int(c["counts"][x]), float(got[x]), int(got[x:x + 1].view(np.uint32)[0]), float(want[x]),
               int(want[x:x + 1].view(np.uint32)[0])))


def _run_case(ctx, c, d_V, failures, pairs=(1,)):
    W, both = c["W"], c["both"]
    d_lt = pk.DeviceArray.from_host(ctx, np.array([c["ltot"]], np.uint64))
    d_c = pk.DeviceArray.from_host(ctx, c["counts"])
    d_cc = d_cl = None
    if c["ctrl"] is not None:
        d_cc = pk.DeviceArray.from_host(ctx, c["ctrl"])
        d_cl = pk.DeviceArray.from_host(ctx, np.array([c["Lc"]], np.uint64))
    first = None
    for sp in pairs:
        ctx.set_option("sweep_pairs", sp)
        out = ctx.pattern_stats_strata(W, both, c["k"], c["max_k"], d_V, c["windows"], d_lt, d_c, d_cc, d_cl, c["a"])
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
    for d in (d_lt, d_c, d_cc, d_cl):
        if d is not None:
            d.free()


@pytest.mark.parametrize("both", [False, True], ids=["plus", "both"])
@pytest.mark.parametrize("W", [2, 4, 6, 8, 10])
def test_stratified_sweep_on_constructed_tables(ctx, W, both):
    failures = []
    d_V = {}
    for spec in sm.small_cases(W, both):
        c = sm.case(W, both, spec)
        if c["S"] not in d_V:
            d_V[c["S"]] = pk.DeviceArray.from_host(ctx, c["V"])
        _run_case(ctx, c, d_V[c["S"]], failures)
        if len(failures) > 20:
            break
    assert not failures, "%d mismatches, the first ones:\n%s" % (len(failures), "\n".join(failures[:8]))


def test_stratified_sweep_at_w12_with_sweep_pairs_on_and_off(ctx):
    failures = []
    try:
        c = sm.case(12, True, sm.big_case(12))
        _run_case(ctx, c, pk.DeviceArray.from_host(ctx, c["V"]), failures, pairs=(1, 0))
    finally:
        ctx.set_option("sweep_pairs", 1)
    assert not failures, "%d mismatches, the first ones:\n%s" % (len(failures), "\n".join(failures[:8]))


@pytest.mark.parametrize("both", [False, True], ids=["plus", "both"])
@pytest.mark.parametrize("W", [4, 10])
def test_one_non_zero_weight_is_the_plain_sweep_and_the_control_sweep(ctx, W, both):
    """against the device's own pengk_pattern_stats / pengk_pattern_stats_control on the stratum's table, every bit of every
    table -- log-p included: the same code made it"""
    S, k, mk = 3, min(1, W - 1), min(2, W - 1)
    Vs = sm.stratum_V(S)
    d_V = ctx.to_device(Vs)
    counts = tm.edge_counts(W, mirrored=bool(both), salt=W + 9)
    ctrl = tm.edge_counts(W, (0, 1, 2, 3), mirrored=False, salt=W + 10)
    d_c, d_cc = ctx.to_device(counts), ctx.to_device(ctrl)
    d_lt, d_cl = ctx.to_device(np.array([tm.LTOTS[1]], np.uint64)), ctx.to_device(np.array([3_000_017], np.uint64))
    for s, w in ((0, 1), (1, 2 ** 40), (2, 3_000_017), (1, 2 ** 64 - 1)):
        windows = np.zeros(S, np.uint64)
        windows[s] = w
        d_Vs = ctx.to_device(Vs[s])
        for control in (False, True):
            if control:
                got = ctx.pattern_stats_strata(W, both, k, mk, d_V, windows, d_lt, d_c, d_cc, d_cl, 0.5)
                want = ctx.pattern_stats_control(W, both, k, mk, d_Vs, d_lt, d_c, d_cc, d_cl, 0.5)
            else:
                got = ctx.pattern_stats_strata(W, both, k, mk, d_V, windows, d_lt, d_c)
                want = ctx.pattern_stats(W, both, k, mk, d_Vs, d_lt, d_c)
            for name, g, t in zip(("bgprob", "expected", "logp", "z"), got, want):
                assert g.to_host().tobytes() == t.to_host().tobytes(), (s, w, control, name)


def test_stratified_sweep_argument_errors(ctx):
    W = 4
    d_V = ctx.to_device(sm.stratum_V(16))
    d_c = ctx.to_device(tm.edge_counts(W))
    d_lt = ctx.to_device(np.array([1000], np.uint64))
    ones = np.ones(16, np.uint64)
    bad = [dict(windows=np.zeros(3, np.uint64)), dict(windows=ones, n_strata=0), dict(windows=ones, n_strata=17),
           dict(windows=np.array([2 ** 63, 2 ** 63], np.uint64)), dict(windows=ones, W=3), dict(windows=ones, W=0),
           dict(windows=ones, k=2, max_k=1), dict(windows=ones, max_k=3), dict(windows=ones, ctrl_counts=d_c),
           dict(windows=ones, ctrl_ltot=d_lt), dict(windows=ones, pseudocount=1.0),
           dict(windows=ones, ctrl_counts=d_c, ctrl_ltot=d_lt, pseudocount=-1.0),
           dict(windows=ones, ctrl_counts=d_c, ctrl_ltot=d_lt, pseudocount=float("nan"))]
    for kw in bad:
        a = dict(W=W, k=0, max_k=1, ctrl_counts=None, ctrl_ltot=None, pseudocount=0.0, n_strata=None)
        a.update(kw)
        with pytest.raises(pk.PengkError) as e:
            ctx.pattern_stats_strata(a["W"], True, a["k"], a["max_k"], d_V, a["windows"], d_lt, d_c, a["ctrl_counts"], a["ctrl_ltot"],
                                     a["pseudocount"], n_strata=a["n_strata"])
        assert e.value.code == pk.ERR_ARG, kw
    ctx.pattern_stats_strata(W, True, 0, 1, d_V, ones, d_lt, d_c)
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


G_S, G_W = 10, 8


def _gated_inputs(poison):
    seqs, lay = sg.scan_layout(poison)
    stratum = sm.gc_strata(seqs, G_S)
    Vs = sm.stratum_V(2 * 3)[3:] if poison else sm.stratum_V(3)
    counts = tm.edge_counts(G_W, mirrored=True, salt=40 + int(poison))
    ltot = np.array([tm.LTOTS[1 + int(poison)]], np.uint64)
    return seqs, stratum, Vs, counts, ltot


GATED_WEIGHTS = np.array([3_000_017, 1, 2 ** 40], np.uint64)


def _gated_want(poison):
    seqs, stratum, Vs, counts, ltot = _gated_inputs(poison)
    bg, win = sm.bg_count(seqs, stratum, G_S, G_W)
    p = sm.markov_tables(G_W, Vs, True, 2)
    m, e, lp, z = sm.sweep(G_W, counts, int(ltot[0]), p, GATED_WEIGHTS, 2)
    return dict(bg=bg, windows=win, bgprob=np.stack(m), expected=e, logp=lp, z=z)


def test_both_entries_in_stream_order_without_host_waits(gated_ctx, gate):
    """the counters of a scan layout and its strata, then the stratified sweep on tables of its own: inputs that hold poison
    until the gate has passed, outputs copied right behind the call that wrote them, one host wait at the end"""
    ctx = gated_ctx
    ch = sg.Chain(gate)
    real, poison = _gated_inputs(False), _gated_inputs(True)
    want, other = _gated_want(False), _gated_want(True)
    assert not np.array_equal(want["bg"], other["bg"]) and want["z"].tobytes() != other["z"].tobytes()
    scan = sg.scan_buffers(ch)
    b = dict(stratum=ch.inp("stratum", real[1], poison[1]), V=ch.inp("V", real[2], poison[2]),
             counts=ch.inp("counts", real[3], poison[3]), ltot=ch.inp("ltot", real[4], poison[4]))
    for name, w in want.items():
        b[name] = ch.out(name, w.shape, w.dtype, added_to=name in ("bg", "windows"))

    def steps():
        ctx.strata_bg_count(scan, b["stratum"], G_S, G_W, bg=b["bg"], windows=b["windows"])
        ch.take("bg", "windows")
        yield
        ctx.pattern_stats_strata(G_W, True, 2, 2, b["V"], GATED_WEIGHTS, b["ltot"], b["counts"], bgprob=b["bgprob"],
                                 expected=b["expected"], logp=b["logp"], z=b["z"])
        ch.take("bgprob", "expected", "logp", "z")
        yield

    def check(got):
        assert set(got) == set(want)
        sg.check_bits({k: got[k] for k in ("bg", "windows")}, want)
        for name in ("bgprob", "expected", "z"):  # (bit for bit; NaN agrees in position)
            assert not _mismatch(got[name].reshape(-1), want[name].reshape(-1)).size, name
        assert not _beyond_one_ulp(got["logp"], want["logp"]).size

    through_the_gate("strata", ch, steps, check, True)
