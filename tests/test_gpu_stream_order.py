"""The stream contract of include/pengk.h, pinned behind the gate of tests/stream_gate.py: work is enqueued on the
context's stream and in its order, calls that take only d_ pointers do not wait on the host, pengk_set_stream re-targets a
context to a caller-owned stream.

Every device buffer is a torch tensor on one torch stream s that the context is re-targeted to.  The inputs hold poison
while bounded device work (torch.cuda._sleep) keeps s busy; behind it copies on s bring the real input, the library calls
follow with no host wait of the test's own, every output is copied on s right behind the call that wrote it, and only
then the host waits, once.  A launch, memset or copy on any other stream, a side stream of the EM that is not forked from
or joined to s, or a blocking copy that is not ordered against s runs while the gate is busy and reads poison or is
overwritten.  The expected values are the oracle's and the numpy models' (tests/test_stream_order_cpu.py shows that they
differ under the poison); nothing the device computed is used as truth.  Every chain runs twice un-gated first: the first
run takes the first-use work (scratch growth, the EM's side streams and counters), the second gives the host time to
enqueue the chain, from which the gate's length follows: 20 times that, at least 50 ms, at most 400 ms.

Measured on an MI355X (every run measures again and prints its figures at the end of the module; pytest -s shows them):
  torch.cuda._sleep    2.40e6 cycles per millisecond (2 389 406 and 2 397 333 in two runs: the shader clock)
  longest chain        of the d_-only ones, (a) at W = 10 on both strands with em_overlap = 2: 0.39 .. 0.45 ms of host time
                       to enqueue (W = 8: 0.18 .. 0.38 ms; (b): 0.14 ms); chain (c), whose calls wait on entry: 1.49 ms
  the gate             20 times either is below the floor: 50.0 ms asked for = 119 866 638 cycles, 49.9 ms by torch events
                       in every test; the gated enqueue of (a) took 0.35 .. 0.39 ms of host time, that of (c) 51.3 ms (its
                       first call waits for the gate)
  timers               50.5 ms between pengk_timer_record before the gate and behind chain (a), the gate 49.9 ms
  positive control     the first fresh stream saw the poison
  sensitivity          by hand, on a scratch build with pengk_seq_strata's launch moved to the null stream: the gated
                       chain (b) fails (300 of 300 strata are the 0xA5 bytes the production wrote over the early result);
                       both un-gated runs before it pass
"""
import numpy as np
import pytest

import peng_motif_amd as pk
import stream_gate as sg

pytestmark = pytest.mark.gpu

FIGURES = []  # what the runs measured, printed at the end of the module


@pytest.fixture(scope="module")
def gate():
    g = sg.Gate(0)
    FIGURES.append("torch.cuda._sleep: %.0f cycles per ms" % g.cycles_per_ms)
    yield g
    print("\n" + "\n".join(FIGURES))


@pytest.fixture(scope="module")
def control(gate):
    """once per module, before any gated test: the set-up can see a copy that overtakes the gate"""
    tries, on_s_real = sg.positive_control(gate)
    FIGURES.append("positive control: poison seen on fresh stream number %d" % tries)
    return tries, on_s_real


@pytest.fixture(scope="module")
def ctx(gate, control):
    c = pk.Context(0)
    c.set_stream(gate.s)
    c.set_option("em_fast", 2)
    yield c
    c.close()


def through_the_gate(label, ch, steps, check, d_only, before_gate=None, after_chain=None, gate_ms=None):
    """twice un-gated, then behind the gate; d_only: the host must not have waited for the gate"""
    for _ in range(2):
        ch.arm(None)
        enqueue_ms = sg.run(steps())
        check(ch.finish())
    target = sg.Gate.length_ms(enqueue_ms) if gate_ms is None else gate_ms
    ch.arm(target, before_gate)
    host_ms = sg.run(steps())
    if after_chain is not None:
        after_chain()
    pending = ch.pending()
    got = ch.finish()
    FIGURES.append("%s: enqueue %.3f ms un-gated, %.3f ms gated; gate %.1f ms asked = %d cycles, %.1f ms measured" % (
        label, enqueue_ms, host_ms, target, ch.g.cycles(target), ch.gate_ms()))
    if d_only:
        assert pending, "%s: the stream was idle after the last enqueue (%.2f ms of host time, gate %.1f ms): a host wait" % (
            label, host_ms, ch.gate_ms())
    check(got)
    return dict(enqueue_ms=enqueue_ms, host_ms=host_ms, target_ms=target, gate_ms=ch.gate_ms())


def test_positive_control_saw_poison(control):
    tries, on_s_real = control
    assert 1 <= tries <= 4  # (positive_control raises when no stream saw it)
    assert on_s_real  # ... and the same copy on s itself waited for the gate and the production


# ---- a. the count path ----------------------------------------------------------------------------------------------------
def chain_a(ctx, gate, W, both, whole, label, overlap=2, **kw):
    ch = sg.Chain(gate)
    b, case = sg.chain_a_buffers(ch, W, both, whole)
    ctx.set_option("em_overlap", overlap)
    try:
        return through_the_gate(label, ch, lambda: sg.chain_a_steps(ctx, ch, b, case, W, both, whole),
                                lambda got: sg.check_chain_a(got, case["want"]), True, **kw)
    finally:
        ctx.set_option("em_overlap", 2)


@pytest.mark.parametrize("whole", [False, True], ids=["invalid_bases", "whole"])
@pytest.mark.parametrize("W,both", sg.A_CONFIGS)
def test_count_path_in_stream_order_without_host_waits(ctx, gate, W, both, whole):
    """set_sequences on torch tensors, count, mirror, bg_model, pattern_stats, em_device (em_fast = 2, 16 PWMs, 3
    iterations, two lanes from W = 10 on).  pengk_count_bg is defined for whole sequences only, so the input with invalid
    bases goes through pengk_count with the packer's background counters as a gated input, and the same input without
    them through pengk_count_bg."""
    chain_a(ctx, gate, W, both, whole, "a W=%d %s %s" % (W, "both" if both else "plus", "whole" if whole else "invalid"))


def test_count_path_with_one_em_lane(ctx, gate):
    chain_a(ctx, gate, 10, True, False, "a W=10 both invalid em_overlap=1", overlap=1)


# ---- b. the scan layout, d_ pointers only ------------------------------------------------------------------------------------
def test_scan_layout_calls_in_stream_order_without_host_waits(ctx, gate):
    """mask_low_complexity, then dyad_count, seq_strata and shuffle_sequences on the masked validity (each reads what the
    first wrote; the first two share one scratch buffer under different layouts), then synth_scan_sequences"""
    ch = sg.Chain(gate)
    b, want = sg.chain_b_buffers(ch)
    through_the_gate("b", ch, lambda: sg.chain_b_steps(ctx, ch, b), lambda got: sg.check_bits(got, want), True)


# ---- c. calls that stage host parameters ---------------------------------------------------------------------------------------
def test_staging_calls_back_to_back(ctx, gate):
    """motif_scan, score_histograms, sites_count, mask_sites, motif_best_sites, centrality_histograms with motifs and
    thresholds of their own, no host wait between them: each may wait on entry (no query() here) and returns with its
    kernels in flight -- the next call's staging into the shared scratch must not overtake them"""
    ch = sg.Chain(gate)
    b, want = sg.chain_c_buffers(ch)
    through_the_gate("c", ch, lambda: sg.chain_c_steps(ctx, ch, b), lambda got: sg.check_bits(got, want), False)


# ---- d. pengk_set_stream itself ----------------------------------------------------------------------------------------------
def test_set_stream_waits_for_the_old_stream_and_moves_the_work(gate, control):
    torch = gate.torch
    W, both, whole = 8, True, False
    c = pk.Context(0)
    try:
        own = c.stream()
        assert own not in (0, gate.s.cuda_stream)  # pengk_create made a stream of its own
        c.set_stream(gate.s)
        assert c.stream() == gate.s.cuda_stream
        ch = sg.Chain(gate)
        b, case = sg.chain_a_buffers(ch, W, both, whole)
        steps = lambda: sg.chain_a_steps(c, ch, b, case, W, both, whole)
        for _ in range(2):
            ch.arm(None)
            sg.run(steps())
            sg.check_chain_a(ch.finish(), case["want"])
        # a gated chain is pending on the old stream: set_stream returns only when it is done
        other = torch.cuda.Stream(device=gate.dev)
        ch.arm(100.0)
        sg.run(steps())
        assert ch.pending()
        c.set_stream(other)
        assert gate.s.query() and c.stream() == other.cuda_stream
        sg.check_chain_a(ch.finish(), case["want"])
        assert ch.gate_ms() >= 50.0
        # ... and the context now works on the new stream: the same chain behind a gate on it
        ch2 = sg.Chain(gate.on(other))
        b2, _ = sg.chain_a_buffers(ch2, W, both, whole)
        through_the_gate("d on the new stream", ch2, lambda: sg.chain_a_steps(c, ch2, b2, case, W, both, whole),
                         lambda got: sg.check_chain_a(got, case["want"]), True)
        # the null stream: still the oracle's count
        c.set_stream(None)
        assert c.stream() == 0
        c.upload(case["packed"])
        counts, ltot = c.count(both)
        c.mirror(W, counts)
        assert int(ltot.to_host()[0]) == int(case["want"]["ltot"][0])
        assert np.array_equal(counts.to_host(), case["want"]["counts"])
        c.set_stream(gate.s.cuda_stream)  # (a hipStream_t as an int)
        assert c.stream() == gate.s.cuda_stream
    finally:
        c.close()
    # the caller's streams outlive the context
    for s in (gate.s, other):
        with torch.cuda.stream(s):
            x = torch.arange(1000, device=gate.dev).sum()
        s.synchronize()
        assert int(x) == 499500


def test_timers_follow_the_contexts_stream(ctx, gate):
    """pengk_timer_record before the gate and behind chain (a): by ordering the interval contains the gate (0.1 for the
    events' resolution)"""
    t0, t1 = ctx.timer(), ctx.timer()
    try:
        r = chain_a(ctx, gate, 10, True, True, "d timers", before_gate=lambda: ctx.record(t0), after_chain=lambda: ctx.record(t1))
        ms = ctx.elapsed_ms(t0, t1)
        FIGURES.append("d timers: %.1f ms between the library's events, the gate %.1f ms" % (ms, r["gate_ms"]))
        assert r["gate_ms"] >= 0.9 * r["target_ms"]
        assert ms >= 0.9 * r["gate_ms"]
    finally:
        pk.lib().pengk_timer_destroy(ctx.h, t0)
        pk.lib().pengk_timer_destroy(ctx.h, t1)


# ---- e. two contexts, two streams, two inputs ------------------------------------------------------------------------------------
def test_two_contexts_on_two_streams_interleaved(gate, control):
    """each context's scratch is its own: the chains of two contexts on two caller streams, each behind its own gate and
    with its own input (one takes the other's poison), enqueued one call of each in turn"""
    torch = gate.torch
    W, both, whole = 10, True, False
    gates = [gate, gate.on(torch.cuda.Stream(device=gate.dev))]
    ctxs = [pk.Context(0), pk.Context(0)]
    try:
        chains, bufs, cases = [], [], []
        for k in range(2):
            ctxs[k].set_stream(gates[k].s)
            ch = sg.Chain(gates[k])
            b, case = sg.chain_a_buffers(ch, W, both, whole, swap=bool(k))
            chains.append(ch), bufs.append(b), cases.append(case)
        steps = lambda k: sg.chain_a_steps(ctxs[k], chains[k], bufs[k], cases[k], W, both, whole)
        for _ in range(2):
            for ch in chains:
                ch.arm(None)
            sg.interleave(steps(0), steps(1))
            for k in range(2):
                sg.check_chain_a(chains[k].finish(), cases[k]["want"])
        for ch in chains:
            ch.arm(150.0)
        sg.interleave(steps(0), steps(1))
        assert chains[0].pending() and chains[1].pending()
        got = [ch.finish() for ch in chains]
        for k in range(2):
            sg.check_chain_a(got[k], cases[k]["want"])
        assert not np.array_equal(got[0]["counts"], got[1]["counts"])
    finally:
        for c in ctxs:
            c.close()
