"""The stream gate: a deterministic way to make mis-ordered device work visible at tiny shapes, and the inputs and
expected values of the three chains that tests/test_gpu_stream_order.py runs behind it (tests/test_stream_order_cpu.py
certifies the inputs on the CPU).

include/pengk.h promises: work is enqueued on the context's stream, functions that take only d_ pointers do not
synchronise with the host, pengk_set_stream re-targets a context to a caller-owned stream.  A test that uploads with a
synchronous copy, calls, and downloads with a synchronous copy cannot see a breach of any of it.  Here

  buffers      every device buffer of a test is a torch tensor (flat uint8: only its data_ptr() crosses the ABI) used on
               ONE torch.cuda.Stream s, and the context is re-targeted to s.  An input buffer first holds POISON: another
               valid input of the same sizes, so nothing can fault; an output buffer holds 0xA5 bytes.
  gate         torch.cuda._sleep(cycles) on s: bounded device work, never a kernel that waits for the host.
  production   behind the gate, device-to-device copies on s overwrite the poison with the real input and the outputs
               with 0xA5 bytes again (zero bytes where the library ADDS to a caller-zeroed array): what ran early is
               overwritten.
  calls        the library calls, with no host wait of the test's own.
  consumption  directly behind the call that wrote it, every output is copied on s into a tensor of its own
               (Chain.take); then ONE s.synchronize(), then the comparison.

Whatever the library issues on another stream runs while the gate is still busy: it reads poison, or its output is
overwritten by the production, and the bits differ.  positive_control() shows that the set-up can see exactly that.
"""
import copy
import functools
import time

import numpy as np

import peng_motif_amd as pk
import motif_centrality_model as mc
import motif_dust_model as md
import motif_dyads_model as dy
import motif_erase_model as me
import motif_match_model as mm
import motif_score_model as ms
import motif_shuffle_model as msh
import motif_sites_model as mst
from oracle import oracle as po

GATE_MIN_MS = 50.0      # the gate runs for at least this long ...
GATE_ENQUEUE_FACTOR = 20.0  # ... and for at least this many times the host time to enqueue the chain behind it,
GATE_MAX_MS = 400.0     # but never longer: every test stays within seconds
JUNK = 0xA5


# ---- the gate --------------------------------------------------------------------------------------------------------
class Gate:
    """A torch stream and the number of torch.cuda._sleep cycles per millisecond on this device (measured once)."""

    def __init__(self, device=0):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", device)
        self.s = torch.cuda.Stream(device=self.dev)
        self.cycles_per_ms = self._calibrate()

    def _calibrate(self):
        cycles = 1_000_000
        for _ in range(6):
            ms_ = self.sleep_ms(cycles)
            if ms_ >= 5.0:
                return cycles / ms_
            cycles *= 10
        raise AssertionError("torch.cuda._sleep(%d) took %.3f ms: no usable gate on this device" % (cycles // 10, ms_))

    def sleep_ms(self, cycles):
        """the device time of one _sleep(cycles) on s, by torch events (waits)"""
        torch = self.torch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.s):
            torch.cuda._sleep(1000)  # (the first launch of the spin kernel: its code object)
            a.record(self.s)
            torch.cuda._sleep(int(cycles))
            b.record(self.s)
        self.s.synchronize()
        return a.elapsed_time(b)

    def cycles(self, gate_ms):
        return int(gate_ms * self.cycles_per_ms)

    def on(self, stream):
        """the same gate on another stream of the device"""
        g = copy.copy(self)
        g.s = stream
        return g

    @staticmethod
    def length_ms(enqueue_ms):
        """the gate for a chain that takes enqueue_ms of host time to enqueue"""
        return min(max(GATE_MIN_MS, GATE_ENQUEUE_FACTOR * enqueue_ms), GATE_MAX_MS)

    def device_bytes(self, a):
        """a device copy of a numpy array as a flat uint8 tensor (complete on return)"""
        torch = self.torch
        a = np.ascontiguousarray(a)
        t = torch.empty(max(a.nbytes, 1), dtype=torch.uint8, device=self.dev)
        if a.nbytes:
            t[:a.nbytes].copy_(torch.from_numpy(a.reshape(-1).view(np.uint8).copy()))
        torch.cuda.synchronize(self.dev)
        return t


class Chain:
    """The device buffers of one chain of calls on gate.s: inputs with their poison, outputs with their consumer copies."""

    def __init__(self, gate):
        self.g = gate
        self.inputs = {}   # name -> (buf, real, poison)
        self.outputs = {}  # name -> (buf, fill behind the gate, junk, result, shape, dtype)
        self.taken = []
        self.gate_events = None

    def inp(self, name, real, poison):
        real, poison = np.ascontiguousarray(real), np.ascontiguousarray(poison)
        assert real.shape == poison.shape and real.dtype == poison.dtype, name
        buf = self.g.device_bytes(poison)
        self.inputs[name] = (buf, self.g.device_bytes(real), self.g.device_bytes(poison))
        return buf

    def out(self, name, shape, dtype, added_to=False):
        shape = tuple(np.atleast_1d(shape).tolist())
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        junk = self.g.device_bytes(np.full(n, JUNK, np.uint8))
        fill = self.g.device_bytes(np.zeros(n, np.uint8)) if added_to else junk
        self.outputs[name] = (self.g.device_bytes(np.full(n, JUNK, np.uint8)), fill, junk,
                              self.g.device_bytes(np.full(n, JUNK, np.uint8)), shape, np.dtype(dtype))
        return self.outputs[name][0]

    def arm(self, gate_ms=None, before_gate=None):
        """poison and 0xA5 bytes into the buffers (waited for), then on s: the gate (gate_ms = None: none) and the
        production.  before_gate: called when s is idle and the gate comes next."""
        torch, s = self.g.torch, self.g.s
        with torch.cuda.stream(s):
            for buf, _, poison in self.inputs.values():
                buf.copy_(poison)
            for buf, _, junk, res, _, _ in self.outputs.values():
                buf.copy_(junk)
                res.copy_(junk)
        s.synchronize()
        self.taken = []
        if before_gate is not None:
            before_gate()
        with torch.cuda.stream(s):
            if gate_ms is not None:
                self.gate_events = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                self.gate_events[0].record(s)
                torch.cuda._sleep(self.g.cycles(gate_ms))
                self.gate_events[1].record(s)
            for buf, real, _ in self.inputs.values():
                buf.copy_(real)
            for buf, fill, _, _, _, _ in self.outputs.values():
                buf.copy_(fill)

    def take(self, *names):
        """the consumer copies of these outputs, on s"""
        torch = self.g.torch
        with torch.cuda.stream(self.g.s):
            for name in names:
                buf, _, _, res, _, _ = self.outputs[name]
                res.copy_(buf)
                self.taken.append(name)

    def pending(self):
        return not self.g.s.query()

    def finish(self):
        """the one host wait; -> {name: numpy array} of the outputs taken"""
        self.g.s.synchronize()
        got = {}
        for name in self.taken:
            _, _, _, res, shape, dtype = self.outputs[name]
            n = int(np.prod(shape)) * dtype.itemsize
            got[name] = res[:n].cpu().numpy().view(dtype).reshape(shape).copy()
        return got

    def gate_ms(self):
        """the gate's device time on the last gated run (after finish)"""
        return self.gate_events[0].elapsed_time(self.gate_events[1])


def run(steps):
    """enqueue a chain (a generator that yields after every library call); -> host milliseconds it took"""
    t0 = time.perf_counter()
    for _ in steps:
        pass
    return (time.perf_counter() - t0) * 1e3


def interleave(*chains):
    """enqueue several chains, one call of each in turn"""
    live = list(chains)
    while live:
        for c in list(live):
            try:
                next(c)
            except StopIteration:
                live.remove(c)


def positive_control(gate, n_bytes=1 << 20, gate_ms=GATE_MIN_MS, tries=4):
    """The consumer copy of a gated buffer, issued on a stream OTHER than gate.s, must read the poison (and the same copy
    on gate.s the real bytes).  Several streams can share one of the process's hardware queues -- a copy on such a stream
    queues up behind the gate like one on s -- so up to `tries` fresh streams are tried.  -> (tries needed, what the
    copy on s read == real); raises when no stream saw the poison: inconclusive is a failure."""
    torch, s = gate.torch, gate.s
    rng = np.random.default_rng(1)
    real, poison = rng.integers(0, 256, n_bytes, dtype=np.uint8), rng.integers(0, 256, n_bytes, dtype=np.uint8)
    d_real, d_poison = gate.device_bytes(real), gate.device_bytes(poison)
    buf, seen_other, seen_s = gate.device_bytes(poison), gate.device_bytes(real), gate.device_bytes(poison)
    for k in range(tries):
        other = torch.cuda.Stream(device=gate.dev)
        with torch.cuda.stream(s):
            buf.copy_(d_poison)
            seen_other.copy_(d_real)
            seen_s.copy_(d_poison)
        torch.cuda.synchronize(gate.dev)
        with torch.cuda.stream(s):
            torch.cuda._sleep(gate.cycles(gate_ms))
            buf.copy_(d_real)
        with torch.cuda.stream(other):
            seen_other.copy_(buf)
        with torch.cuda.stream(s):
            seen_s.copy_(buf)
        pending = not s.query()
        torch.cuda.synchronize(gate.dev)
        on_s_real = bool(torch.equal(seen_s, d_real))
        if pending and bool(torch.equal(seen_other, d_poison)):
            return k + 1, on_s_real
    raise AssertionError("positive control inconclusive: on none of %d fresh streams did a copy overtake the gate" % tries)


# ---- chain (a): the count path ------------------------------------------------------------------------------------------
A_N_SEQ, A_LEN, A_K = 2000, 100, 2
A_CONFIGS = [(8, True), (10, True), (10, False)]  # (W, both strands)
A_N_PWM, A_ITERATIONS, A_SATURATION = 16, 3, 1e4
# (sequence, position) of the invalid bases of the inputs that have some -- the same in the real input and in its poison,
# so that both pack to the same words, items and bounds: in the middle, at both ends, two in a row, and one that leaves a
# run shorter than every W behind it
A_INVALID = [(3, 40), (3, 41), (500, 0), (777, 99), (1000, 8), (1200, 50), (1999, 95)]
A_WORDS = {False: "GCTGAGTCAT", True: "TTACGCAATC"}  # planted in every fifth sequence: real, poison


def count_codes(poison, whole):
    """byte codes and offsets of the count input (whole: without invalid bases) or of its poison"""
    rng = np.random.default_rng(4100 + int(poison))
    p = (0.35, 0.15, 0.2, 0.3) if poison else (0.2, 0.3, 0.3, 0.2)
    codes = (rng.choice(4, (A_N_SEQ, A_LEN), p=p) + 1).astype(np.uint8)
    word = np.array(["ACGT".index(c) + 1 for c in A_WORDS[bool(poison)]], np.uint8)
    for i in range(0, A_N_SEQ, 5):
        at = int(rng.integers(0, A_LEN - len(word) + 1))
        codes[i, at:at + len(word)] = word
    if not whole:
        for i, q in A_INVALID:
            codes[i, q] = 0
    return codes.reshape(-1), np.arange(A_N_SEQ + 1, dtype=np.int64) * A_LEN


def seed_pwms(counts, W, rng):
    """A_N_PWM start PWMs: the highest-count k-mers (ties by ascending id) as 0.7 / 0.1 rows, the last four random"""
    order = np.lexsort((np.arange(counts.size), -counts.astype(np.int64)))[:A_N_PWM]
    pw = np.full((A_N_PWM, W, 4), 0.1, np.float32)
    for i, x in enumerate(order):
        for q in range(W):
            pw[i, q, (int(x) >> (2 * q)) & 3] = 0.7
    pw[-4:] = rng.dirichlet(np.ones(4), size=(4, W)).astype(np.float32)
    return pw


@functools.lru_cache(maxsize=None)
def chain_a_case(W, both, whole, poison):
    """the packed input of chain (a), its start PWMs and every expected output, from the oracle"""
    codes, offs = count_codes(poison, whole)
    p = pk.Packed(codes, offs, W)
    counts, ltot = po.count(codes, offs, W, both)
    bgc = po.bg_counts(codes, offs, 2)
    V = po.bg_V(bgc, 2)
    bgp = np.stack([po.bgprob(W, k, V, both) for k in range(A_K + 1)])
    e, lp, z = po.stats(W, counts, bgp[A_K], ltot)
    pw0 = seed_pwms(counts, W, np.random.default_rng(4200 + int(poison)))
    em = [po.em(W, counts, bgp[A_K], pw0[i], A_SATURATION, 0.0, A_ITERATIONS, mode=0, final_norm=False) for i in range(A_N_PWM)]
    want = dict(counts=counts.astype(np.uint32), ltot=np.array([ltot], np.uint64), bgc=bgc.astype(np.uint64),
                V=V, bgprob=bgp, expected=e, logp=lp, z=z,
                pwms=np.stack([r[0] for r in em]).astype(np.float32),
                state=np.array([[r[1], 0] for r in em], np.int32), change=np.array([r[2] for r in em], np.float32))
    assert all(r[1] == A_ITERATIONS for r in em)
    return dict(packed=p, pwms=pw0, want=want)


def chain_a_buffers(ch, W, both, whole, swap=False):
    """the buffers of chain (a) on a Chain; swap: the poison as the real input and the other way round"""
    real, poison = chain_a_case(W, both, whole, swap), chain_a_case(W, both, whole, not swap)
    pr, pp = real["packed"], poison["packed"]
    assert (len(pr.words), len(pr.items), pr.max_bin_bound, pr.all_whole, pr.n_windows) == \
           (len(pp.words), len(pp.items), pp.max_bin_bound, pp.all_whole, pp.n_windows) and pr.all_whole == int(whole)
    NP = 4 ** W
    b = dict(words=ch.inp("words", pr.words, pp.words), items=ch.inp("items", pr.items, pp.items),
             pwms_in=ch.inp("pwms_in", real["pwms"], poison["pwms"]))
    if whole:  # pengk_count_bg counts the background on the device; else the packer's counters are an input
        b["bgc"] = ch.out("bgc", 84, np.uint64)
    else:
        b["bgc"] = ch.inp("bgc_in", real["want"]["bgc"], poison["want"]["bgc"])
    for name, shape, dtype in (("counts", NP, np.uint32), ("ltot", 1, np.uint64), ("V", 84, np.float32),
                               ("bgprob", (A_K + 1, NP), np.float32), ("expected", NP, np.float32), ("logp", NP, np.float32),
                               ("z", NP, np.float32), ("pwms", (A_N_PWM, W, 4), np.float32), ("state", (A_N_PWM, 2), np.int32),
                               ("change", A_N_PWM, np.float32)):
        b[name] = ch.out(name, shape, dtype)
    return b, real


def chain_a_steps(ctx, ch, b, case, W, both, whole, em=True):
    """set_sequences, count (count_bg on a whole input), mirror, bg_model, pattern_stats, em_device: d_ pointers only"""
    p = case["packed"]
    ctx.set_sequences(b["words"], b["items"], len(p.words), len(p.items), W, p.item_windows, p.max_bin_bound, p.all_whole)
    ctx.set_option("n_windows_hint", p.n_windows)
    yield
    if whole:
        ctx.count_bg(both, b["counts"], b["ltot"], b["bgc"])
        ch.take("bgc")
    else:
        ctx.count(both, b["counts"], b["ltot"])
    ch.take("ltot")
    yield
    if both:
        ctx.mirror(W, b["counts"])
        yield
    ch.take("counts")
    ctx.bg_model(b["bgc"], 2, out=b["V"])
    ch.take("V")
    yield
    ctx.pattern_stats(W, both, A_K, A_K, b["V"], b["ltot"], b["counts"], b["bgprob"], b["expected"], b["logp"], b["z"])
    ch.take("bgprob", "expected", "logp", "z")
    yield
    if em:
        # (the start PWMs go into the in/out buffer on the stream, like any producer of a pipeline would write them)
        with ch.g.torch.cuda.stream(ch.g.s):
            b["pwms"].copy_(b["pwms_in"])
        ctx.em_device(W, A_N_PWM, b["pwms"], b["counts"], b["bgprob"][A_K * 4 ** W * 4:], b["state"], b["change"],
                      A_SATURATION, 0.0, A_ITERATIONS)
        ch.take("pwms", "state", "change")  # directly behind em_device: a lane that is not joined shows as stale PWMs
        yield


def ulp_diff(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    d = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
    d[same] = 0
    return int(d.max()) if d.size else 0


def check_chain_a(got, want):
    """as tests/test_gpu_parity.py: integer tables and float tables bit for bit, log-p within one float32 ulp (device
    log against glibc's); the EM's PWMs, iteration counts and `change` bit for bit"""
    for name, g in got.items():
        w = want[name]
        assert g.shape == w.shape and g.dtype == w.dtype, name
        if name == "logp":
            assert ulp_diff(g, w) <= 1, name
        else:
            bad = np.flatnonzero(g.reshape(-1).view(np.uint8) != w.reshape(-1).view(np.uint8))
            assert len(bad) == 0, "%s: %d bytes differ, the first at %d" % (name, len(bad), bad[0])


def em_lanes(n_pwm, em_overlap, max_lanes=4):
    """the streams the serial EM's batches take turns on at W >= 10 (launch_serial_ahead, csrc/em.hip)"""
    lanes = min(max(em_overlap, 1), max_lanes)
    while lanes > 1 and n_pwm < 8 * lanes:
        lanes -= 1
    return lanes


# ---- chains (b) and (c): the scan layout -----------------------------------------------------------------------------------
B_LENGTHS = [0, 1, 2, 31, 32, 33, 64, 65, 256, 257, 300]
B_N_SEQ = 300
B_DUST_T, B_MAX_GAP, B_SHUFFLE_SEED, B_SEQ0 = 20, 20, 0x5EED5EED5EED, 1000
B_SYNTH = dict(seed=11, seq0=12345, n=257, L=70)  # what pengk_synth_scan_sequences writes into the fifth buffer


def scan_seqs(poison):
    """B_N_SEQ sequences of 0 .. 300 bases with skewed compositions (low-complexity stretches) and invalid bases; the
    poison has the same lengths, hence the same layout"""
    lens = B_LENGTHS + np.random.default_rng(4300).integers(0, 301, B_N_SEQ - len(B_LENGTHS)).tolist()
    rng = np.random.default_rng(4301 + int(poison))
    out = []
    for k, L in enumerate(lens):
        w = rng.dirichlet(np.full(4, (0.15, 0.4, 1.0)[k % 3]))
        c = (rng.choice(4, L, p=w) + 1).astype(np.uint8)
        if k % 2 and L:
            c[rng.integers(0, L, 1 + k % 3)] = 0
        out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def scan_layout(poison):
    seqs = scan_seqs(poison)
    return seqs, pk.ScanLayout(*ms.flatten(seqs))


def _valid_of(lay, seqs):
    v = np.zeros(len(lay.valid), np.uint32)
    w = me.valid_words(seqs)
    v[:len(w)] = w
    return v


def strata_of_words(stored, valid_of, G=10):
    """pengk_seq_strata on words that keep the letters of `stored` under the validity of `valid_of` (the same sequences
    with more bases invalid): include/pengk.h counts n over the validity bits and gc over the STORED letters -- "every other
    letter is stored as A ..., so no validity word is read for it" -- which is tests/motif_match_model.py's stratum where
    the two agree, as in every layout the host builds.  -> (stratum per sequence, the 256 counts)"""
    s = np.full(len(stored), mm.NONE, np.uint16)
    for i, (c, v) in enumerate(zip(stored, valid_of)):
        n = int(((np.asarray(v) >= 1) & (np.asarray(v) <= 4)).sum())
        if n:
            gc = int(((np.asarray(c) == 2) | (np.asarray(c) == 3)).sum())
            s[i] = mm.length_bin(len(c)) * G + min(G - 1, (gc * G) // n)
    return s, mm.histogram(s)


@functools.lru_cache(maxsize=None)
def chain_b_want(poison):
    """mask_low_complexity, then dyad_count, seq_strata and shuffle_sequences on the masked validity, and the synthetic set"""
    seqs, lay = scan_layout(poison)
    masked, bits, touched = md.mask_codes(seqs, B_DUST_T)
    mv = _valid_of(lay, masked)
    dc, dm = dy.tables(masked, B_MAX_GAP, True)
    st, sh = strata_of_words(seqs, masked)  # (the words keep the masked letters: only the validity is the mask's)
    sw, sv = msh.shuffle_layout(lay.words, mv, lay.offs, lay.lens, lay.n_seq, B_SHUFFLE_SEED, B_SEQ0)
    out_w, out_v = np.zeros(len(lay.words), np.uint64), np.zeros(len(lay.valid), np.uint32)
    out_w[:len(sw)], out_v[:len(sv)] = sw, sv
    syn = pk.ScanLayout(*po.synth(B_SYNTH["seed"], B_SYNTH["seq0"], B_SYNTH["n"], B_SYNTH["L"]))
    return dict(masked_valid=mv, masked=np.array([bits, touched], np.uint64), dyads=dc.astype(np.uint64), mono=dm.astype(np.uint64),
                stratum=st.astype(np.uint16), strata=sh.astype(np.uint64), shuffled_words=out_w, shuffled_valid=out_v,
                synth_words=syn.words, synth_valid=syn.valid, synth_offs=syn.offs, synth_lens=syn.lens)


def scan_buffers(ch, swap=False):
    """the scan layout of chains (b) and (c) as input buffers: (words, valid, offs, lens, n_seq)"""
    (_, real), (_, poison) = scan_layout(swap), scan_layout(not swap)
    assert np.array_equal(real.offs, poison.offs) and np.array_equal(real.lens, poison.lens)
    return (ch.inp("words", real.words, poison.words), ch.inp("valid", real.valid, poison.valid),
            ch.inp("offs", real.offs, poison.offs), ch.inp("lens", real.lens, poison.lens), real.n_seq)


def chain_b_buffers(ch, swap=False):
    scan = scan_buffers(ch, swap)
    want = chain_b_want(swap)
    b = dict(scan=scan)
    for name, w in want.items():
        b[name] = ch.out(name, w.shape, w.dtype, added_to=name in ("masked", "dyads", "mono", "strata"))
    return b, want


def chain_b_steps(ctx, ch, b):
    words, valid, offs, lens, n = b["scan"]
    ctx.mask_low_complexity(b["scan"], B_DUST_T, out_valid=b["masked_valid"], masked=b["masked"])
    ch.take("masked_valid", "masked")
    yield
    masked = (words, b["masked_valid"], offs, lens, n)
    ctx.dyad_count(masked, B_MAX_GAP, True, counts=b["dyads"], mono=b["mono"])
    ch.take("dyads", "mono")
    yield
    ctx.seq_strata(masked, stratum=b["stratum"], hist=b["strata"])
    ch.take("stratum", "strata")
    yield
    ctx.shuffle_sequences(masked, B_SHUFFLE_SEED, B_SEQ0, words=b["shuffled_words"], valid=b["shuffled_valid"])
    ch.take("shuffled_words", "shuffled_valid")
    yield
    pk._check(pk.lib().pengk_synth_scan_sequences(ctx.h, B_SYNTH["seed"], B_SYNTH["seq0"], B_SYNTH["n"], B_SYNTH["L"],
                                                  b["synth_words"].data_ptr(), b["synth_valid"].data_ptr(),
                                                  b["synth_offs"].data_ptr(), b["synth_lens"].data_ptr()))
    ch.take("synth_words", "synth_valid", "synth_offs", "synth_lens")
    yield


def check_bits(got, want):
    for name, g in got.items():
        w = want[name]
        assert g.shape == w.shape and g.dtype == w.dtype, name
        bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
        assert len(bad) == 0, "%s: %d of %d entries differ, the first at %d: %r, the model %r" % (
            name, len(bad), g.size, bad[0], g.reshape(-1)[bad[0]], w.reshape(-1)[bad[0]])


# chain (c): six calls that stage host parameters, each with motifs and thresholds of its own
C_WIDTHS = dict(scan=[6, 10, 33], sites=[8, 5], erase=[7, 12], best=[4, 11, 16])
C_SEQ0 = 77


def _random_S(rng, w):
    S = rng.integers(-300, 301, (w, 4)).astype(np.int32)
    S[rng.random((w, 4)) < 0.05] = -2000
    S[rng.random((w, 4)) < 0.02] = 2000
    return S


@functools.lru_cache(maxsize=None)
def chain_c_motifs():
    """the four motif sets and their thresholds (fixed on the real input: a call's host parameters are no device input)"""
    rng = np.random.default_rng(4400)
    S = {k: [_random_S(rng, w) for w in ws] for k, ws in C_WIDTHS.items()}
    seqs, _ = scan_layout(False)
    thr = {}
    for k, q in (("sites", 70), ("erase", 90), ("best", 40)):
        thr[k] = []
        for s in S[k]:
            b = ms.best_scores(seqs, s, True)
            thr[k].append(int(np.percentile(b[b > ms.SENTINEL], q)))
    return S, thr


@functools.lru_cache(maxsize=None)
def chain_c_want(poison):
    seqs, lay = scan_layout(poison)
    S, thr = chain_c_motifs()
    n = len(seqs)
    lens = np.array([len(c) for c in seqs])
    max_len = int(lens.max())
    best = np.stack([ms.best_scores(seqs, s, True) for s in S["scan"]]).astype(np.int32)
    rng_ = [ms.score_range(s) for s in S["scan"]]
    hist = np.concatenate([ms.histogram(best[m], lo, hi) for m, (lo, hi) in enumerate(rng_)]).astype(np.uint64)
    counts = np.zeros((len(S["sites"]), n), np.uint64)
    for m, (s, t) in enumerate(zip(S["sites"], thr["sites"])):
        for i, _, _, _ in mst.sites(seqs, s, t, True):
            counts[m, i] += 1
    erased_seqs, n_sites, erased = me.mask(seqs, S["erase"], thr["erase"], True)
    bs = [mc.best_sites(seqs, s, True, m, C_SEQ0) for m, s in enumerate(S["best"])]
    bb, site = np.stack([x for x, _ in bs]).astype(np.int32), np.stack([x for _, x in bs]).astype(np.uint64)
    hd, hl = zip(*[mc.histograms(bb[m], site[m], lens, w, thr["best"][m], max_len) for m, w in enumerate(C_WIDTHS["best"])])
    return dict(best=best, hist=hist, site_counts=counts, erased_valid=_valid_of(lay, erased_seqs),
                erase_sites=np.asarray(n_sites, np.uint64), erased=np.array([erased], np.uint64), best_score=bb, best_site=site,
                central_offsets=np.stack(hd).astype(np.uint64), central_lengths=np.stack(hl).astype(np.uint64))


def chain_c_buffers(ch, swap=False):
    scan = scan_buffers(ch, swap)
    want = chain_c_want(swap)
    b = dict(scan=scan)
    for name, w in want.items():
        b[name] = ch.out(name, w.shape, w.dtype,
                         added_to=name in ("hist", "erase_sites", "erased", "central_offsets", "central_lengths"))
    return b, want


def chain_c_steps(ctx, ch, b):
    S, thr = chain_c_motifs()
    scan = b["scan"]
    n = scan[4]
    max_len = max(len(c) for c in scan_layout(False)[0])
    ctx.motif_scan(scan, S["scan"], C_WIDTHS["scan"], True, best=b["best"])
    ch.take("best")
    yield
    lo, hi = zip(*[ms.score_range(s) for s in S["scan"]])
    ctx.score_histograms(b["best"], n, lo, hi, hist=b["hist"])
    ch.take("hist")
    yield
    ctx.sites_count(scan, S["sites"], C_WIDTHS["sites"], True, thr["sites"], counts=b["site_counts"])
    ch.take("site_counts")
    yield
    ctx.mask_sites(scan, S["erase"], C_WIDTHS["erase"], True, thr["erase"], out_valid=b["erased_valid"], sites=b["erase_sites"],
                   erased=b["erased"])
    ch.take("erased_valid", "erase_sites", "erased")
    yield
    ctx.motif_best_sites(scan, S["best"], C_WIDTHS["best"], True, seq0=C_SEQ0, best=b["best_score"], site=b["best_site"])
    ch.take("best_score", "best_site")
    yield
    ctx.centrality_histograms(b["best_score"], b["best_site"], scan[3], n, C_WIDTHS["best"], thr["best"], max_len,
                              hd=b["central_offsets"], hl=b["central_lengths"])
    ch.take("central_offsets", "central_lengths")
    yield
