"""The ends of the count of csrc/count.hip: the last chunk of an item (scan_items' wave-uniform tail body beside the full
and the predicated ones) and the launch sequence of the one-level partition at W = 8 and 10 (one clear; bucket-major
table fed by pass B, by overflowed slices and by the fix-up; counters kept beside it).  Everything is integer and
compared bit for bit with the oracle: the table (mirrored under both strands), ltot, the 84 fused counters, and the
number of deferred items with the model of tests/count_edges_model.py.  Tables are counted into fresh, uncleared device
buffers, so a bin the count does not write shows.

Tail inputs: per W one input of groups of 200 sequences of one length L = W - 1 + 16 k + r (k = 0, 1, 2; r = 1 .. 16:
r windows in the last chunk, r = 16 a full one, k = 0 and r = 1 a one-window run), each followed by 56 filler sequences
of another length: every group is three whole waves of equally long items and a fourth that is not.  At these lengths
no run is longer than an item at either packing; groups of 64 + r windows follow, which the 64-window packing cuts in
two (head and tail items then alternate in a wave, which is ragged).  The ragged variant makes one sequence of every
64 one base longer: no wave of it is uniform."""
import functools

import numpy as np
import pytest

import count_edges_model as cm
import peng_motif_amd as pk
from oracle import oracle as po

pytestmark = pytest.mark.gpu

GROUP, FILLER = 200, 56


@pytest.fixture(scope="module")
def ctx():
    c = pk.Context(0)
    yield c
    c.set_option("count_impl", 0)
    c.set_option("key_cap_override", 0)
    c.close()


def emitters(W):
    return (1, 2) if W >= 8 else (1,)


def tail_sequence(rng, W, L, i):
    """sequence i of a group: random with a planted poly-A; a repeat of period 1 .. W through the last 2W bases (windows
    are suppressed inside the last chunk, and the last base's 3-mer is a repeat's); a reverse-complement palindrome of W
    bases at the end (the last window is its own reverse complement)"""
    s = cm.rand(rng, L)
    kind = i % (W + 2)
    if kind == 0:
        n = min(L, W + 3)
        a = int(rng.integers(0, L - n + 1))
        s[a:a + n] = 1
    elif kind <= W:
        n = min(L, 2 * W)
        s[L - n:] = cm.tile(cm.rand(rng, kind), n)
    else:
        h = cm.rand(rng, W // 2)
        s[L - W:] = np.concatenate([h, cm.revcomp_codes(h)])
    return s


@functools.lru_cache(None)
def tail_input(W, ragged):
    rng = np.random.default_rng(7000 + W)
    seqs = []
    for k in (0, 1, 2):
        for r in range(1, 17):
            L = W - 1 + 16 * k + r
            seqs += [tail_sequence(rng, W, L, i) for i in range(GROUP)]
            seqs += [cm.rand(rng, W + 5) for _ in range(FILLER)]
    assert len(seqs) % 64 == 0
    for r in (1, 8, 15, 16):
        seqs += [tail_sequence(rng, W, W - 1 + 64 + r, i) for i in range(GROUP)]
    if ragged:
        for w in range(0, len(seqs), 64):
            j = w + (7 * (w // 64)) % min(64, len(seqs) - w)
            seqs[j] = np.concatenate([seqs[j], cm.rand(rng, 1)])
    return cm.join(seqs)


class Reference:
    """the oracle's answers for one input, computed once"""

    def __init__(self, codes, offs, W):
        self.codes, self.offs, self.W = codes, offs, W
        self.bg = po.bg_counts(codes, offs, 2)

    @functools.lru_cache(None)
    def count(self, both):
        want, ltot = po.count(self.codes, self.offs, self.W, both)
        assert int(want.max()) < 2 ** 32
        return want.astype(np.uint32), ltot


def check(ctx, ref, p, both, impl, what, with_bg=True, deferred_want=None):
    """count what is attached into an uncleared table and compare everything with the reference"""
    want, ltot = ref.count(both)
    ctx.set_option("count_impl", impl)
    try:
        counts = ctx.empty(4 ** p.W, np.uint32)
        if with_bg:
            assert p.all_whole == 1, what
            counts, lt, bg = ctx.count_bg(both, counts=counts)
        else:
            counts, lt = ctx.count(both, counts=counts)
        deferred = ctx.info("deferred_items")
        if both:
            ctx.mirror(p.W, counts)
        got = counts.to_host()
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError("%s: %d bins differ, the first: bin %d, device %d, oracle %d"
                                 % (what, bad.size, bad[0], got[bad[0]], want[bad[0]]))
        assert int(lt.to_host()[0]) == ltot == p.n_windows, what
        if with_bg:
            assert np.array_equal(bg.to_host().astype(np.int64), ref.bg), "%s: fused background counters" % what
        if deferred_want is None:
            deferred_want = int(cm.deferral_model(p.words, p.items, p.W, both).sum())
        assert deferred == deferred_want, "%s: %d items deferred, the model says %d" % (what, deferred, deferred_want)
    finally:
        ctx.set_option("count_impl", 0)


def name(both, impl):
    return "%s, %s emitter" % ("both strands" if both else "plus strand", {0: "default", 1: "direct", 2: "partitioned"}[impl])


@pytest.mark.parametrize("ragged", (False, True), ids=("equal", "ragged"))
@pytest.mark.parametrize("W", (8, 10, 12))
def test_tails(ctx, W, ragged):
    """every number of windows in the last chunk, in waves of equally long items (the tail body; the full body alone at
    r = 16) and, ragged, in waves where one item is a base longer (the predicated body)"""
    codes, offs = tail_input(W, ragged)
    ref = Reference(codes, offs, W)
    for M in (0, 64):
        p = pk.Packed(codes, offs, W, M)
        cont = cm.item_fields(p.items)[2]
        assert (cont.sum() > 0) == (M == 64)
        deferred = {both: int(cm.deferral_model(p.words, p.items, W, both).sum()) for both in (False, True)}
        ctx.upload(p)
        for both in (False, True):
            for impl in emitters(W):
                check(ctx, ref, p, both, impl, "tails, W = %d, %s, items of %d windows, %s"
                      % (W, "ragged" if ragged else "equal", p.item_windows, name(both, impl)), deferred_want=deferred[both])


def synth_packed(seed, n, L, W):
    codes, offs = po.synth(seed, 0, n, L)
    return Reference(codes, offs, W), pk.Packed(codes, offs, W)


def test_launch_sequence_on_one_context(ctx):
    """W = 10, 8, 10 again with inputs of different sizes on one context (scratch left by one call must not reach the
    next), then the same with 64-entry key slices, where most keys overflow into the bucket-major table; with and
    without the background counters"""
    cases = [synth_packed(11, 3000, 150, 10), synth_packed(12, 700, 90, 8), synth_packed(13, 1500, 211, 10)]
    for cap in (0, 64):
        ctx.set_option("key_cap_override", cap)
        try:
            for ref, p in cases:
                ctx.upload(p)
                for with_bg in (True, False):
                    for both in (True, False):
                        check(ctx, ref, p, both, 0, "launch sequence, W = %d, %d items, slices of %s keys, %s, %s"
                              % (p.W, len(p.items), cap or "default", "count_bg" if with_bg else "count", name(both, 0)),
                              with_bg=with_bg, deferred_want=0)
        finally:
            ctx.set_option("key_cap_override", 0)


@pytest.mark.parametrize("W", (8, 10))
def test_deferred_items_under_the_partitioned_emitter(ctx, W):
    """the model's repeats of every period (dozens of deferred items) and its 20 000-base repeats (every item behind the
    first deferred, each fix-up walking back to the head): the fix-up adds into the bucket-major table, alone and
    beside overflowed slices; the model's number of deferred items is reported"""
    for cls in ("periods", "long_fixup"):
        (part,), (p,) = cm.CLASSES[cls](W), cm.packed(cls, W)
        ref = Reference(part["codes"], part["offs"], W)
        ctx.upload(p)
        for cap in (0, 64):
            ctx.set_option("key_cap_override", cap)
            try:
                for both in (False, True):
                    want = int(cm.deferral_model(p.words, p.items, W, both).sum())
                    assert want > 0
                    for with_bg in (True, False):
                        check(ctx, ref, p, both, 2, "%s, W = %d, slices of %s keys, %s, %s"
                              % (cls, W, cap or "default", "count_bg" if with_bg else "count", name(both, 2)),
                              with_bg=with_bg and p.all_whole == 1, deferred_want=want)
            finally:
                ctx.set_option("key_cap_override", 0)
