"""The count kernels of csrc/count.hip -- scan_items under the direct and the partitioned emitters, count_fixup_kernel,
the fused and the stand-alone background counts -- on the constructed inputs of tests/count_edges_model.py: item
lengths up to the 16-bit window field, every stream alignment, repeats of every period around W, repeats that end on
either side of a prologue, fix-ups that walk back to the head of a long run, runs cut by invalid bases.  Everything is
integer and compared bit for bit: with the oracle at W <= 12, with the model's sparse reference at W = 14, and the
number of deferred items with the model's prediction.  tests/test_count_edges_cpu.py asserts that the inputs hold the
classes they are built for.  (Stream offsets above 2^32 bases need a large input: tests/test_gpu_fullsize.py.)

And directly against the COMPILED REFERENCE at W <= 12 (tests/golden/edges_count_w*.npz, written by
tests/golden/make_edge_golden.py from the reference's own count of the same sequences): the sha256 of the device's table,
the stored bins and ltot, for every emitter.  W = 14 stays oracle-only: the reference's size_t counter table alone is
2 GiB there.  These tests read tests/golden only, never the reference."""
import numpy as np
import pytest

import count_edges_model as cm
import edge_fixtures as ef
import peng_motif_amd as pk
from oracle import oracle as po

pytestmark = pytest.mark.gpu

CLS = list(cm.CLASSES)


@pytest.fixture(scope="module")
def ctx():
    c = pk.Context(0)
    yield c
    c.set_option("count_impl", 0)
    c.close()


class Tables14:
    """two 4^14 tables on the device and two pinned host buffers to fetch them into (1 GiB each), shared by the module's
    W = 14 tests: a fresh pageable copy per comparison would cost a second each"""

    def __init__(self, ctx):
        self.ctx, n = ctx, 4 ** 14
        self.dev = [ctx.empty(n, np.uint32) for _ in range(2)]
        self.ptr, self.host = [], []
        for _ in range(2):
            q = pk.C.c_void_p()
            pk._check(pk.lib().pengk_host_alloc(ctx.h, 4 * n, pk.C.byref(q)))
            self.ptr.append(q.value)
            self.host.append(np.ctypeslib.as_array((pk.C.c_uint32 * n).from_address(q.value)))

    def fetch(self, k):
        pk._check(pk.lib().pengk_memcpy_d2h(self.ctx.h, self.ptr[k], self.dev[k].ptr, self.dev[k].nbytes))
        return self.host[k]

    def close(self):
        self.host = []
        for q in self.ptr:
            pk.lib().pengk_host_free(self.ctx.h, q)


@pytest.fixture(scope="module")
def big(ctx):
    made = []

    def get():
        if not made:
            made.append(Tables14(ctx))
        return made[0]
    yield get
    for t in made:
        t.close()


def same(a, b):
    step = 1 << 24
    return all(np.array_equal(a[i:i + step], b[i:i + step]) for i in range(0, len(a), step))


def emitters(W):
    return (1, 2) if W >= 8 else (1,)


def mode(both, impl):
    return "%s, %s emitter" % ("both strands" if both else "plus strand", {0: "default", 1: "direct", 2: "partitioned"}[impl])


def run(ctx, both, impl, whole, counts=None):
    """count what is attached (count_bg where the input is whole) -> (counts on the device, mirrored under both strands,
    ltot, the 84 fused counters or None, deferred items)"""
    ctx.set_option("count_impl", impl)
    try:
        if whole:
            counts, lt, bg = ctx.count_bg(both, counts=counts)
            bg = bg.to_host().astype(np.int64)
        else:
            (counts, lt), bg = ctx.count(both, counts=counts), None
        deferred = ctx.info("deferred_items")
        if both:
            ctx.mirror(ctx.W, counts)
        return counts, int(lt.to_host()[0]), bg, deferred
    finally:
        ctx.set_option("count_impl", 0)


def first_difference(got, want):
    bad = np.flatnonzero(got != want)
    return "%d bins differ, the first: bin %d, device %d, reference %d" % (bad.size, bad[0], got[bad[0]], want[bad[0]])


_SEEN = {}  # (class, W): {(tag, emitter): (sha256 of the device's table, its stored bins, ltot, fused background counters)}


def _against_the_reference(cls, part, W, both, impl, got, lt, bg):
    """what the reference test needs of a device table, taken while the oracle test has it in hand"""
    fix = ef.load(ef.count_file(W))
    tag = ef.count_tag(cls, part, W, both)
    r = fix["index"].get(tag)
    idx = fix["slice_idx"][fix["slice_off"][r]:fix["slice_off"][r + 1]].astype(np.int64) if r is not None else np.zeros(0, np.int64)
    _SEEN.setdefault((cls, W), {})[tag, impl] = (ef.digest(got), got[idx], lt, bg)


def _count_class(ctx, cls, W):
    """every part of a class under both strand modes and every emitter, noted in _SEEN"""
    for part, p in zip(cm.CLASSES[cls](W), cm.packed(cls, W)):
        for both in (False, True):
            for impl in emitters(W):
                ctx.upload(p)
                counts, lt, bg, deferred = run(ctx, both, impl, p.all_whole)
                got = counts.to_host().astype(np.uint64)
                _against_the_reference(cls, part, W, both, impl, got, lt, bg)


@pytest.mark.parametrize("W", cm.WS)
@pytest.mark.parametrize("cls", CLS)
def test_classes_against_the_oracle(ctx, cls, W):
    """table (mirrored under both strands), ltot, the fused and the stand-alone background counters where the input is
    whole, and the number of deferred items, for every emitter that exists at W"""
    for part, p in zip(cm.CLASSES[cls](W), cm.packed(cls, W)):
        bg_want = po.bg_counts(part["codes"], part["offs"], 2)
        for both in (False, True):
            want, ltot = po.count(part["codes"], part["offs"], W, both)
            defer_want = int(cm.deferral_model(p.words, p.items, W, both).sum())
            for impl in emitters(W):
                what = "%s, W = %d, %s" % (part["name"], W, mode(both, impl))
                ctx.upload(p)
                counts, lt, bg, deferred = run(ctx, both, impl, p.all_whole)
                got = counts.to_host().astype(np.uint64)
                _against_the_reference(cls, part, W, both, impl, got, lt, bg)
                assert np.array_equal(got, want), "%s: %s" % (what, first_difference(got, want))
                assert lt == ltot, what
                assert deferred == defer_want, "%s: %d items deferred, the model says %d" % (what, deferred, defer_want)
                if p.all_whole:
                    assert np.array_equal(bg, bg_want), what
                    assert np.array_equal(ctx.bg_count().to_host().astype(np.int64), bg_want), what


@pytest.mark.parametrize("W", cm.WS)
@pytest.mark.parametrize("cls", CLS)
def test_classes_against_the_reference(ctx, cls, W):
    """The device's tables of test_classes_against_the_oracle (counted again only if that test did not run) against the
    compiled reference's fixture: inputs first (sha256 of codes and offsets: "inputs drifted" means regenerate), then the
    sha256 of the mirrored table, the stored bins (every count value the table holds, the largest bins, zero bins next
    to them; the whole table for W <= 6), ltot and the fused background counters -- for every emitter."""
    tags = [ef.count_tag(cls, part, W, both) for part in cm.CLASSES[cls](W) for both in (False, True)]
    if not all((t, impl) in _SEEN.get((cls, W), {}) for t in tags for impl in emitters(W)):
        _count_class(ctx, cls, W)
    fix = ef.load(ef.count_file(W))
    seen = _SEEN[cls, W]
    for part, p in zip(cm.CLASSES[cls](W), cm.packed(cls, W)):
        for both in (False, True):
            tag = ef.count_tag(cls, part, W, both)
            drift = ef.inputs_match(fix, tag, ef.count_inputs(part))
            assert drift is None, drift
            r = fix["index"][tag]
            a, e = fix["slice_off"][r], fix["slice_off"][r + 1]
            for impl in emitters(W):
                what = "%s, %s" % (tag, mode(both, impl))
                sha, bins, lt, bg = seen[tag, impl]
                bad = np.flatnonzero(bins != fix["slice_val"][a:e])
                assert not bad.size, "%s: bin %d: device %d, reference %d" % (what, fix["slice_idx"][a + bad[0]], bins[bad[0]], fix["slice_val"][a + bad[0]]) if bad.size else None
                assert np.array_equal(sha, fix["sha_counts"][r]), "%s: the table's sha256 is not the reference's (the stored bins agree)" % what
                assert lt == int(fix["ltot"][r]), what
                if bg is not None:
                    assert np.array_equal(bg, fix["bgcounts"][r]), what


def test_w14_against_the_sparse_reference(ctx, big):
    """all classes as one input at W = 14, packed at M = 64 and at M = 65535: the direct emitter's non-zero bins, their
    values and their sum against the sparse reference (canonical ids, nothing mirrored), and the partitioned emitter's
    table against the direct one's.  No dense 4^14 oracle table."""
    W, t = 14, big()
    codes, offs = cm.everything(W)
    for M, modes in ((64, (False, True)), (cm.NW_MAX, (True,))):
        p = pk.Packed(codes, offs, W, M)
        assert cm.item_fields(p.items)[1].max() == M and p.all_whole == 0
        for both in modes:
            ids, cnt, ltot = cm.sparse_count_arrays(codes, offs, W, both)[:3]
            defer_want = int(cm.deferral_model(p.words, p.items, W, both).sum())
            what = "all classes, W = 14, M = %d, %s" % (M, "both strands" if both else "plus strand")
            ctx.upload(p)
            for impl in (1, 2):
                ctx.set_option("count_impl", impl)
                try:
                    _, lt = ctx.count(both, counts=t.dev[impl - 1])
                    assert ctx.info("deferred_items") == defer_want, (what, impl)
                    assert int(lt.to_host()[0]) == ltot == p.n_windows, (what, impl)
                finally:
                    ctx.set_option("count_impl", 0)
            direct, part = t.fetch(0), t.fetch(1)
            got_ids = np.flatnonzero(direct)
            got_cnt = direct[got_ids].astype(np.int64)
            assert int(got_cnt.sum()) == int(cnt.sum()), what
            assert np.array_equal(got_ids, ids), "%s: non-zero bins differ" % what
            assert np.array_equal(got_cnt, cnt), "%s: direct emitter: %s" % (what, first_difference(got_cnt, cnt))
            assert same(direct, part), "%s: the partitioned emitter's table is not the direct one's" % what


SPLIT = [("periods", 0), ("prologue_edge", 0), ("item_lengths", 0), ("item_lengths", 1), ("item_lengths", 2)]


@pytest.mark.parametrize("W", (4, 8, 10, 12, 14))
@pytest.mark.parametrize("cls,k", SPLIT, ids=["%s%d" % c for c in SPLIT])
def test_the_table_does_not_depend_on_how_runs_are_cut_into_items(ctx, big, cls, k, W):
    """every re-split item list of the model, attached by hand through set_sequences: the table, ltot and (where whole)
    the fused and the stand-alone background counters of the packer's items, and as many deferred items as the model
    predicts for that list (lists of up to 100 000 items: the model replays every continuing item's prologue at once)"""
    t = big() if W == 14 else None
    part, p = cm.CLASSES[cls](W)[k], cm.packed(cls, W)[k]
    for both in (False, True):
        words, _ = ctx.upload(p)
        base, lt0, bg0, _ = run(ctx, both, 0, p.all_whole, t.dev[0] if t else None)
        assert lt0 == p.n_windows
        base = t.fetch(0) if t else base.to_host()
        for name, items in cm.resplits(p.items):
            what = "%s, W = %d, %s, items cut %s" % (part["name"], W, "both strands" if both else "plus strand", name)
            nw = cm.item_fields(items)[1]
            ctx.set_sequences(words, ctx.to_device(items), len(p.words), len(items), W, max(64, int(nw.max())),
                              p.max_bin_bound, p.all_whole)
            got, lt, bg, deferred = run(ctx, both, 0, p.all_whole, t.dev[1] if t else None)
            got = t.fetch(1) if t else got.to_host()
            assert same(got, base), "%s: %s" % (what, first_difference(got, base))
            assert lt == lt0, what
            if p.all_whole:
                assert np.array_equal(bg, bg0), "%s: fused background counters" % what
                alone = ctx.bg_count().to_host().astype(np.int64)
                assert np.array_equal(alone, bg0), "%s: stand-alone background count" % what
            if len(items) <= 100_000:
                want = int(cm.deferral_model(p.words, items, W, both).sum())
                assert deferred == want, "%s: %d items deferred, the model says %d" % (what, deferred, want)


@pytest.mark.parametrize("W", (8, 10, 12, 14))
def test_the_sizing_hint_does_not_change_the_table(ctx, big, W):
    """n_windows_hint sizes the key slices of the partitioned emitters: at 1 every level's slices are at their floor and
    overflow into the direct path, at the true figure and at 64 times that they hold everything; 0 = items x item_windows"""
    (p,) = cm.packed("periods", W)
    t = big() if W == 14 else None
    for both in (False, True):
        ctx.upload(p)
        ctx.set_option("n_windows_hint", 0)
        base, lt0, _, d0 = run(ctx, both, 2, False, t.dev[0] if t else None)
        assert lt0 == p.n_windows and d0 == int(cm.deferral_model(p.words, p.items, W, both).sum())
        base = t.fetch(0) if t else base.to_host()
        try:
            for hint in (1, p.n_windows, 64 * p.n_windows):
                ctx.set_option("n_windows_hint", hint)
                got, lt, _, d = run(ctx, both, 2, False, t.dev[1] if t else None)
                got = t.fetch(1) if t else got.to_host()
                assert same(got, base) and lt == lt0 and d == d0, "periods, W = %d, %s, n_windows_hint = %d" % (W, mode(both, 2), hint)
        finally:
            ctx.set_option("n_windows_hint", 0)


def test_a_bin_bound_of_2_to_the_32_is_refused(ctx):
    """pengk_count / pengk_count_bg count in 32-bit bins: a shard whose max_bin_bound says a bin could wrap is refused
    with PENGK_ERR_RANGE, one below that is counted, exactly"""
    W = 6
    codes, offs = po.synth(3, 0, 50, 120)
    p = pk.Packed(codes, offs, W)
    assert p.all_whole == 1
    want, ltot = po.count(codes, offs, W, True)
    words, items = ctx.to_device(p.words), ctx.to_device(p.items)
    ctx.set_sequences(words, items, len(p.words), len(p.items), W, p.item_windows, 2 ** 32, 1)
    for call in (ctx.count, ctx.count_bg):
        with pytest.raises(pk.PengkError) as e:
            call(True)
        assert e.value.code == pk.ERR_RANGE
    ctx.set_sequences(words, items, len(p.words), len(p.items), W, p.item_windows, 2 ** 32 - 1, 1)
    for whole in (False, True):
        counts, lt, bg, _ = run(ctx, True, 0, whole)
        assert lt == ltot and np.array_equal(counts.to_host().astype(np.uint64), want)
        assert bg is None or np.array_equal(bg, po.bg_counts(codes, offs, 2))
