"""The count at W = 10 on both strands through the 16-bucket split of csrc/count.hip: pass A with groups of 128 keys of 16
bits (256-entry rings, exact slice fills, suppressed windows travelling as the keys of the never-counted id 4^W - 1), pass B
with 2^16 bins as packed 16-bit halves checked once per workgroup, pass C storing 0 in the last bin.

Everything is integer and compared bit for bit with the oracle (pinned to the compiled reference): the table before and
after pengk_mirror_counts, ltot and the 84 fused background counters, through pengk_count and pengk_count_bg, into
fresh, uncleared device buffers.  Every case runs with count_group = 0 (automatic: groups of 128 here) and with
count_group = 64 (the 32-bucket emitter), which must give the same bits; the info keys "count_group_used" and
"count_wrapped_workgroups" tell which emitter and which path of pass B ran, and the test hook "count_slice_fill" reads the
fills pass A published, which pin the fill model the exact-fill cases are built with."""
import functools

import numpy as np
import pytest

import count_edges_model as cm
import peng_motif_amd as pk
from oracle import oracle as po

pytestmark = pytest.mark.gpu

W = 10
LAST = 4 ** W - 1  # poly-T: never a canonical id (its reverse complement 0 is smaller)


@pytest.fixture(scope="module")
def ctx():
    c = pk.Context(0)
    yield c
    for k in ("count_impl", "count_group", "key_cap_override"):
        c.set_option(k, 0)
    c.close()


class Reference:
    """the oracle's answers for one input, computed once"""

    def __init__(self, codes, offs, w=W):
        self.codes, self.offs, self.W = codes, offs, w
        self.bg = po.bg_counts(codes, offs, 2)

    @functools.lru_cache(None)
    def count(self, both=True):
        want, ltot = po.count(self.codes, self.offs, self.W, both)
        assert int(want.max()) < 2 ** 32
        return want.astype(np.uint32), ltot

    @functools.lru_cache(None)
    def before_mirror(self):
        return canonical_only(self.count(True)[0], self.W)


def canonical_only(want, w=W):
    """a mirrored both-strand table as it stands before pengk_mirror_counts: counts on the ids x <= revcomp(x) only"""
    x = np.arange(4 ** w, dtype=np.int64)
    out = want.copy()
    out[x > cm.revcomp_ids(x, w)] = 0
    return out


def differ(what, got, want):
    bad = np.flatnonzero(got != want)
    return "%s: %d bins differ, the first: bin %d, device %d, oracle %d" % (what, bad.size, bad[0], got[bad[0]], want[bad[0]])


def run(ctx, ref, p, group, with_bg, what, both=True):
    """count what is attached with count_group = group; everything against the oracle.  -> info of that count"""
    want, ltot = ref.count(both)
    what = "%s, count_group %d, %s" % (what, group, "count_bg" if with_bg else "count")
    ctx.set_option("count_group", group)
    try:
        counts = ctx.empty(4 ** p.W, np.uint32)
        if with_bg:
            assert p.all_whole == 1, what
            counts, lt, bg = ctx.count_bg(both, counts=counts)
        else:
            counts, lt = ctx.count(both, counts=counts)
        info = {k: ctx.info(k) for k in ("count_group_used", "count_wrapped_workgroups", "deferred_items")}
        got = counts.to_host()
        if both:
            before = ref.before_mirror()
            assert np.array_equal(got, before), differ(what + ", before the mirror", got, before)
            assert got[4 ** p.W - 1] == 0, what
            ctx.mirror(p.W, counts)
            got = counts.to_host()
            assert got[4 ** p.W - 1] == got[0], what
        assert np.array_equal(got, want), differ(what, got, want)
        assert int(lt.to_host()[0]) == ltot == p.n_windows, what
        if with_bg:
            assert np.array_equal(bg.to_host().astype(np.int64), ref.bg), "%s: fused background counters" % what
        return info
    finally:
        ctx.set_option("count_group", 0)


def both_emitters(ctx, ref, p, what, with_bg=(True, False), deferred=None):
    """groups of 128 (automatic) and of 64 on the attached input (deferred items: as many as the model says);
    -> pass-B workgroups that recounted, under groups of 128"""
    wrapped = 0
    if deferred is None:
        deferred = int(cm.deferral_model(p.words, p.items, p.W, True).sum())
    for bg in sorted(set(bool(b) and p.all_whole == 1 for b in with_bg)):  # (the fused background count needs whole sequences)
        for group, used in ((0, 128), (64, 64)):
            info = run(ctx, ref, p, group, bg, what)
            assert info["count_group_used"] == used, what
            assert info["deferred_items"] == deferred, "%s: %d items deferred, the model says %d" % (what, info["deferred_items"], deferred)
            if used == 64:
                assert info["count_wrapped_workgroups"] == 0, what
            else:
                wrapped = max(wrapped, info["count_wrapped_workgroups"])
    return wrapped


# ---- 1. ragged and tiny -----------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def ragged_sequences():
    rng = np.random.default_rng(12801)
    seqs = []
    for i in range(3000):
        s = cm.rand(rng, int(rng.integers(W, 301)))
        if i % 17 == 0:
            s[rng.integers(0, len(s), size=1 + i % 3)] = 0  # N
        seqs.append(s)
    return seqs


def test_ragged_lengths_with_N(ctx):
    """a few thousand sequences of W .. 300 bases, some with N: items of mixed lengths in every wave, whatever ids occur
    split and joined through the 16-bit keys; no workgroup of pass B wraps"""
    for with_n in (True, False):  # (with N: pengk_count alone; the sequences without N: pengk_count_bg too)
        codes, offs = cm.join([s for s in ragged_sequences() if with_n or s.min() > 0])
        ref, p = Reference(codes, offs), pk.Packed(codes, offs, W)
        assert p.all_whole == (0 if with_n else 1)
        ctx.upload(p)
        assert both_emitters(ctx, ref, p, "ragged, %s N" % ("with" if with_n else "without")) == 0


@pytest.mark.parametrize("n", (1, 63, 64, 65, 257))
def test_tiny_item_counts(ctx, n):
    """dead lanes, a single wave, a partial last workgroup"""
    seqs = [s for s in ragged_sequences() if s.min() > 0][:n]
    codes, offs = cm.join(seqs)
    ref, p = Reference(codes, offs), pk.Packed(codes, offs, W, 512)  # (items of up to 512 windows: one per sequence)
    assert len(p.items) == n and p.all_whole == 1
    ctx.upload(p)
    assert both_emitters(ctx, ref, p, "%d items" % n) == 0


# ---- 2. suppressed windows as ordinary keys ---------------------------------------------------------------------------------
def test_suppressed_windows_travel_as_keys_of_the_last_bin(ctx):
    """poly-A and poly-T runs, tandem repeats of period 1 .. 9 and reverse-complement palindromes longer than W between
    random flanks, in waves of equally long sequences (the full and tail bodies append suppressed windows) and of mixed
    ones: the last bin is 0 before the mirror and table[0] after it (checked by run())"""
    rng = np.random.default_rng(12802)
    seqs = []
    for rep in range(40):
        for L in (200, 200 + rep % 5):
            units = [cm.seq("A"), cm.seq("T")] + [cm.rand(rng, q) for q in range(1, 10)]
            for u in units:
                n = int(rng.integers(W + 1, 60))
                seqs.append(np.concatenate([cm.rand(rng, 50), cm.tile(u, n), cm.rand(rng, L - 50 - n)]))
            for half in (6, 8, 11):
                h = cm.rand(rng, half)
                pal = np.concatenate([h, cm.revcomp_codes(h)])
                seqs.append(np.concatenate([cm.rand(rng, 40), pal, cm.rand(rng, L - 40 - 2 * half)]))
    seqs = sorted(seqs[:len(seqs) // 2], key=len) + seqs[len(seqs) // 2:]  # waves of equal lengths, then mixed ones
    codes, offs = cm.join(seqs)
    ref, p = Reference(codes, offs), pk.Packed(codes, offs, W)
    want, ltot = ref.count()
    assert ltot > int(canonical_only(want).sum()), "no window of this input is suppressed"
    assert want[0] > 0  # poly-A / poly-T
    ctx.upload(p)
    both_emitters(ctx, ref, p, "suppressed windows")


# ---- 3. the ring at its worst case ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kinds", (1, 2))
def test_every_lane_appends_to_the_same_ring(ctx, kinds):
    """4096 copies of one random 200-bp sequence (of two, alternating): at every step all 64 lanes of a wave (every other
    lane) append the same key to the same ring"""
    rng = np.random.default_rng(12803)
    base = [cm.rand(rng, 200) for _ in range(kinds)]
    codes, offs = cm.join([base[i % kinds] for i in range(4096)])
    ref, p = Reference(codes, offs), pk.Packed(codes, offs, W)
    ctx.upload(p)
    both_emitters(ctx, ref, p, "4096 copies of %d sequences" % kinds)


# ---- 4. exact fills and partial groups --------------------------------------------------------------------------------------
def fills16(p):
    """Model of the 16-bucket emitter's slice fills, [wave][bucket], for an item list that no wave walks twice (one item
    per lane of the grid) and in which no window is suppressed or deferred: wave g appends the windows of the items 64 g ..
    64 g + 63, each to the bucket its canonical id's bits [8, 12) name, and publishes exactly that many."""
    ws, nw, _ = cm.item_fields(p.items)
    pos, which = cm._ranges(ws, nw)
    canon = cm.window_ids(cm.stream_bases(p.words), p.W)[1][pos]
    out = np.zeros(((len(ws) + 63) // 64, 16), np.int64)
    np.add.at(out, (which // 64, (canon >> 8) & 15), 1)
    return out


def device_fills(ctx):
    """the fills pass A of the last count published, [wave][bucket] over every launched wave"""
    n = ctx.info("count_slices")
    assert n > 0 and n % 16 == 0
    out = np.zeros(n, np.int64)
    for i in range(n):
        ctx.set_option("count_probe_slice", i)
        out[i] = ctx.info("count_slice_fill")
    ctx.set_option("count_probe_slice", 0)
    return out.reshape(-1, 16)


@functools.lru_cache(None)
def exact_fill_input(residue):
    """64 clean sequences (no window suppressed on either strand), the last cut so that bucket 5 of the wave that scans
    it ends `residue` entries into a group (128: on a group's end)"""
    rng = np.random.default_rng(12804)
    seqs = [cm.clean_random(rng, 150, W) for _ in range(63)]
    tail = cm.clean_random(rng, 4700, W)
    for n in range(len(tail), W, -1):
        codes, offs = cm.join(seqs + [tail[:n]])
        p = pk.Packed(codes, offs, W)
        f = fills16(p)
        if f[-1, 5] > 128 and (f[-1, 5] - 1) % 128 + 1 == residue:
            assert cm.sparse_count_arrays(codes, offs, W, True)[3].all() and cm.deferral_model(p.words, p.items, W, True).sum() == 0
            return codes, offs, f
    raise AssertionError("no cut of the last sequence leaves %d entries in the last group" % residue)


@pytest.mark.parametrize("residue", (1, 127, 128))
def test_slices_that_end_inside_a_group(ctx, residue):
    """slices whose last group holds 1, 127 and 128 entries; with slices of 128 and 256 keys the first groups fill the
    slice, the following ones overflow into the bucket-major table and the partial last group of a full slice adds only
    its valid entries; with slices of the default size it leaves as a line and pass B reads its valid entries alone"""
    codes, offs, fills = exact_fill_input(residue)
    assert fills.max() > 2 * 256 and (fills % 128 != 0).any()
    ref, p = Reference(codes, offs), pk.Packed(codes, offs, W)
    ctx.upload(p)
    for cap in (0, 128, 256):
        ctx.set_option("key_cap_override", cap)
        try:
            what = "last group of %d entries, slices of %s keys" % (residue, cap or "default")
            both_emitters(ctx, ref, p, what)
            # the model against the device: what pass A published is the model's fill, capped at what a full slice holds
            assert run(ctx, ref, p, 0, False, what)["count_group_used"] == 128
            got = device_fills(ctx)
            want = np.zeros_like(got)
            want[:len(fills)] = np.minimum(fills, cap) if cap else fills
            assert np.array_equal(got, want), "%s: published fills\n%s\nthe model's\n%s" % (what, got[:len(fills)], want[:len(fills)])
        finally:
            ctx.set_option("key_cap_override", 0)


def test_deferred_items_beside_overflowed_slices(ctx):
    """the model's repeats of every period cut into items of 64 windows: dozens of deferred items, whose fix-up adds
    into the bucket-major table in its 16-bucket layout, beside slices of 128 keys and of the default size"""
    (part,), (p,) = cm.CLASSES["periods"](W), cm.packed("periods", W)
    ref = Reference(part["codes"], part["offs"])
    want = int(cm.deferral_model(p.words, p.items, W, True).sum())
    assert want > 0
    ctx.upload(p)
    for cap in (0, 128):
        ctx.set_option("key_cap_override", cap)
        try:
            both_emitters(ctx, ref, p, "periods, slices of %s keys" % (cap or "default"), deferred=want)
        finally:
            ctx.set_option("key_cap_override", 0)


# ---- 5. the wrap path -------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def wrap_unit():
    """a 10-mer whose ten rotations have distinct canonical ids, some with payload bit 15 (id bit 19) clear and some set"""
    rng = np.random.default_rng(12805)
    while True:
        u = cm.rand(rng, W)
        ids = cm.window_ids(np.concatenate([u, u]).astype(np.int64)[:2 * W - 1] - 1, W)[1]
        if len(set(ids.tolist())) == W and 2 <= int(((ids >> 19) & 1).sum()) <= W - 2:
            return u, ids


def test_a_workgroup_whose_packed_bins_wrap_recounts_exactly(ctx):
    """20 000 copies of a 200-bp tandem repeat of one 10-mer: ten ids with ~390 000 counts each, in both halves of the
    packed words, and at most a handful of pass-B workgroups per bucket -- their halves wrap, the check at the end of
    the workgroup sees it, and the slices are recounted with device-scope adds"""
    u, ids = wrap_unit()
    copies = 20000
    codes, offs = cm.join([cm.tile(u, 200)] * copies)
    ref, p = Reference(codes, offs), pk.Packed(codes, offs, W)
    want, _ = ref.count()
    # the workgroups of pass B per bucket, as launch_partition_w sizes them
    bpb = min((2 * ctx.info("num_cu") + 15) // 16, (p.n_windows // 16 + 1 + 65535) // 65536, (len(p.items) + 255) // 256 * 4)
    for half in (0, 1):
        share = [int(want[i]) // bpb for i in ids.tolist() if (i >> 19) & 1 == half]
        assert share and max(share) > 65535, "bit 15 %s: %s counts per workgroup do not wrap a 16-bit half" % (half, share)
    ctx.upload(p)
    assert both_emitters(ctx, ref, p, "tandem repeat of a 10-mer", with_bg=(True,)) >= 1


# ---- 6. where the 16-bucket split does not apply -----------------------------------------------------------------------------
@pytest.mark.parametrize("w,both", ((10, False), (8, True)), ids=("W10-plus", "W8-both"))
def test_other_configurations_keep_the_emitter_of_64(ctx, w, both):
    codes, offs = po.synth(21, 0, 700, 120)
    ref, p = Reference(codes, offs, w), pk.Packed(codes, offs, w)
    ctx.upload(p)
    info = run(ctx, ref, p, 0, True, "W = %d, %s" % (w, "both strands" if both else "plus strand"), both=both)
    assert info["count_group_used"] == 64 and info["count_wrapped_workgroups"] == 0
    ctx.set_option("count_group", 128)
    try:
        with pytest.raises(pk.PengkError) as e:
            ctx.count(both)
        assert "count_group 128" in str(e.value) and "W = 10 on both strands" in str(e.value)
        assert "count_group 128" in pk.lib().pengk_last_error().decode()
    finally:
        ctx.set_option("count_group", 0)
    run(ctx, ref, p, 64, False, "W = %d after the refusal" % w, both=both)


def test_count_group_values(ctx):
    with pytest.raises(pk.PengkError):
        ctx.set_option("count_group", 32)
    codes, offs = po.synth(22, 0, 300, 100)
    ref, p = Reference(codes, offs), pk.Packed(codes, offs, W)
    ctx.upload(p)
    assert run(ctx, ref, p, 128, True, "count_group forced")["count_group_used"] == 128
    ctx.set_option("count_group", 64)
    assert ctx.info("count_group") == 64  # (the option as set; count_group_used: what the last count ran)
    ctx.set_option("count_group", 0)
    ctx.set_option("count_impl", 1)  # the direct emitter has no groups
    try:
        assert run(ctx, ref, p, 0, True, "direct emitter")["count_group_used"] == 0
        ctx.set_option("count_group", 128)
        with pytest.raises(pk.PengkError):
            ctx.count(True)
    finally:
        ctx.set_option("count_group", 0)
        ctx.set_option("count_impl", 0)
