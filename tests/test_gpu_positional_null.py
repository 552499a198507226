"""--positional-null composition on the device (include/pengk.h, "the composition null of the positional report"):
pengk_position_pairs against the numpy model of tests/positional_null_model.py, the table bit for bit -- every width, anchor
and strand setting at the lengths where a word, a tile or the binned range ends, with one invalid base at every position in
turn, with a word's first and last pair on either side of a word seam and a tile seam, on 70 000 bases of one key, far out
of range, across the tiles and workgroups of 100 000 sequences, in two calls, on a subset of the offset arrays, at the ends of
n_bins and bin_size, repeated, on a caller-owned stream, and the argument errors."""
import numpy as np
import pytest
import torch  # noqa: F401  (the gate's streams are torch's: its HIP runtime is loaded before the library's, whichever test runs first)

import peng_motif_amd as pk
import motif_positional_model as mp
import motif_score_model as ms
import positional_null_model as pn
import stream_gate as sg
from test_gpu_stream_order import through_the_gate

pytestmark = pytest.mark.gpu

ANCHORS = (mp.START, mp.END, mp.CENTER)


@pytest.fixture(scope="module")
def ctx():
    c = pk.Context(0)
    yield c
    c.close()


def check_pairs(ctx, seqs, K, anchor, S, B, both, all_valid=False, want=None, scan=None):
    if scan is None:
        scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    got = ctx.position_pairs(scan, K, anchor, S, B, both, all_valid=all_valid).to_host()
    if want is None:
        want = pn.pair_tables(seqs, K, anchor, S, B, both)
    assert got.shape == want.shape == (B, 16)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "K %d anchor %d S %d B %d bin %d pair %s%s: %d, the model %d (%d entries differ)" % (
        K, anchor, S, B, bad[0][0], mp.LETTERS[bad[0][1] >> 2], mp.LETTERS[bad[0][1] & 3], got[tuple(bad[0])], want[tuple(bad[0])], len(bad))
    return int(want.sum())


def test_symbol():
    assert hasattr(pk.lib(), "pengk_position_pairs")


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("K", [4, 5, 6, 7])
def test_lengths_at_the_edges(ctx, K, both):
    S, B = 10, 20
    lengths = mp.edge_lengths(K, S, B)
    assert {0, K + 1, 63, 64, 65, 64 + K - 1, 64 + K, 199, 200, 200 + K} <= set(lengths)
    for skew in (True, False):
        seqs = mp.random_sequences(10 + K, lengths, skew=skew)
        scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
        for anchor in ANCHORS:
            assert check_pairs(ctx, seqs, K, anchor, S, B, both, scan=scan) > 0
            check_pairs(ctx, seqs, K, anchor, S, B, both, all_valid=True, scan=scan)
            check_pairs(ctx, seqs, K, anchor, 3, 9, both, scan=scan)    # (most of the longer ones out of range)
        for c in seqs[1:]:   # every one alone (but the empty one: a set without a word)
            check_pairs(ctx, [c], K, mp.CENTER, S, B, both)


@pytest.mark.parametrize("both", [False, True])
def test_one_invalid_base_at_every_position(ctx, both):
    base = mp.random_sequences(21, [70])[0]
    seqs = []
    for p in range(70):
        c = base.copy()
        c[p] = 0
        seqs.append(c)
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    for K in (4, 5, 6, 7):
        for anchor in ANCHORS:
            check_pairs(ctx, seqs, K, anchor, 5, 14, both, scan=scan)
    for c in seqs[::7] + seqs[60:]:
        check_pairs(ctx, [c], 6, mp.START, 5, 14, both)


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("K", [4, 5, 6, 7])
def test_words_across_the_seams(ctx, K, both):
    """a marked window of K bases -- its first pair and its last pair unlike anything around it: C G .. T C in a sea of A --
    laid over base 32 (two words of the layout), base 64 (two tiles) and base 128, begun at every offset in front of the seam;
    the other strand's pair reads s[p+K-1] and s[p+K-2] from the far side"""
    seqs = []
    for seam in (32, 64, 128):
        for begin in range(seam - K - 1, seam + 2):
            c = np.full(150, 1, np.uint8)
            c[begin:begin + K] = mp.codes_of(("CG" + "A" * K)[:K - 2] + "TC")
            seqs.append(c)
            d = mp.random_sequences(100 + begin, [150])[0]
            d[begin + K] = 0       # ... and random letters, the last word in front of an invalid base
            seqs.append(d)
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    for anchor in ANCHORS:
        check_pairs(ctx, seqs, K, anchor, 10, 20, both, scan=scan)
        check_pairs(ctx, seqs, K, anchor, 1, 64, both, scan=scan)
    for c in seqs[::5]:
        check_pairs(ctx, [c], K, mp.START, 7, 22, both)


@pytest.mark.parametrize("both", [False, True])
def test_70000_bases_of_one_key(ctx, both):
    """one hot counter: every lane of every tile adds the same pair"""
    for text in ("A" * 70000, "AC" * 35000):
        c = mp.codes_of(text)
        scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten([c])))
        for anchor in ANCHORS:
            for S, B in ((65536, 2), (1000, 64)):
                assert check_pairs(ctx, [c], 6, anchor, S, B, both, scan=scan) >= 64000
        check_pairs(ctx, [c], 4, mp.START, 65536, 2, both, all_valid=True, scan=scan)
        check_pairs(ctx, [c], 7, mp.CENTER, 10, 20, both, scan=scan)
    h = ctx.position_pairs(ctx.upload_scan(pk.ScanLayout(*ms.flatten([mp.codes_of("A" * 70000)]))), 6, mp.START, 65536, 2, both).to_host()
    assert h[0, 0] == 65536 and h[1, 0] == 70000 - 5 - 65536 and h[0, 15] == (65536 if both else 0)


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("anchor", ANCHORS)
def test_70000_random_bases_mostly_out_of_range(ctx, anchor, both):
    c = mp.random_sequences(22, [70000])[0]
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten([c])))
    assert check_pairs(ctx, [c], 6, anchor, 10, 20, both, all_valid=True, scan=scan) > 150
    check_pairs(ctx, [c], 7, anchor, 1, 64, both, scan=scan)
    c[np.random.default_rng(23).integers(0, 70000, 50)] = 0
    c[[3, 69990, 35001]] = 0
    assert check_pairs(ctx, [c], 5, anchor, 2000, 64, both) > 60000     # (and all of it in range)
    check_pairs(ctx, [c], 6, anchor, 10, 20, both)


@pytest.fixture(scope="module")
def many():
    return mp.many_sequences()


def pool_pairs(pool, idx, *args):
    return pn.pair_tables(pool, *args, weights=np.bincount(idx, minlength=len(pool)))


@pytest.fixture(scope="module")
def many_on_device(ctx, many):
    seqs, idx, pool = many
    lay = pk.ScanLayout(*ms.flatten(seqs))
    return lay, ctx.to_device(lay.words), ctx.to_device(lay.valid)


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("K,anchor", [(6, mp.CENTER), (4, mp.START), (5, mp.END), (7, mp.CENTER)])
def test_100000_sequences(ctx, many, many_on_device, K, anchor, both):
    seqs, idx, pool = many
    lay, words, valid = many_on_device
    assert len(seqs) == 100000
    scan = (words, valid, ctx.to_device(lay.offs), ctx.to_device(lay.lens), len(lay.lens))
    check_pairs(ctx, seqs, K, anchor, 10, 20, both, scan=scan, want=pool_pairs(pool, idx, K, anchor, 10, 20, both))


@pytest.fixture(scope="module")
def many_want(many):
    _, idx, pool = many
    return pool_pairs(pool, idx, 6, mp.CENTER, 7, 13, True)


@pytest.mark.parametrize("cut", [1, 255, 256, 257, 50001])
def test_two_calls_give_the_table_of_one(ctx, many_on_device, many_want, cut):
    lay, words, valid = many_on_device
    n = len(lay.lens)
    pairs = ctx.to_device(np.zeros((13, 16), np.uint64))
    for a, b in ((0, cut), (cut, n)):
        part = (words, valid, ctx.to_device(lay.offs[a:b]), ctx.to_device(lay.lens[a:b]), b - a)
        ctx.position_pairs(part, 6, mp.CENTER, 7, 13, True, pairs=pairs)
    assert np.array_equal(pairs.to_host(), many_want)


def test_a_subset_that_is_not_contiguous(ctx, many, many_on_device):
    seqs, idx, pool = many
    lay, words, valid = many_on_device
    pick = np.flatnonzero(np.random.default_rng(24).random(len(seqs)) < 0.3)[::-1].copy()   # (and in reverse order)
    part = (words, valid, ctx.to_device(lay.offs[pick]), ctx.to_device(lay.lens[pick]), len(pick))
    for K, anchor, both in ((6, mp.END, False), (5, mp.CENTER, True)):
        got = ctx.position_pairs(part, K, anchor, 10, 20, both).to_host()
        assert np.array_equal(got, pool_pairs(pool, idx[pick], K, anchor, 10, 20, both))


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("K", [4, 5, 6, 7])
def test_one_bin_64_bins_and_bins_of_one_position(ctx, K, both):
    seqs = mp.random_sequences(40 + K, [0, 5, 63, 64, 65, 70, 130, 200, 257, 300], skew=True) + mp.random_sequences(50 + K, [90, 91, 400])
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    for anchor in ANCHORS:
        for S, B in ((1, 1), (1, 64), (3, 64), (65536, 1), (65536, 64), (64, 2)):
            check_pairs(ctx, seqs, K, anchor, S, B, both, scan=scan)


def test_no_sequence_and_argument_errors(ctx):
    seqs = [mp.codes_of("ACGTTGCATT" * 4)]
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    pairs = ctx.to_device(np.full((20, 16), 7, np.uint64))
    ctx.position_pairs(scan, 6, mp.START, 10, 20, True, pairs=pairs, n_seq=0)
    assert (pairs.to_host() == 7).all()
    ctx.position_pairs(scan, 6, mp.START, 10, 20, True, pairs=pairs)   # added to, not written
    ctx.position_pairs(scan, 6, mp.START, 10, 20, True, pairs=pairs)
    assert np.array_equal(pairs.to_host(), 7 + 2 * pn.pair_tables(seqs, 6, mp.START, 10, 20, True))
    good = dict(K=6, anchor=2, bin_size=10, n_bins=20, both=1)
    for name, values in (("K", (3, 8, -1, 0)), ("anchor", (-1, 3)), ("bin_size", (0, -1, 65537)), ("n_bins", (0, -1, 65)),
                         ("both", (2, -1))):
        for v in values:
            a = dict(good, **{name: v})
            with pytest.raises(pk.PengkError) as e:
                ctx.position_pairs(scan, a["K"], a["anchor"], a["bin_size"], a["n_bins"], a["both"], pairs=pairs)
            assert e.value.code == pk.ERR_ARG, (name, v)
    with pytest.raises(pk.PengkError) as e:
        ctx.position_pairs(scan, 6, 2, 10, 20, True, pairs=pairs, n_seq=1 << 32)
    assert e.value.code == pk.ERR_ARG
    # a null pointer with n_seq > 0 (d_valid may be null: every base valid); with n_seq = 0 nothing is read
    ptrs = [x.ptr for x in scan[:4]]
    call = lambda w, v, o, l, n, c: pk.lib().pengk_position_pairs(ctx.h, w, v, o, l, n, 6, 2, 10, 20, 1, c)
    cp = pairs.ptr
    assert call(None, ptrs[1], ptrs[2], ptrs[3], 1, cp) == pk.ERR_ARG
    assert call(ptrs[0], ptrs[1], None, ptrs[3], 1, cp) == pk.ERR_ARG
    assert call(ptrs[0], ptrs[1], ptrs[2], None, 1, cp) == pk.ERR_ARG
    assert call(ptrs[0], ptrs[1], ptrs[2], ptrs[3], 1, None) == pk.ERR_ARG
    assert call(None, None, None, None, 0, None) == 0
    assert call(ptrs[0], None, ptrs[2], ptrs[3], 1, cp) == 0
    ctx.synchronize()


@pytest.mark.parametrize("K", [4, 5, 6, 7])
def test_the_same_call_repeated_gives_the_same_table(ctx, K):
    seqs = mp.random_sequences(10 + K, mp.edge_lengths(K, 10, 20), skew=True)
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    for anchor, S, B in ((mp.START, 1, 64), (mp.END, 3, 9), (mp.CENTER, 1, 64), (mp.CENTER, 10, 20)):
        want = pn.pair_tables(seqs, K, anchor, S, B, True)
        pairs = ctx.to_device(np.zeros_like(want))
        for r in range(25):
            ctx.position_pairs(scan, K, anchor, S, B, True, pairs=pairs)
            assert np.array_equal(pairs.to_host(), (r + 1) * want), (anchor, S, B, r)


def test_on_a_caller_owned_stream_in_order_without_a_host_wait():
    """after pengk_set_stream, behind the gate of tests/stream_gate.py: the scan layout holds poison until the gate has passed,
    the tables are zeroed behind it and copied right behind the calls that add to them, one host wait at the end.  The word
    count and the pair count share their scratch in the stream's order."""
    gate = sg.Gate(0)
    sg.positive_control(gate)   # (raises when the set-up cannot see a copy that overtakes the gate)
    c = pk.Context(0)
    try:
        c.set_stream(gate.s)
        ch = sg.Chain(gate)
        (real, _), (poison, _) = sg.scan_layout(False), sg.scan_layout(True)
        want = dict(pairs=pn.pair_tables(real, 6, mp.CENTER, 10, 20, True), counts=mp.tables(real, 6, mp.CENTER, 10, 20, True))
        assert not np.array_equal(want["pairs"], pn.pair_tables(poison, 6, mp.CENTER, 10, 20, True))
        scan = sg.scan_buffers(ch)
        b = {name: ch.out(name, w.shape, w.dtype, added_to=True) for name, w in want.items()}

        def steps():
            c.position_count(scan, 6, mp.CENTER, 10, 20, True, counts=b["counts"])
            yield
            c.position_pairs(scan, 6, mp.CENTER, 10, 20, True, pairs=b["pairs"])
            ch.take("pairs", "counts")
            yield

        through_the_gate("position_pairs", ch, steps, lambda got: sg.check_bits(got, want), True)
    finally:
        c.close()
