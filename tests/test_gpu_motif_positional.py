"""--positional on the device (include/pengk.h, "positional words"): pengk_position_count against the numpy model of
tests/motif_positional_model.py, the table bit for bit -- every width, anchor and strand setting at the lengths where a
word, a tile or the binned range ends, with one invalid base at every position in turn, without input validity, with a
word and its equal predecessor on either side of a tile seam and of a word seam, on runs that count once, far out of range,
across the tiles and workgroups of 100 000 sequences, in two calls, on a subset of the offset arrays, at the ends of
n_bins and bin_size, and the argument errors."""
import numpy as np
import pytest

import peng_motif_amd as pk
import motif_positional_model as mp
import motif_score_model as ms

pytestmark = pytest.mark.gpu

ANCHORS = (mp.START, mp.END, mp.CENTER)


@pytest.fixture(scope="module")
def ctx():
    c = pk.Context(0)
    yield c
    c.close()


def check_table(ctx, seqs, K, anchor, S, B, both, all_valid=False, want=None, scan=None):
    if scan is None:
        scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    got = ctx.position_count(scan, K, anchor, S, B, both, all_valid=all_valid).to_host()
    if want is None:
        want = mp.tables(seqs, K, anchor, S, B, both)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "K %d anchor %d bin %d key %s: %d, the model %d (%d entries differ)" % (
        K, anchor, bad[0][0], mp.word_string(int(bad[0][1]), K), got[tuple(bad[0])], want[tuple(bad[0])], len(bad))
    return int(want.sum())


def test_symbol():
    assert hasattr(pk.lib(), "pengk_position_count")


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("K", [4, 5, 6, 7])
def test_lengths_at_the_edges(ctx, K, both):
    """0 .. K+1, 63 .. 65, 64+K-1, 64+K, S B - 1, S B, S B + K, odd and even: two letters only, so that words overlap
    themselves, and uniform ones"""
    S, B = 10, 20
    lengths = mp.edge_lengths(K, S, B)
    assert {0, K + 1, 63, 64, 65, 64 + K - 1, 64 + K, 199, 200, 200 + K} <= set(lengths)
    for skew in (True, False):
        seqs = mp.random_sequences(10 + K, lengths, skew=skew)
        scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
        for anchor in ANCHORS:
            assert check_table(ctx, seqs, K, anchor, S, B, both, scan=scan) > 0
            check_table(ctx, seqs, K, anchor, S, B, both, all_valid=True, scan=scan)
            check_table(ctx, seqs, K, anchor, 3, 9, both, scan=scan)    # (most of the longer ones out of range)
        for c in seqs[1:]:   # every one alone (but the empty one: a set without a word)
            check_table(ctx, [c], K, mp.CENTER, S, B, both)


@pytest.mark.parametrize("both", [False, True])
def test_one_invalid_base_at_every_position(ctx, both):
    base = mp.random_sequences(21, [70], skew=True)[0]
    seqs = []
    for p in range(70):
        c = base.copy()
        c[p] = 0
        seqs.append(c)
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    for K in (4, 5, 6, 7):
        for anchor in ANCHORS:
            check_table(ctx, seqs, K, anchor, 5, 14, both, scan=scan)
    for c in seqs[::7] + seqs[60:]:
        check_table(ctx, [c], 6, mp.START, 5, 14, both)


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("K", [4, 5, 6, 7])
def test_equal_predecessors_across_the_seams(ctx, K, both):
    """a stretch of period d = 1 .. K-1 laid over base 32 (two words of the layout) and base 64 (two tiles), begun at every
    base in front of the seam: the predecessor that decides stands on the other side"""
    rng = np.random.default_rng(30 + K)
    seqs = []
    for seam in (32, 64, 128):
        for d in range(1, K):
            unit = rng.permutation(4)[:d] if d <= 4 else rng.integers(0, 4, d)
            for begin in range(seam - K - d, seam + 1):
                c = rng.integers(1, 5, 150).astype(np.uint8)
                n = K + d + 1
                c[begin:begin + n] = np.resize(unit, n) + 1
                seqs.append(c)
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    for anchor in ANCHORS:
        check_table(ctx, seqs, K, anchor, 10, 20, both, scan=scan)
    # ... and with the base in front of the seam invalid: the predecessor does not stand, the word heads a clump
    for c in seqs[::3]:
        c[31] = 0
    check_table(ctx, seqs, K, mp.START, 10, 20, both)


@pytest.mark.parametrize("both", [False, True])
def test_70000_bases_of_one_letter_count_once(ctx, both):
    for letter in "AT":
        c = mp.codes_of(letter * 70000)
        scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten([c])))
        for K in (4, 7):
            h = ctx.position_count(scan, K, mp.START, 65536, 2, both, all_valid=True).to_host()
            key = 0 if both or letter == "A" else 4 ** K - 1
            assert h.sum() == 1 and h[0, key] == 1
        assert ctx.position_count(scan, 6, mp.END, 10, 20, both).to_host().sum() == 0       # (its one head is far from the end)
        assert ctx.position_count(scan, 6, mp.CENTER, 65536, 1, both).to_host().sum() == 1
    check_table(ctx, [mp.codes_of("A" * 35000 + "N" + "A" * 34999)], 6, mp.START, 65536, 2, both)   # two clumps


@pytest.mark.parametrize("both", [False, True])
def test_70000_bases_of_AC_count_their_first_two_positions(ctx, both):
    c = mp.codes_of("AC" * 35000)
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten([c])))
    h = ctx.position_count(scan, 6, mp.START, 65536, 2, both).to_host()
    assert h.sum() == 2 and h[0, mp.key_of("ACACAC")] == 1 and h[0, mp.key_of("CACACA")] == 1
    for K in (4, 5, 7):
        for anchor in ANCHORS:
            check_table(ctx, [c], K, anchor, 1000, 64, both, scan=scan)


def test_a_word_that_is_its_own_reverse_complement_overlapping_itself(ctx):
    c = mp.codes_of("AT" * 10)
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten([c])))
    for both in (False, True):
        h = ctx.position_count(scan, 6, mp.START, 100, 1, both).to_host()
        assert h.sum() == 2 and h[0, mp.key_of("ATATAT")] == 1 and h[0, mp.key_of("TATATA")] == 1
    # GGATATATCC: on both strands the same set of words read from either end
    seqs = [mp.codes_of("GGATATATCC" * 9), mp.codes_of("ACGT" * 40), mp.codes_of("GAATTC" * 30)]
    for K in (4, 5, 6, 7):
        for anchor in ANCHORS:
            check_table(ctx, seqs, K, anchor, 4, 64, True)


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("anchor", ANCHORS)
def test_70000_random_bases_mostly_out_of_range(ctx, anchor, both):
    c = mp.random_sequences(22, [70000])[0]
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten([c])))
    assert check_table(ctx, [c], 6, anchor, 10, 20, both, all_valid=True, scan=scan) > 150
    check_table(ctx, [c], 7, anchor, 1, 64, both, scan=scan)
    c[np.random.default_rng(23).integers(0, 70000, 50)] = 0
    c[[3, 69990, 35001]] = 0
    assert check_table(ctx, [c], 5, anchor, 2000, 64, both) > 60000     # (and all of it in range)
    check_table(ctx, [c], 6, anchor, 10, 20, both)


@pytest.fixture(scope="module")
def many():
    return mp.many_sequences()


def pool_table(pool, idx, *args):
    return mp.tables(pool, *args, weights=np.bincount(idx, minlength=len(pool)))


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
    assert len(seqs) == 100000 and {len(s) for s in seqs} == set(range(301))
    scan = (words, valid, ctx.to_device(lay.offs), ctx.to_device(lay.lens), len(lay.lens))
    check_table(ctx, seqs, K, anchor, 10, 20, both, scan=scan, want=pool_table(pool, idx, K, anchor, 10, 20, both))


@pytest.fixture(scope="module")
def many_want(many):
    _, idx, pool = many
    return pool_table(pool, idx, 6, mp.CENTER, 7, 13, True)


@pytest.mark.parametrize("cut", [1, 255, 256, 257, 50001])
def test_two_calls_give_the_table_of_one(ctx, many_on_device, many_want, cut):
    lay, words, valid = many_on_device
    n = len(lay.lens)
    counts = ctx.to_device(np.zeros((13, 4096), np.uint64))
    for a, b in ((0, cut), (cut, n)):
        part = (words, valid, ctx.to_device(lay.offs[a:b]), ctx.to_device(lay.lens[a:b]), b - a)
        ctx.position_count(part, 6, mp.CENTER, 7, 13, True, counts=counts)
    assert np.array_equal(counts.to_host(), many_want)


def test_a_subset_that_is_not_contiguous(ctx, many, many_on_device):
    seqs, idx, pool = many
    lay, words, valid = many_on_device
    pick = np.flatnonzero(np.random.default_rng(24).random(len(seqs)) < 0.3)[::-1].copy()   # (and in another order)
    part = (words, valid, ctx.to_device(lay.offs[pick]), ctx.to_device(lay.lens[pick]), len(pick))
    for K, anchor, both in ((6, mp.END, False), (5, mp.CENTER, True)):
        got = ctx.position_count(part, K, anchor, 10, 20, both).to_host()
        assert np.array_equal(got, pool_table(pool, idx[pick], K, anchor, 10, 20, both))


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("K", [4, 5, 6, 7])
def test_one_bin_64_bins_and_bins_of_one_position(ctx, K, both):
    seqs = mp.random_sequences(40 + K, [0, 5, 63, 64, 65, 70, 130, 200, 257, 300], skew=True) + mp.random_sequences(50 + K, [90, 91, 400])
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    for anchor in ANCHORS:
        for S, B in ((1, 1), (1, 64), (10, 1), (3, 64), (65536, 1), (65536, 64), (64, 2)):
            check_table(ctx, seqs, K, anchor, S, B, both, scan=scan)


def test_no_sequence_and_argument_errors(ctx):
    seqs = [mp.codes_of("ACGTTGCATT" * 4)]
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    counts = ctx.to_device(np.full((20, 4096), 7, np.uint64))
    ctx.position_count(scan, 6, mp.START, 10, 20, True, counts=counts, n_seq=0)
    assert (counts.to_host() == 7).all()
    ctx.position_count(scan, 6, mp.START, 10, 20, True, counts=counts)   # added to, not written
    ctx.position_count(scan, 6, mp.START, 10, 20, True, counts=counts)
    assert np.array_equal(counts.to_host(), 7 + 2 * mp.tables(seqs, 6, mp.START, 10, 20, True))
    good = dict(K=6, anchor=2, bin_size=10, n_bins=20, both=1)
    for name, values in (("K", (3, 8, -1, 0)), ("anchor", (-1, 3)), ("bin_size", (0, -1, 65537)), ("n_bins", (0, -1, 65)),
                         ("both", (2, -1))):
        for v in values:
            a = dict(good, **{name: v})
            with pytest.raises(pk.PengkError) as e:
                ctx.position_count(scan, a["K"], a["anchor"], a["bin_size"], a["n_bins"], a["both"], counts=counts)
            assert e.value.code == pk.ERR_ARG, (name, v)
    with pytest.raises(pk.PengkError) as e:
        ctx.position_count(scan, 6, 2, 10, 20, True, counts=counts, n_seq=1 << 32)
    assert e.value.code == pk.ERR_ARG
    # a null pointer with n_seq > 0 (d_valid may be null: every base valid); with n_seq = 0 nothing is read
    ptrs = [x.ptr for x in scan[:4]]
    call = lambda w, v, o, l, n, c: pk.lib().pengk_position_count(ctx.h, w, v, o, l, n, 6, 2, 10, 20, 1, c)
    cp = counts.ptr
    assert call(None, ptrs[1], ptrs[2], ptrs[3], 1, cp) == pk.ERR_ARG
    assert call(ptrs[0], ptrs[1], None, ptrs[3], 1, cp) == pk.ERR_ARG
    assert call(ptrs[0], ptrs[1], ptrs[2], None, 1, cp) == pk.ERR_ARG
    assert call(ptrs[0], ptrs[1], ptrs[2], ptrs[3], 1, None) == pk.ERR_ARG
    assert call(None, None, None, None, 0, None) == 0
    assert call(ptrs[0], None, ptrs[2], ptrs[3], 1, cp) == 0
    ctx.synchronize()


@pytest.mark.parametrize("K", [4, 5, 6, 7])
def test_the_same_call_repeated_gives_the_same_table(ctx, K):
    """100 calls on one small set under each anchor: the table is the model's every time (a draft of the kernel was right
    most of the time and wrong in one call of ten; a single comparison would have let it through)"""
    seqs = mp.random_sequences(10 + K, mp.edge_lengths(K, 10, 20), skew=True)
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    for anchor, S, B in ((mp.START, 1, 64), (mp.END, 3, 9), (mp.CENTER, 1, 64), (mp.CENTER, 10, 20)):
        want = mp.tables(seqs, K, anchor, S, B, False)
        counts = ctx.to_device(np.zeros_like(want))
        for r in range(25):
            ctx.position_count(scan, K, anchor, S, B, False, counts=counts)
            assert np.array_equal(counts.to_host(), (r + 1) * want), (anchor, S, B, r)
