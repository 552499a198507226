"""--holdout on the device (include/pengk.h, "a hold-out share"): pengk_split_sequences against the numpy model of
tests/motif_holdout_model.py, bit for bit -- both compacted shares, the counts and the classes, at the wave and tile edges,
at the threshold's ends, sharded, at the top of the index range, through an index list -- its argument errors, and the
two consumers of its output: pengk_pack_scan of the training pair against the host packer, and pengk_motif_enrich over the
two pairs against the call over the whole set."""
import numpy as np
import pytest

import peng_motif_amd as pk
import motif_erase_model as me
import motif_holdout_model as mh
import motif_score_model as ms

pytestmark = pytest.mark.gpu

TILE = 2048  # csrc/split.hip: sequences per workgroup
THRESHOLDS = [0, 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32]
BIG = 100003  # 48 full tiles and 1699 sequences of a 49th


@pytest.fixture(scope="module")
def ctx():
    c = pk.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def arrays():
    """offs / lens of BIG sequences of 1 - 40 bases in the scan layout's manner (every sequence from a word boundary)"""
    rng = np.random.default_rng(21)
    lens = rng.integers(1, 41, BIG).astype(np.uint32)
    offs = (np.concatenate([[0], np.cumsum((lens.astype(np.int64) + 31) // 32)])[:-1] * 32).astype(np.int64)
    return offs, lens


def run_split(ctx, seed, seq0, offs, lens, threshold, index=None):
    """the device's split of the host arrays offs / lens: ((offs0, lens0, index0), (offs1, lens1, index1), classes)"""
    n = len(offs)
    d_offs, d_lens = ctx.to_device(offs if n else np.zeros(1, np.int64)), ctx.to_device(lens if n else np.zeros(1, np.uint32))
    d_index = None if index is None else ctx.to_device(np.ascontiguousarray(index, np.uint32))
    a, b, cls = ctx.split_sequences(seed, seq0, n, threshold, d_offs, d_lens, index=d_index, want_class=True)
    out = []
    for o, l, i, k in (a, b):
        assert k <= n
        out.append((o.to_host()[:k], l.to_host()[:k], i.to_host()[:k]))
    return out[0], out[1], cls.to_host()[:n]


def check_split(ctx, seed, seq0, offs, lens, threshold, index=None):
    got0, got1, cls = run_split(ctx, seed, seq0, offs, lens, threshold, index)
    want = mh.classes(seed, seq0, len(offs), threshold, index)
    assert np.array_equal(cls, want)
    for got, c in ((got0, 0), (got1, 1)):
        idx = np.flatnonzero(want == c)
        assert len(got[2]) == len(idx)
        assert np.array_equal(got[2], idx.astype(np.uint32))
        assert np.array_equal(got[0], offs[idx]) and np.array_equal(got[1], lens[idx])
    return got0, got1


def test_symbols():
    for name in ("pengk_split_sequences", "pengk_holdout_summary"):
        assert hasattr(pk.lib(), name)


@pytest.mark.parametrize("threshold", THRESHOLDS)
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_split_small_sizes(ctx, arrays, n, threshold):
    offs, lens = arrays
    check_split(ctx, 5, 0, offs[:n], lens[:n], threshold)


@pytest.mark.parametrize("threshold", THRESHOLDS + [mh.threshold_of(0.1)])
def test_split_many_tiles(ctx, arrays, threshold):
    offs, lens = arrays
    assert BIG > 3 * TILE and BIG % TILE
    _, hold = check_split(ctx, 1, 0, offs, lens, threshold)
    if threshold == mh.threshold_of(0.1):
        assert 9000 < len(hold[2]) < 11000


@pytest.mark.parametrize("k", [1000, 2 * TILE + 100, 3 * TILE], ids=["mid_wave", "mid_tile", "tile_edge"])
def test_split_of_two_shards_is_the_split_of_the_whole(ctx, arrays, k):
    offs, lens = arrays
    n = 4 * TILE + 77
    assert k % 64 or k % TILE == 0
    t = mh.threshold_of(0.3)
    whole = check_split(ctx, 9, 0, offs[:n], lens[:n], t)
    first = check_split(ctx, 9, 0, offs[:k], lens[:k], t)
    second = check_split(ctx, 9, k, offs[k:n], lens[k:n], t)
    for c in (0, 1):
        assert np.array_equal(np.concatenate([first[c][0], second[c][0]]), whole[c][0])
        assert np.array_equal(np.concatenate([first[c][1], second[c][1]]), whole[c][1])
        assert np.array_equal(np.concatenate([first[c][2], second[c][2] + np.uint32(k)]), whole[c][2])


def test_split_at_the_top_of_the_index_range(ctx, arrays):
    offs, lens = arrays
    n = TILE + 300
    check_split(ctx, 3, 2 ** 32 - n, offs[:n], lens[:n], 2 ** 31)


def test_split_through_an_index_list(ctx, arrays):
    """a strided subset of a file: classes by the file's indices, places and written indices by the subset's"""
    offs, lens = arrays
    idx = np.arange(3, 3 + 7 * (2 * TILE + 500), 7, dtype=np.uint32)
    sub0, sub1 = check_split(ctx, 4, 100, offs[idx], lens[idx], 2 ** 31, index=idx)
    whole = mh.classes(4, 100, int(idx[-1]) + 1, 2 ** 31)
    assert np.array_equal(idx[sub1[2]], idx[whole[idx] == 1]) and np.array_equal(idx[sub0[2]], idx[whole[idx] == 0])


def test_split_argument_errors_write_nothing(ctx, arrays):
    offs, lens = arrays
    n = 300
    d_offs, d_lens = ctx.to_device(offs[:n]), ctx.to_device(lens[:n])
    C = pk.C
    mark64, mark32 = np.full(n, -7, np.int64), np.full(n, 0xABCDEF01, np.uint32)
    outs = [ctx.to_device(mark64), ctx.to_device(mark32), ctx.to_device(mark32), ctx.to_device(mark64), ctx.to_device(mark32),
            ctx.to_device(mark32)]
    cls = ctx.to_device(np.full(n, 9, np.uint8))

    def call(seq0, n_seq, threshold, o=None, offs_in=d_offs, lens_in=d_lens, index=None):
        o = o or outs
        n0, n1 = C.c_uint64(77), C.c_uint64(78)
        rc = pk.lib().pengk_split_sequences(ctx.h, 1, seq0, n_seq, threshold, index, offs_in.ptr, lens_in.ptr, cls.ptr, o[0].ptr,
                                            o[1].ptr, o[2].ptr, C.byref(n0), o[3].ptr, o[4].ptr, o[5].ptr, C.byref(n1))
        return rc, n0.value, n1.value

    bad = [call(2 ** 32 - n + 1, n, 5), call(2 ** 32 + 1, 0, 5), call(0, 2 ** 32 + 1, 5), call(0, n, 2 ** 32 + 1),
           call(0, n, 5, o=[d_offs] + outs[1:]), call(0, n, 5, o=outs[:4] + [d_lens] + outs[5:]),
           call(0, n, 5, o=outs[:2] + [d_lens] + outs[3:]), call(0, n, 5, index=outs[5].ptr)]
    for rc, n0, n1 in bad:
        assert (rc, n0, n1) == (pk.ERR_ARG, 77, 78)
    ctx.synchronize()
    for o, m in zip(outs, [mark64, mark32, mark32, mark64, mark32, mark32]):
        assert np.array_equal(o.to_host(), m)
    assert (cls.to_host() == 9).all()
    assert np.array_equal(d_offs.to_host(), offs[:n]) and np.array_equal(d_lens.to_host(), lens[:n])
    assert call(2 ** 32 - n, n, 5)[0] == 0  # (the same call within the range)


# ---- the consumers ---------------------------------------------------------------------------------------------------------
def mixed_sequences(seed, n, W):
    """sequences shorter than W, at the word edges and longer, every third with invalid bases"""
    rng = np.random.default_rng(seed)
    lens = [0, 1, W - 1, W, 31, 32, 33, 64, 65] + rng.integers(0, 150, n - 9).tolist()
    seqs = [rng.integers(1, 5, L).astype(np.uint8) for L in lens]
    for c in seqs[9::3]:
        if len(c):
            c[rng.integers(0, len(c), 2)] = 0
    order = rng.permutation(n)
    return [seqs[i] for i in order]


@pytest.mark.parametrize("W", [4, 10])
def test_pack_of_the_training_pair_is_the_host_pack_of_those_sequences(ctx, W):
    seqs = mixed_sequences(30 + W, 2 * TILE + 345, W)
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    t = mh.threshold_of(0.25)
    (o0, l0, i0, n0), (o1, l1, i1, n1), _ = ctx.split_sequences(2, 0, len(seqs), t, scan[2], scan[3])
    want0, want1 = mh.split(2, 0, len(seqs), t)
    assert (n0, n1) == (len(want0), len(want1)) and n1 > 400
    for o, l, n, want in ((o0, l0, n0, want0), (o1, l1, n1, want1)):
        host = pk.Packed(*ms.flatten([seqs[i] for i in want]), W, 64)
        words, items, st = ctx.pack_scan((scan[0], scan[1], o, l, n), W, 64)
        assert (st.n_words, st.n_items) == (len(host.words), len(host.items))
        assert np.array_equal(words.to_host(), host.words)
        assert np.array_equal(items.to_host()[:st.n_items], host.items)
        assert (st.n_bases, st.n_windows, st.max_bin_bound, st.all_whole, st.n_sequences, st.max_len) == \
            (host.n_bases, host.n_windows, host.max_bin_bound, host.all_whole, host.n_sequences, host.max_len)


@pytest.mark.parametrize("both", [False, True], ids=["plus", "both"])
def test_enrich_over_the_two_pairs_adds_up_to_the_whole(ctx, both):
    rng = np.random.default_rng(41)
    seqs = mixed_sequences(40, TILE + 500, 6)
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    Ss = [me.word_S("ACG"), rng.integers(-300, 301, (6, 4)).astype(np.int32), rng.integers(-300, 301, (13, 4)).astype(np.int32)]
    lens = [len(S) for S in Ss]
    hi = [me.score_range(S)[1] for S in Ss]
    thr = [h - 500 for h in hi]
    whole, scored = ctx.motif_enrich(scan, Ss, lens, both, thr, hi)
    (o0, l0, _, n0), (o1, l1, _, n1), _ = ctx.split_sequences(6, 0, len(seqs), mh.threshold_of(0.4), scan[2], scan[3])
    assert n0 > 500 and n1 > 500
    h0, s0 = ctx.motif_enrich((scan[0], scan[1], o0, l0, n0), Ss, lens, both, thr, hi)
    h1, s1 = ctx.motif_enrich((scan[0], scan[1], o1, l1, n1), Ss, lens, both, thr, hi)
    assert int(scored.sum()) > 0 and sum(int(h.sum()) for h in whole) > 0
    assert np.array_equal(s0 + s1, scored)
    for m in range(len(Ss)):
        assert np.array_equal(h0[m] + h1[m], whole[m])
