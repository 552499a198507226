"""--erase on the device (include/pengk.h, "erasing sites and packing on the device"): pengk_mask_sites against the numpy
model of tests/motif_erase_model.py -- the output validity words bit for bit, the site and erased counts exact, at the
chunk-table edges, the word edges, across motif groups and across workgroups -- and pengk_pack_scan_sizes /
pengk_pack_scan against the host packer, bit for bit, on the cases tests/test_motif_erase_cpu.py holds the host packer
to; then the count of a masked, device-packed set against the oracle's count of the masked codes."""
import numpy as np
import pytest

import peng_motif_amd as pk
import motif_erase_model as me
import motif_score_model as ms
from oracle import oracle as po

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = pk.Context(0)
    yield c
    c.close()


def random_S(rng, w):
    S = rng.integers(-300, 301, (w, 4)).astype(np.int32)
    S[rng.random((w, 4)) < 0.05] = -2000
    return S


def check_mask(ctx, seqs, Ss, ts, both, all_valid=False):
    """the device's mask of the sequences against the model's; all_valid: the input validity is not given (the sequences
    must then hold no invalid base)"""
    lay = pk.ScanLayout(*ms.flatten(seqs))
    scan = ctx.upload_scan(lay)
    lens = [len(S) for S in Ss]
    out, sites, erased = ctx.mask_sites(scan, Ss, lens, both, ts, all_valid=all_valid)
    masked, n, e = me.mask(seqs, Ss, ts, both)
    got = out.to_host()
    want = me.valid_words(masked)
    assert np.array_equal(got[:len(want)], want)
    assert np.array_equal(sites.to_host()[:len(Ss)], n)
    assert int(erased.to_host()[0]) == e
    if Ss and seqs and not all_valid:  # the cross-check: the row sums of pengk_sites_count on the same arguments
        rows = ctx.sites_count(scan, Ss, lens, both, ts).to_host()[:len(Ss), :len(seqs)].sum(axis=1)
        assert np.array_equal(rows.astype(np.uint64), n)
    return e


# ---- the mask ------------------------------------------------------------------------------------------------------------
def test_symbols():
    for name in ("pengk_mask_sites", "pengk_pack_scan_sizes", "pengk_pack_scan"):
        assert hasattr(pk.lib(), name)


@pytest.mark.parametrize("case", me.mask_cases(), ids=lambda c: c["name"])
def test_mask_constructed_cases(ctx, case):
    check_mask(ctx, case["seqs"], case["Ss"], case["ts"], case["both"])


@pytest.mark.parametrize("both", [False, True])
def test_mask_widths_and_lengths(ctx, both):
    """widths at the chunk-table edges, lengths at the word edges, invalid bases; thresholds at which about one window
    strand in ten is a site, so that covers merge, stand apart and cross words"""
    rng = np.random.default_rng(5)
    erased = 0
    for w in (1, 4, 5, 8, 9, 64):
        lens = [0, w - 1, w, 31, 32, 33, 64, 65] + rng.integers(0, 200, 40).tolist()
        seqs = [rng.integers(1, 5, L).astype(np.uint8) for L in lens]
        for c in seqs[8::2]:
            if len(c):
                c[rng.integers(0, len(c), 2)] = 0
        S = random_S(rng, w)
        lo, hi = me.score_range(S)
        # a threshold from the scores themselves: the 90th percentile of the + strand's window scores
        b = np.concatenate([np.where((c >= 1) & (c <= 4), c - 1, 0) for c in seqs if len(c) >= w])
        win = np.lib.stride_tricks.sliding_window_view(b, w)
        t = int(np.percentile(np.asarray(S, np.int64)[np.arange(w)[None, :], win].sum(axis=1), 90))
        assert lo <= t <= hi
        erased += check_mask(ctx, seqs, [S], [t], both)
    assert erased > 0


def test_mask_without_input_validity(ctx):
    rng = np.random.default_rng(6)
    seqs = [rng.integers(1, 5, L).astype(np.uint8) for L in [0, 3, 31, 32, 33, 64, 65, 97] + rng.integers(0, 150, 30).tolist()]
    S = [me.word_S("AC"), random_S(rng, 9)]
    assert check_mask(ctx, seqs, S, [200, 150], True, all_valid=True) > 0


def test_mask_41_motifs_two_groups(ctx):
    rng = np.random.default_rng(7)
    words = ["".join("ACGT"[x] for x in rng.integers(0, 4, 4)) for _ in range(41)]
    assert me.groups([4] * 41, False) == [0] * 40 + [1]
    seqs = [rng.integers(1, 5, L).astype(np.uint8) for L in rng.integers(20, 120, 50).tolist()]
    seqs[3][7] = 0
    assert check_mask(ctx, seqs, [me.word_S(x) for x in words], [400] * 41, False) > 0
    assert check_mask(ctx, seqs, [me.word_S(x) for x in words], [400] * 41, True) > 0


def test_mask_600_sequences(ctx):
    """more sequences than a workgroup holds and a last workgroup partly filled; several motifs per group"""
    rng = np.random.default_rng(8)
    seqs = [rng.integers(1, 5, L).astype(np.uint8) for L in rng.integers(0, 90, 600).tolist()]
    for c in seqs[::7]:
        if len(c):
            c[rng.integers(0, len(c))] = 0
    Ss = [me.word_S("ACG"), me.word_S("TTGCA"), random_S(rng, 12)]
    assert check_mask(ctx, seqs, Ss, [300, 500, 400], True) > 0


def test_mask_no_motif_and_no_sequence(ctx):
    rng = np.random.default_rng(9)
    seqs = [rng.integers(0, 5, L).astype(np.uint8) for L in (10, 40, 64)]
    check_mask(ctx, seqs, [], [], True)   # the input validity, copied
    check_mask(ctx, [], [me.word_S("ACGT")], [400], True)


def test_mask_argument_errors(ctx):
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten([np.ones(40, np.uint8)])))
    with pytest.raises(pk.PengkError) as e:
        ctx.mask_sites(scan, [me.word_S("ACGT")], [4], True, [400], out_valid=scan[1])
    assert e.value.code == pk.ERR_ARG
    with pytest.raises(pk.PengkError) as e:
        ctx.mask_sites(scan, [np.full((4, 4), 2001, np.int32)], [4], True, [400])
    assert e.value.code == pk.ERR_ARG
    with pytest.raises(pk.PengkError) as e:
        ctx.mask_sites(scan, [np.zeros((4, 4), np.int32)], [0], True, [400])
    assert e.value.code == pk.ERR_ARG


# ---- the packer ------------------------------------------------------------------------------------------------------------
def check_pack(ctx, seqs, W, M, name=""):
    host = pk.Packed(*ms.flatten(seqs), W, M)
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    words, items, st = ctx.pack_scan(scan, W, M)
    assert (st.n_words, st.n_items) == (len(host.words), len(host.items)), name
    assert np.array_equal(words.to_host(), host.words), name
    assert np.array_equal(items.to_host()[:st.n_items], host.items), name
    got = (st.n_bases, st.n_windows, st.max_bin_bound, st.all_whole, st.n_sequences, st.max_len, st.W, st.item_windows)
    assert got == (host.n_bases, host.n_windows, host.max_bin_bound, host.all_whole, host.n_sequences, host.max_len, host.W,
                   host.item_windows), name


@pytest.mark.parametrize("W", [4, 10, 14])
def test_pack_constructed_cases(ctx, W):
    for name, seqs, M in me.pack_cases(W):
        check_pack(ctx, seqs, W, M, name)


def test_pack_100000_sequences(ctx):
    """more sequences than a tile of the prefix sums holds, whole and cut ones mixed"""
    rng = np.random.default_rng(10)
    codes = rng.integers(1, 5, 100000 * 40).astype(np.uint8)
    codes[rng.integers(0, len(codes), 20000)] = 0
    seqs = list(codes.reshape(100000, 40))
    check_pack(ctx, seqs, 10, 0)
    check_pack(ctx, list(np.maximum(codes, 1).reshape(100000, 40)), 10, 64)  # every sequence whole: all_whole = 1


def test_pack_without_input_validity(ctx):
    rng = np.random.default_rng(11)
    seqs = [rng.integers(1, 5, L).astype(np.uint8) for L in (3, 10, 33, 64, 300)]
    host = pk.Packed(*ms.flatten(seqs), 10, 64)
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    words, items, st = ctx.pack_scan(scan, 10, 64, all_valid=True)
    assert np.array_equal(words.to_host(), host.words) and np.array_equal(items.to_host()[:st.n_items], host.items)


def test_pack_argument_errors(ctx):
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten([np.ones(40, np.uint8)])))
    for W, M in ((9, 0), (16, 0), (10, 63), (10, 65536)):
        with pytest.raises(pk.PengkError) as e:
            ctx.pack_scan(scan, W, M)
        assert e.value.code == pk.ERR_ARG


# ---- mask, pack, count -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [8, 10])
def test_count_after_mask_and_pack(ctx, W):
    seqs = me.planted(1, n=600)
    seqs[5][50] = 0
    S = ms.log_odds(me.consensus_pwm("TGACTCAGCA"), np.full(4, 0.25, np.float32))
    t = me.score_range(S)[1] - 600
    masked, n, erased = me.mask(seqs, [S], [t], True)
    assert erased > 1000
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    out, sites, er = ctx.mask_sites(scan, [S], [len(S)], True, [t])
    assert int(er.to_host()[0]) == erased
    _, _, st = ctx.pack_scan(scan, W, valid=out, attach=True)
    for both in (False, True):
        counts, ltot = ctx.count(both)
        if both:
            ctx.mirror(W, counts)
        want, lt = po.count(*ms.flatten(masked), W, both)
        assert int(ltot.to_host()[0]) == lt == st.n_windows
        got = counts.to_host().astype(np.uint64)
        assert np.array_equal(got, want)
