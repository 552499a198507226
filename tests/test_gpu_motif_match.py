"""The control matching on the device (include/pengk.h, "a control set matched to the input"): pengk_seq_strata and
pengk_select_strata against the numpy model of tests/motif_match_model.py, bit for bit -- the strata at the length-bin,
word and GC-bin edges, with and without validity words, across workgroups; the selection on constructed stratum arrays at
the tile edges, beyond one part of the tile scan, with every stratum present, over shards; then the scans over the
selected offsets against the models' values on the selected sequences."""
import ctypes as C

import numpy as np
import pytest

import peng_motif_amd as pk
import motif_enrich_model as me
import motif_match_model as mm
import motif_score_model as ms

pytestmark = pytest.mark.gpu

TILE = 2048          # sequences per workgroup of the selection (csrc/match.hip: SEL_TILE)
PART = 2048 * TILE   # ... and per pass of the scan over the tiles' sums


@pytest.fixture(scope="module")
def ctx():
    c = pk.Context(0)
    yield c
    c.close()


def test_symbols():
    for name in ("pengk_seq_strata", "pengk_match_quotas", "pengk_select_strata"):
        assert hasattr(pk.lib(), name)


# ---- strata ------------------------------------------------------------------------------------------------------------------
def check_strata(ctx, seqs, G, use_length, all_valid=False, prefill=None):
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    hist = None if prefill is None else ctx.to_device(prefill)
    s, h = ctx.seq_strata(scan, G, use_length, all_valid=all_valid, hist=hist)
    ws, wh = mm.strata(seqs, G, use_length, all_valid)
    got = s.to_host()[:len(seqs)]
    assert got.dtype == np.uint16 and np.array_equal(got, ws), np.flatnonzero(got != ws)[:10]
    assert np.array_equal(h.to_host(), wh + (0 if prefill is None else prefill))
    return ws


EDGE_LENGTHS = [0, 1, 31, 32, 33, 47, 48, 63, 64, 95, 96, 6143, 6144, 70000]


@pytest.mark.parametrize("use_length", [0, 1])
@pytest.mark.parametrize("G", [1, 2, 10, 16])
def test_strata_at_the_length_and_word_edges(ctx, G, use_length):
    rng = np.random.default_rng(10 * G + use_length)
    seqs = [rng.integers(1, 5, L).astype(np.uint8) for L in EDGE_LENGTHS]
    seqs += [np.zeros(L, np.uint8) for L in (1, 32, 33, 100)]  # invalid bases only
    for L in (33, 64, 65, 97):  # invalid bases at the word edges
        c = rng.integers(1, 5, L).astype(np.uint8)
        c[[0, 31, 32, L - 1]] = 0
        seqs.append(c)
    seqs += [rng.integers(0, 5, L).astype(np.uint8) for L in rng.integers(1, 300, 60)]
    s = check_strata(ctx, seqs, G, use_length)
    assert (s[1:len(EDGE_LENGTHS)] // G).tolist() == ([0, 0, 0, 0, 0, 1, 1, 2, 2, 3, 14, 15, 15] if use_length else [0] * 13)
    assert s[0] == mm.NONE and np.all(s[14:18] == mm.NONE)


@pytest.mark.parametrize("G", [1, 2, 10, 16])
def test_gc_share_exactly_on_every_bin_edge(ctx, G):
    """gc * G an exact multiple of n: n = 16 * G valid bases of which 16 k are C or G, k = 0 .. G, among invalid bases
    that the share must not count; a base fewer stays in the bin below"""
    seqs = []
    for k in range(G + 1):
        for less in (0, 1):
            gc = max(16 * k - less, 0)
            c = np.array([2, 3] * (gc // 2) + [2] * (gc % 2) + [1] * (16 * G - gc) + [0] * 7, np.uint8)
            seqs.append(np.random.default_rng(k).permutation(c))
    s = check_strata(ctx, seqs, G, 0)
    assert s[::2].tolist() == [min(k, G - 1) for k in range(G + 1)]
    assert s[1::2].tolist() == [min(max(k - 1, 0), G - 1) for k in range(G + 1)]


def test_strata_without_validity_words_and_added_to_a_filled_histogram(ctx):
    rng = np.random.default_rng(7)
    seqs = [rng.integers(0, 5, L).astype(np.uint8) for L in EDGE_LENGTHS[:11] + rng.integers(1, 200, 50).tolist()]
    check_strata(ctx, seqs, 10, 1, all_valid=True)
    check_strata(ctx, seqs, 10, 1, prefill=rng.integers(0, 2 ** 40, 256).astype(np.uint64))


def test_strata_of_200000_short_sequences(ctx):
    rng = np.random.default_rng(8)
    lens = rng.integers(20, 110, 200000)
    N = int(lens.sum())
    p = np.repeat(rng.random(200000), lens)  # every sequence with a GC share of its own, 2 % of the other bases invalid
    flat = np.where(rng.random(N) < p, rng.integers(2, 4, N), rng.choice([1, 4, 0], N, p=[0.49, 0.49, 0.02])).astype(np.uint8)
    seqs = np.split(flat, np.cumsum(lens)[:-1])
    s = check_strata(ctx, seqs, 10, 1)
    assert len(np.unique(s)) >= 30


def test_strata_arguments(ctx):
    seqs = [np.array([1, 2, 3, 4], np.uint8)]
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    for kw in (dict(gc_bins=0), dict(gc_bins=17), dict(use_length=2), dict(n_seq=2 ** 32)):
        with pytest.raises(pk.PengkError) as e:
            ctx.seq_strata(scan, **kw)
        assert e.value.code == pk.ERR_ARG and "pengk_seq_strata" in str(e.value)
    prefill = np.arange(256, dtype=np.uint64)
    s, h = ctx.seq_strata(scan, n_seq=0, hist=ctx.to_device(prefill))  # nothing happens
    assert np.array_equal(h.to_host(), prefill)


# ---- select ------------------------------------------------------------------------------------------------------------------
def run_select(ctx, s, count, quota, rank0=None):
    """the device's kept indices of the stratum array s, after checking its offsets and lengths against them"""
    n = len(s)
    offs = (np.arange(n, dtype=np.int64) * 7 + 3) * 32
    lens = (np.arange(n, dtype=np.uint64) * 2654435761 % 1000).astype(np.uint32)
    r0 = np.zeros(256, np.uint64) if rank0 is None else rank0
    so, sl, si, k = ctx.select_strata(ctx.to_device(s), n, count, quota, r0, ctx.to_device(offs), ctx.to_device(lens))
    idx = si.to_host()[:k].astype(np.int64)
    assert np.array_equal(so.to_host()[:k], offs[idx]) and np.array_equal(sl.to_host()[:k], lens[idx])
    return idx


def check_select(ctx, s, quota, count=None):
    s = np.ascontiguousarray(s, np.uint16)
    count = mm.histogram(s) if count is None else count
    got = run_select(ctx, s, count, quota)
    want = mm.select(s, count, quota)
    assert np.array_equal(got, want), (len(got), len(want))
    return want


@pytest.mark.parametrize("c", [1, 2, 63, 64, 65, 1000])
def test_one_stratum_at_the_quota_edges(ctx, c):
    s = np.full(c, 37, np.uint16)
    for q in sorted({0, 1, c - 1, c}):
        quota = np.zeros(256, np.uint64)
        quota[37] = q
        assert len(check_select(ctx, s, quota)) == q


def test_all_256_strata_and_unassigned_entries(ctx):
    rng = np.random.default_rng(11)
    s = rng.integers(0, 256, 20000).astype(np.uint16)
    s[rng.random(20000) < 0.05] = mm.NONE
    s[:300] = mm.NONE  # whole waves without a stratum
    count = mm.histogram(s)
    assert np.all(count > 0)
    quota = (count * rng.random(256)).astype(np.uint64)
    quota[0], quota[255], quota[100] = count[0], count[255], 0
    sel = check_select(ctx, s, quota)
    assert np.array_equal(mm.histogram(s[sel]), quota)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 511, 512, 513, TILE - 1, TILE, TILE + 1, 3 * TILE + 77])
def test_sizes_at_the_wave_and_tile_edges(ctx, n):
    rng = np.random.default_rng(n)
    s = rng.choice([0, 3, 9, 200, 255, mm.NONE], n).astype(np.uint16)
    count = mm.histogram(s)
    check_select(ctx, s, (count * 2) // 3)
    check_select(ctx, np.sort(s), count // 2)  # long runs of one stratum: every lane of a wave in one group


def test_beyond_one_part_of_the_tile_scan(ctx):
    n = PART + TILE + 5
    rng = np.random.default_rng(12)
    s = rng.choice([1, 17, mm.NONE], n, p=[0.7, 0.2, 0.1]).astype(np.uint16)
    count = mm.histogram(s)
    quota = np.zeros(256, np.uint64)
    quota[1], quota[17] = count[1] // 3, count[17] - 1
    sel = check_select(ctx, s, quota)
    assert sel[-1] > PART  # kept sequences behind the first part


def test_300000_sequences_in_three_shards(ctx):
    rng = np.random.default_rng(13)
    n = 300000
    s = rng.integers(0, 160, n).astype(np.uint16)
    s[rng.random(n) < 0.01] = mm.NONE
    count = mm.histogram(s)
    quota = (count * rng.random(256)).astype(np.uint64)
    one = check_select(ctx, s, quota)
    assert np.array_equal(mm.histogram(s[one]), quota)
    got = []
    for a, b in ((0, 99999), (99999, 100000 + TILE), (100000 + TILE, n)):
        got.append(a + run_select(ctx, np.ascontiguousarray(s[a:b]), count, quota, rank0=mm.histogram(s[:a])))
    assert np.array_equal(np.concatenate(got), one)


def test_select_arguments(ctx):
    s = np.array([1, 1, 2], np.uint16)
    count = mm.histogram(s)
    ok = run_select(ctx, s, count, count)
    assert ok.tolist() == [0, 1, 2]
    d = ctx.to_device(s)
    z = np.zeros(256, np.uint64)
    bufs = [ctx.empty(4, np.int64), ctx.empty(4, np.uint32)]
    over = count.copy()
    over[2] += 1
    for cnt, quota, rank0, n in ((count, over, z, 3), (count, count, over, 3), (count, count, z, 2 ** 32),
                                 (count + np.uint64(2 ** 32), count, z, 3)):
        k = C.c_uint64(99)
        rc = pk.lib().pengk_select_strata(ctx.h, d.ptr, n, cnt.ctypes.data, quota.ctypes.data, rank0.ctypes.data, bufs[0].ptr,
                                          bufs[1].ptr, bufs[0].ptr, bufs[1].ptr, bufs[1].ptr, C.byref(k))
        assert rc == pk.ERR_ARG and b"pengk_select_strata" in pk.lib().pengk_last_error()
    so, sl, si, k = ctx.select_strata(d, 0, count, count, z, bufs[0], bufs[1])  # nothing happens
    assert k == 0


# ---- together ----------------------------------------------------------------------------------------------------------------
def test_scans_over_the_selected_offsets_equal_the_models_on_the_selected_sequences(ctx):
    pos, ctrl = mm.scenario(5, 300, 1500)
    rng = np.random.default_rng(14)
    for c in ctrl[::7]:
        c[rng.integers(0, len(c), 3)] = 0
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(ctrl)))
    s_in, h_in = ctx.seq_strata(ctx.upload_scan(pk.ScanLayout(*ms.flatten(pos))))
    s_ctrl, h_ctrl = ctx.seq_strata(scan)
    h_in, h_ctrl = h_in.to_host(), h_ctrl.to_host()
    assert np.array_equal(h_in, mm.strata(pos)[1]) and np.array_equal(h_ctrl, mm.strata(ctrl)[1])
    quota, short = pk.match_quotas(h_in, h_ctrl, 2)
    so, sl, si, k = ctx.select_strata(s_ctrl, len(ctrl), h_ctrl, quota, np.zeros(256, np.uint64), scan[2], scan[3])
    want = mm.select(mm.strata(ctrl)[0], h_ctrl, quota)
    assert 0 < k == len(want) < len(ctrl) and np.array_equal(si.to_host()[:k], want)
    kept = [ctrl[i] for i in want]
    sub = (scan[0], scan[1], so, sl, k)  # a subset of a scan layout: shorter offs / lens into the same words
    S = ms.log_odds(mm.word_pwm(mm.GC_RICH_8MER), np.full(4, 0.25, np.float32))
    for both in (False, True):
        best = ctx.motif_scan(sub, [S], [len(S)], both).to_host()
        assert np.array_equal(best[0, :k], ms.best_scores(kept, S, both))
        thr, hi = int(np.percentile(ms.best_scores(kept, S, both), 60)), me.score_hi(S)
        hists, scored = ctx.motif_enrich(sub, [S], [len(S)], both, [thr], [hi])
        wh, wn = me.histogram(me.best_scores(me.Packed(kept), S, both), thr, hi)
        assert np.array_equal(hists[0], wh) and int(scored[0]) == wn == k
