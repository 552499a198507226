"""The sequence-scan kernels of csrc/score.hip, csrc/sites.hip and csrc/site_stats.hip (scan, sampler, synthetic generator, histograms, sites and their
exclusive scan, best sites, centrality histograms, site profiles) compared value by value at the sizes the per-feature
modules (test_gpu_motif_score / _sites / _centrality / _refine) only sum over: more sequences than one trip of a
grid-stride loop, more scan elements than one pass of xscan_parts_kernel, many blocks and slices of
pengk_sites_slices, sequences far beyond 2^16 bases, histogram bins on both sides of the LDS split, more motifs than one
LDS group.  The large set is modelled by tests/scan_batch_model.py (pinned to the per-sequence models by
tests/test_scan_batch_model_cpu.py); the small sets by the per-sequence models themselves.  Every comparison is equality
of arrays over ALL sequences, and every test asserts from the model or from the device's num_cu that it reached the path
it is there for.  A new scan kernel belongs here: add its comparison on the `big` set instead of a new random_seqs."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import peng_motif_amd as pk
import motif_centrality_model as mc
import motif_refine_model as mr
import motif_score_model as ms
import motif_sites_model as mst
import scan_batch_model as sbm
from oracle import oracle as po
from test_gpu_motif_centrality import sub_scan
from test_gpu_motif_score import random_V
from test_gpu_motif_sites import random_S, random_seqs, thresholds

pytestmark = pytest.mark.gpu

SCAN_THREADS, XS_TILE, HIST_LDS_BINS, SCAN_TABLES = 256, 2048, 16384, 40  # csrc/scan_walk.h, csrc/sites.hip, csrc/score.hip
CLASSES = np.array([20, 31, 32, 33, 47, 65])
CLASS_P = [0.2, 0.2, 0.2, 0.2, 0.15, 0.05]
BIG_SEQ0 = 2 ** 40 + 987654321  # GOLDEN * (g + 1) wraps many times over
WORKERS = 8


@pytest.fixture(scope="module")
def ctx():
    c = pk.Context(0)
    yield c
    c.close()


def pmap(fn, items):
    """numpy releases the GIL in its inner loops: the motifs' models run side by side"""
    with ThreadPoolExecutor(WORKERS) as ex:
        return list(ex.map(fn, items))


class Big:
    """the large set: n a little above two trips of the scan kernels' grid-stride loop, short sequences of six length
    classes in a random order, 1 % of the bases invalid; behind every trip boundary and among the last 256 indices
    sequences shorter than the narrowest motif (w = 4) and sequences without any valid window"""

    def __init__(self, num_cu):
        self.trip = trip = num_cu * 8 * SCAN_THREADS
        self.n = n = 2 * trip + trip // 8 + 77
        rng = np.random.default_rng(20240607)
        lens = CLASSES[rng.choice(len(CLASSES), n, p=CLASS_P)]
        self.short = [trip, 2 * trip + 1, n - 1, n - 100, n - 200]
        self.no_window = [trip + 1, 2 * trip, n - 2, n - 77, n - 255]
        lens[self.short] = [3, 3, 1, 0, 2]
        self.lens = lens
        self.offs = offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        codes = rng.integers(1, 5, int(offs[-1]), dtype=np.uint8)
        codes[rng.integers(0, 100, len(codes), dtype=np.uint8) == 0] = 0
        for k, i in enumerate(self.no_window):
            codes[offs[i]:offs[i + 1]:(1 if k % 2 else 3)] = 0  # all N, or every third base
        self.codes = codes
        self.codes_a = np.where(codes == 0, 1, codes).astype(np.uint8)  # d_valid = NULL: another letter is stored as A
        mrng = np.random.default_rng(77)
        self.S = [random_S(mrng, 4), random_S(mrng, 10), random_S(mrng, 13),
                  mrng.integers(-2000, 2001, (20, 4)).astype(np.int32),  # a score range of several LDS histograms
                  random_S(mrng, 33), np.zeros((6, 4), np.int32), mrng.integers(0, 2, (13, 4)).astype(np.int32),
                  random_S(mrng, 60)]
        self.widths = [len(s) for s in self.S]
        self.thr = thresholds(self.S, np.full(4, 0.25, np.float32), 0.02)  # (the all-zero motif: 1, no site)
        self._model = {}

    def model(self, kind):
        """the batched model of every motif: "both" (sites at thr and best sites at seq0 = 0 with it), "all_valid" (best
        scores of the all-valid copy), "seq0" (best sites under BIG_SEQ0)"""
        if kind not in self._model:
            def one(m):
                if kind == "both":
                    return sbm.scan_mixed(self.codes, self.offs, self.S[m], True, thr=self.thr[m], m=m, seq0=0)
                if kind == "all_valid":
                    return sbm.scan_mixed(self.codes_a, self.offs, self.S[m], True)
                return sbm.scan_mixed(self.codes, self.offs, self.S[m], True, m=m, seq0=BIG_SEQ0)
            self._model[kind] = pmap(one, range(len(self.S)))
        return self._model[kind]

    def stack(self, kind, key):
        return np.stack([r[key] for r in self.model(kind)])


@pytest.fixture(scope="module")
def big(ctx):
    b = Big(ctx.info("num_cu"))
    b.layout = pk.ScanLayout(b.codes, b.offs)
    b.scan = ctx.upload_scan(b.layout)
    return b


def test_the_big_set_is_what_the_paths_need(ctx, big):
    num_cu, n = ctx.info("num_cu"), big.n
    assert n > 2 * num_cu * 8 * SCAN_THREADS and n > num_cu * 16 * 256  # a second and a third trip; the sampler's second
    assert n % 256 and n % 2048 and n % 4096
    assert len(big.S) * n > XS_TILE * XS_TILE  # xscan_parts_kernel loops and carries
    assert n > 16 * pk.SITES_BLOCK and n >= 4096  # many site blocks; the LDS histogram paths
    assert min(big.widths) > max(big.lens[big.short]) and np.all(big.lens[big.no_window] >= min(big.widths))
    for i in big.short + big.no_window:  # right behind a trip boundary, or among the last 256
        assert min(i % big.trip, n - 1 - i) < 256
    best = big.stack("both", "best")
    assert np.all(best[:, big.short + big.no_window] == ms.SENTINEL)
    assert np.all((best[0] > ms.SENTINEL).sum() == n - len(big.short) - len(big.no_window))
    assert 0.005 < (big.codes == 0).mean() < 0.02


# ---- 1. pengk_motif_scan ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("both", [True, False], ids=["both", "plus"])
def test_best_scores_of_every_sequence(ctx, big, both):
    key = "best" if both else "best_plus"
    got = ctx.motif_scan(big.scan, big.S, big.widths, both).to_host()
    assert np.array_equal(got, big.stack("both", key))
    got = ctx.motif_scan(big.scan, big.S, big.widths, both, all_valid=True).to_host()
    want = big.stack("all_valid", key)
    assert np.array_equal(got, want)
    assert np.count_nonzero(want != big.stack("both", key)) > big.n // 100  # (the invalid bases matter)


# ---- 2. pengk_score_histograms ---------------------------------------------------------------------------------------
def test_score_histograms_on_both_sides_of_the_lds_split(ctx, big):
    want_best = big.stack("both", "best")
    best = ctx.motif_scan(big.scan, big.S, big.widths, True)
    assert np.array_equal(best.to_host(), want_best)
    lo, hi = zip(*[ms.score_range(s) for s in big.S])
    want = [ms.histogram(want_best[m], lo[m], hi[m]) for m in range(len(big.S))]
    nb = [hi[m] - lo[m] + 2 for m in range(len(big.S))]
    assert big.n >= 256 * 16  # the LDS path
    assert nb[3] > HIST_LDS_BINS and want[3][1:nb[3] - HIST_LDS_BINS].sum() > 1000 and want[3][nb[3] - HIST_LDS_BINS:].sum() > 1000
    assert any(x <= HIST_LDS_BINS for x in nb) and all(int(w[0]) >= len(big.short) + len(big.no_window) for w in want)
    hist, offs = ctx.score_histograms(best, big.n, lo, hi)
    hist = hist.to_host()
    for m in range(len(big.S)):
        assert np.array_equal(hist[offs[m]:offs[m + 1]], want[m]), m
    # a second call adds
    d = ctx.to_device(hist)
    ctx.score_histograms(best, big.n, lo, hi, hist=d)
    assert np.array_equal(d.to_host(), 2 * hist)


# ---- 3. pengk_sample_background --------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 0])
def test_sampled_negatives_of_every_sequence(ctx, big, K):
    assert big.n > ctx.info("num_cu") * 16 * 256
    seed, seq0 = 2 ** 63 + 11, 3_000_000_000
    th = ms.thresholds(random_V(np.random.default_rng(5 + K)), K)
    got = ctx.sample_background(big.scan, seed, seq0, K, th).to_host()
    neg = np.concatenate(ms.sample(big.lens, seed, seq0, K, th)) + np.uint8(1)
    want = pk.ScanLayout(neg, big.offs)
    assert np.array_equal(want.offs, big.layout.offs) and len(got) == len(want.words)
    assert np.array_equal(got, want.words)


# ---- 4. pengk_sites_count / _slices / _emit --------------------------------------------------------------------------
def model_records(big, sites=None):
    """per motif: the model's records as pengk_site with the GLOBAL sequence in an int64 array beside them"""
    out = []
    for m, r in enumerate(big.model("both") if sites is None else sites):
        s = r["sites"]
        rec = np.zeros(len(s), pk.SITE)
        rec["pos"], rec["score"], rec["motif_strand"] = s["pos"], s["score"], 2 * m + s["strand"].astype(np.uint32)
        out.append((s["seq"].copy(), rec))
    return out


def slice_records(records, i0, i1):
    """the raw buffer of slice [i0, i1): motif, then sequence, then position, + before -"""
    parts = []
    for seq, rec in records:
        a, b = np.searchsorted(seq, [i0, i1])
        r = rec[a:b].copy()
        r["seq"] = seq[a:b] - i0
        parts.append(r)
    return np.concatenate(parts)


def check_slices(bounds, recs, n, budget, seq_totals):
    """the header's contract, and h_records against the model's sums"""
    assert int(bounds[0]) == 0 and int(bounds[-1]) == n and np.all(np.diff(bounds.astype(np.int64)) > 0)
    csum = np.concatenate([[0], np.cumsum(seq_totals)])
    assert np.array_equal(recs.astype(np.int64), csum[bounds[1:].astype(np.int64)] - csum[bounds[:-1].astype(np.int64)])
    assert np.all((recs <= budget) | (np.diff(bounds.astype(np.int64)) == 1))


def test_one_slice_through_the_multi_pass_scan(ctx, big):
    nm, n = len(big.S), big.n
    want_counts = big.stack("both", "counts")
    total = int(want_counts.sum())
    assert nm * n > XS_TILE * XS_TILE and 2 * 10 ** 6 < total < 2 ** 24  # one slice under the default budget
    counts = ctx.sites_count(big.scan, big.S, big.widths, True, big.thr)
    assert np.array_equal(counts.to_host(), want_counts.astype(np.uint64))
    bounds, recs, tot = ctx.sites_slices(counts, n, nm)
    assert bounds.tolist() == [0, n] and recs.tolist() == [total]
    assert tot.tolist() == want_counts.sum(axis=1).tolist() and min(t for m, t in enumerate(tot.tolist()) if m != 5) > 1000
    got = ctx.sites_records(big.scan, big.S, big.widths, True, big.thr, counts, 0, n, total)
    want = slice_records(model_records(big), 0, n)
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("which", ["whole_blocks", "cut_blocks"])
def test_budgets_that_cut_slices(big, which):
    nm, n = len(big.S), big.n
    want_counts = big.stack("both", "counts")
    seq_tot = want_counts.sum(axis=0)
    nblk = (n + pk.SITES_BLOCK - 1) // pk.SITES_BLOCK
    blk = np.add.reduceat(seq_tot, np.arange(nblk) * pk.SITES_BLOCK)
    typical = int(np.median(blk))
    # a little above a typical block total: slices of whole blocks; well below it: every block is cut between sequences
    budget = typical + typical // 8 if which == "whole_blocks" else typical // 3
    assert nblk > 16 and int(seq_tot.sum()) > 16 * budget and budget > seq_tot.max()
    if which == "whole_blocks":
        assert np.count_nonzero(blk <= budget) > nblk // 2
    else:
        assert np.all(blk[:-1] > budget)
    records = model_records(big)
    c = pk.Context(0)
    try:
        c.set_option("sites_record_budget", budget)
        scan = c.upload_scan(big.layout)
        counts = c.sites_count(scan, big.S, big.widths, True, big.thr)
        bounds, recs, tot = c.sites_slices(counts, n, nm)
        assert tot.tolist() == want_counts.sum(axis=1).tolist()
        assert len(recs) > 16
        check_slices(bounds, recs, n, budget, seq_tot)
        at_block = np.count_nonzero(bounds[1:-1] % np.uint64(pk.SITES_BLOCK) == 0)
        assert at_block > len(recs) // 2 if which == "whole_blocks" else at_block < len(recs) // 2
        buf = c.empty(int(recs.max()) * pk.SITE.itemsize, np.uint8)
        for k in range(len(recs)):
            i0, i1 = int(bounds[k]), int(bounds[k + 1])
            got = c.sites_records(scan, big.S, big.widths, True, big.thr, counts, i0, i1, int(recs[k]), buf)
            assert got.tobytes() == slice_records(records, i0, i1).tobytes(), (k, i0, i1)
    finally:
        c.close()


def test_a_budget_of_one_and_too_small_slice_arrays(big):
    """a prefix of a few blocks under a budget of 1 (one launch per slice), then max_slices below the count"""
    nm, n = len(big.S), 2 * pk.SITES_BLOCK + 333
    seq_tot = big.stack("both", "counts")[:, :n].sum(axis=0)
    records = [(seq[:np.searchsorted(seq, n)], rec[:np.searchsorted(seq, n)]) for seq, rec in model_records(big)]
    c = pk.Context(0)
    try:
        c.set_option("sites_record_budget", 1)
        full = c.upload_scan(big.layout)  # (kept: sub_scan borrows its arrays)
        scan = sub_scan(full, 0, n)
        counts = c.sites_count(scan, big.S, big.widths, True, big.thr)
        bounds, recs, tot = c.sites_slices(counts, n, nm)
        assert tot.tolist() == [len(seq) for seq, _ in records]
        # the model's slices: a sequence with records closes the slice before it unless it starts one
        assert len(recs) > pk.SITES_BLOCK and np.count_nonzero(seq_tot > 1) > 1000
        check_slices(bounds, recs, n, 1, seq_tot)
        buf = c.empty(int(recs.max()) * pk.SITE.itemsize, np.uint8)
        for k in range(len(recs)):
            i0, i1 = int(bounds[k]), int(bounds[k + 1])
            got = c.sites_records(scan, big.S, big.widths, True, big.thr, counts, i0, i1, int(recs[k]), buf)
            assert got.tobytes() == slice_records(records, i0, i1).tobytes(), (k, i0, i1)
        # max_slices 0 and 1: the full count comes back, only the first entries are written
        MARK = np.uint64(0xABCDABCDABCDABCD)
        for max_slices in [0, 1]:
            hb, hr = np.full(4, MARK), np.full(4, MARK)
            t2, ns = np.zeros(nm, np.uint64), C.c_uint64()
            pk._check(pk.lib().pengk_sites_slices(c.h, counts.ptr, n, nm, t2.ctypes.data, max_slices, hb.ctypes.data,
                                                  hr.ctypes.data, C.byref(ns)))
            assert ns.value == len(recs) and t2.tolist() == tot.tolist()
            assert hb[:max_slices + 1].tolist() == (bounds[:2].tolist() if max_slices else [int(MARK)])
            assert hr[:max_slices].tolist() == recs[:max_slices].tolist()
            assert np.all(hb[max_slices + 1 if max_slices else 0:] == MARK) and np.all(hr[max_slices:] == MARK)
    finally:
        c.close()


# ---- 5. pengk_motif_best_sites, pengk_centrality_histograms ----------------------------------------------------------
def low_thresholds(best):
    return [int(np.percentile(b[b > ms.SENTINEL], 30)) for b in best]


def test_best_sites_of_every_sequence(ctx, big):
    for kind, seq0 in [("both", 0), ("seq0", BIG_SEQ0)]:
        best, site = ctx.motif_best_sites(big.scan, big.S, big.widths, True, seq0=seq0)
        assert best.to_host().tobytes() == big.stack(kind, "best_site").tobytes(), kind
        assert site.to_host().tobytes() == big.stack(kind, "site").tobytes(), kind
    a, b = big.stack("both", "site"), big.stack("seq0", "site")
    assert np.array_equal(big.stack("both", "best_site"), big.stack("seq0", "best_site"))
    for m, share in [(5, 2), (6, 10)]:  # the tie-heavy motifs: the key chooses, and another seq0 chooses otherwise
        assert np.count_nonzero(a[m] > 1) > big.n // 2 and np.count_nonzero(a[m] != b[m]) > big.n // share


def test_centrality_histograms_over_mixed_lengths(ctx, big):
    wb, ws = big.stack("both", "best_site"), big.stack("both", "site")
    best, site = ctx.to_device(wb), ctx.to_device(ws)
    thr = low_thresholds(wb)
    sums = []
    for max_len in [int(CLASSES.max()), 40]:  # the longest class is counted; 47 and 65 are left out
        assert 3 * max_len + 2 <= 16384 and big.n >= 4096  # the LDS path
        hd, hl = ctx.centrality_histograms(best, site, big.scan[3], big.n, big.widths, thr, max_len)
        hd, hl = hd.to_host(), hl.to_host()
        for m, w in enumerate(big.widths):
            wd, wl = mc.histograms(wb[m], ws[m], big.lens, w, thr[m], max_len)
            assert hd[m].tobytes() == wd.tobytes() and hl[m].tobytes() == wl.tobytes(), (max_len, m)
        wl0 = mc.histograms(wb[0], ws[0], big.lens, 4, thr[0], max_len)[1]
        sums.append(int(wl0.sum()))
        assert wl0[min(max_len, 65)] > 1000 if max_len == 65 else (wl0[33] > 1000 and wl0[20] > 1000)
        assert np.count_nonzero(mc.histograms(wb[0], ws[0], big.lens, 4, thr[0], max_len)[0]) > max_len  # both parities
    assert sums[1] < sums[0] - 10000


# ---- 6. pengk_site_profiles ------------------------------------------------------------------------------------------
def test_site_profiles_of_every_sequence(ctx, big):
    wb, ws = big.stack("both", "best_site"), big.stack("both", "site")
    best, site = ctx.to_device(wb), ctx.to_device(ws)
    thr = low_thresholds(wb)
    flanks = [0, 3, 40]
    assert pk.clamp_flank(60, 40) == 2 and big.widths[7] == 60
    jobs = [(m, f) for f in flanks for m in range(len(big.S))]
    model = dict(zip(jobs, pmap(lambda j: sbm.site_profile_mixed(big.codes, big.offs, wb[j[0]], ws[j[0]], big.widths[j[0]],
                                                                 thr[j[0]], j[1]), jobs)))
    for f in flanks:
        got = ctx.site_profiles(big.scan, best, site, big.widths, thr, f).to_host()
        want = np.stack([model[(m, f)] for m in range(len(big.S))])
        assert got.tobytes() == want.tobytes(), f
        assert want[7].any() and want[:, 0].sum() > big.n
    # two halves of the set, each scanned under its own seq0, add up to one call
    k = big.trip + 1001
    c = None
    for i0, i1 in [(0, k), (k, big.n)]:
        part = sub_scan(big.scan, i0, i1)
        b, s = ctx.motif_best_sites(part, big.S, big.widths, True, seq0=i0)
        c = ctx.site_profiles(part, b, s, big.widths, thr, 3, counts=c)
    assert c.to_host().tobytes() == np.stack([model[(m, 3)] for m in range(len(big.S))]).tobytes()


# ---- 7. long sequences -------------------------------------------------------------------------------------------------
LONG_WIDTHS = [1, 10, 33, 64]


def make_long_set():
    rng = np.random.default_rng(4242)
    lens = [4096, 65535, 65536, 65537, 70001, 200003, 300, 64, 65, 1000, 131077, 33]
    seqs = [rng.integers(1, 5, L).astype(np.uint8) for L in lens]
    S = [random_S(rng, w) for w in LONG_WIDTHS]
    for i in [0, 4]:
        seqs[i][3:9] = 0  # an N run near the start
    for i in [3, 4, 10]:
        seqs[i][65530:65546] = 0  # across the word boundary at 2^16
    seqs[4][65600] = 0
    seqs[4][-5:] = 0  # at the very end
    seqs[10][131072 - 70:131072 + 3] = 0
    seqs[1][-1] = 0
    # planted: the best window of motif 1 (w = 10) in the last window of the longest sequence, that of motif 2 (w = 33)
    # in the first window of the 65 536-base one
    seqs[5][-10:] = np.argmax(S[1], axis=1) + 1
    seqs[2][:33] = np.argmax(S[2], axis=1) + 1
    return seqs, S


@pytest.fixture(scope="module")
def long_set():
    return make_long_set()


def test_long_sequences_best_scores_and_sites(ctx, long_set):
    seqs, S = long_set
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    for both in [True, False]:
        got = ctx.motif_scan(scan, S, LONG_WIDTHS, both).to_host()
        for m in range(len(S)):
            assert np.array_equal(got[m].astype(np.int64), ms.best_scores(seqs, S[m], both)), (both, m)
    bg = np.full(4, 0.25, np.float32)
    thr = thresholds(S, bg, 0.04)
    thr[0] = int(S[0].max())  # (w = 1: the best base only)
    want = mst.all_sites(seqs, S, thr, True)
    per_seq = np.bincount(want["seq"].astype(np.int64), minlength=len(seqs))
    budget = 5000
    assert per_seq[5] > 20000 and np.count_nonzero(per_seq > budget) >= 5  # tens of thousands from one sequence
    assert int(want["pos"].max()) == 200003 - 1 and np.count_nonzero(want["pos"] > 65535) > 10000
    got, tot = ctx.motif_sites(scan, S, LONG_WIDTHS, True, thr)
    assert got.tobytes() == want.tobytes()
    assert tot.tolist() == np.bincount(want["motif"], minlength=len(S)).tolist()
    c = pk.Context(0)
    try:  # a budget below one sequence's records: such a sequence is a slice of its own
        c.set_option("sites_record_budget", budget)
        scan2 = c.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
        counts = c.sites_count(scan2, S, LONG_WIDTHS, True, thr)
        bounds, recs, _ = c.sites_slices(counts, len(seqs), len(S))
        check_slices(bounds, recs, len(seqs), budget, per_seq)
        for i in np.nonzero(per_seq > budget)[0]:
            assert i in bounds.tolist() and i + 1 in bounds.tolist()
        got, _ = c.motif_sites(scan2, S, LONG_WIDTHS, True, thr)
        assert got.tobytes() == want.tobytes()
    finally:
        c.close()


def test_long_sequences_best_sites_centrality_and_profiles(ctx, long_set):
    seqs, S = long_set
    lens = np.array([len(c) for c in seqs])
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    best, site = ctx.motif_best_sites(scan, S, LONG_WIDTHS, True, seq0=7)
    gb, gs = best.to_host(), site.to_host()
    model = [mc.best_sites(seqs, S[m], True, m, 7) for m in range(len(S))]
    wb, ws = np.stack([b for b, _ in model]), np.stack([s for _, s in model])
    assert int(ws[1, 5]) == 2 * (200003 - 10) and int(ws[2, 2]) == 0  # the planted sites: p > 65535, p = 0
    assert np.count_nonzero((ws >> np.uint64(1)) > 65535) >= 4
    assert gb.tobytes() == wb.tobytes() and gs.tobytes() == ws.tobytes()
    thr = [int(b[b > ms.SENTINEL].min()) for b in wb]
    for max_len in [pk.CENTRALITY_MAX_LEN, 65535]:  # 65 536 counted or not; 65 537 and longer never
        assert 3 * max_len + 2 > 16384  # the global bins
        hd, hl = ctx.centrality_histograms(best, site, scan[3], len(seqs), LONG_WIDTHS, thr, max_len)
        hd, hl = hd.to_host(), hl.to_host()
        for m, w in enumerate(LONG_WIDTHS):
            wd, wl = mc.histograms(wb[m], ws[m], lens, w, thr[m], max_len)
            assert hd[m].tobytes() == wd.tobytes() and hl[m].tobytes() == wl.tobytes(), (max_len, m)
            assert int(wl.sum()) == int(((lens >= w) & (lens <= max_len)).sum())
            assert int(wl[65536:].sum()) == (1 if max_len == 65536 else 0) and wl[65535] == 1
    for flank in [0, 8, 40]:
        got = ctx.site_profiles(scan, best, site, LONG_WIDTHS, thr, flank).to_host()
        want = np.stack([mr.site_profile(seqs, wb[m], ws[m], w, thr[m], flank) for m, w in enumerate(LONG_WIDTHS)])
        assert got.tobytes() == want.tobytes(), flank
        if flank:  # the planted sites at both ends: the flank columns outside the sequence fall in bin 4
            F = pk.clamp_flank(33, flank)
            assert want[2, 0, 4] >= 1 and want[1, 10 + 2 * pk.clamp_flank(10, flank) - 1, 4] >= 1 and F >= 1


# ---- 8. pengk_synth_scan_sequences -----------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [7, 2 ** 63 + 99])
@pytest.mark.parametrize("L", [9, 10, 31, 32, 33, 200])
def test_synthetic_scan_sequences_equal_the_cpu_generator(ctx, L, seed):
    stride = ctx.info("num_cu") * 16 * 256  # the generator's threads: one word each
    n = stride // ((L + 31) // 32) + 1001 if (L == 200 and seed == 7) or L == 33 else 5003
    if L in (33, 200) and seed == 7:
        assert n * ((L + 31) // 32) > stride
    seq0 = 123456789
    words, valid, offs, lens, _ = ctx.synth_scan(seed, seq0, n, L)
    codes, coffs = po.synth(seed, seq0, n, L)
    want = pk.ScanLayout(codes, coffs)
    assert np.array_equal(words.to_host(), want.words) and np.array_equal(valid.to_host(), want.valid)
    assert np.array_equal(offs.to_host(), want.offs) and np.array_equal(lens.to_host(), want.lens)
    word = np.array(["ACGT".index(ch) + 1 for ch in "GCTGAGTCAT"], np.uint8)
    if L >= 10:
        hits = sum(int(np.all(codes.reshape(n, L)[:, p:p + 10] == word, axis=1).sum()) for p in range(L - 9))
        assert n // 20 < hits < n // 5  # every tenth sequence is planted


# ---- 9. motif groups ---------------------------------------------------------------------------------------------------
def group_cases():
    rng = np.random.default_rng(909)
    out = []
    for nm in [41, 80, 100]:  # one table each on the + strand: 40 fill a group exactly
        widths = (rng.integers(1, 5, nm)).tolist()
        out.append(("plus%d" % nm, [random_S(rng, w) for w in widths], widths, False))
    widths = [64, 64, 17, 1, 64]  # both strands: 32 tables, then a motif that no longer fits
    out.append(("both_wide", [random_S(rng, w) for w in widths], widths, True))
    return out


@pytest.mark.parametrize("case", group_cases(), ids=lambda c: c[0])
def test_motif_groups(ctx, case):
    _, S, widths, both = case
    tables = [(w + 3) // 4 * (2 if both else 1) for w in widths]
    assert sum(tables) > SCAN_TABLES  # more than one group
    if not both:
        assert len(S) > SCAN_TABLES and sum(tables[:SCAN_TABLES]) == SCAN_TABLES  # a group filled exactly, then more records
    else:
        assert tables[0] == 32 and tables[1] + tables[2] > SCAN_TABLES >= tables[2] + tables[3]  # 32 tables, then one that no longer fits
    rng = np.random.default_rng(len(S))
    seqs = [c for _ in range(4) for c in random_seqs(rng)]
    assert len(seqs) > 250
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    got = ctx.motif_scan(scan, S, widths, both).to_host()
    want = np.stack([ms.best_scores(seqs, s, both) for s in S])
    assert np.array_equal(got.astype(np.int64), want)
    # distinct thresholds: one staged at another motif's record shows
    thr = []
    for b in want:
        t = int(np.percentile(b[b > ms.SENTINEL], 40))
        while t in thr:
            t -= 5
        thr.append(t)
    sites, tot = ctx.motif_sites(scan, S, widths, both, thr)
    wsites = mst.all_sites(seqs, S, thr, both)
    assert sites.tobytes() == wsites.tobytes() and len(wsites) > 50 * len(S)
    assert tot.tolist() == np.bincount(wsites["motif"], minlength=len(S)).tolist()
    best, site = ctx.motif_best_sites(scan, S, widths, both, seq0=3)
    model = [mc.best_sites(seqs, s, both, m, 3) for m, s in enumerate(S)]
    assert best.to_host().tobytes() == np.stack([b for b, _ in model]).tobytes()
    assert site.to_host().tobytes() == np.stack([s for _, s in model]).tobytes()
