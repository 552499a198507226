"""Motif pair spacing on the device (--spacing; include/pengk.h, "motif pair spacing") against the numpy model of
tests/motif_spacing_model.py.  The kernel's inputs are the best-site arrays, so most cases upload constructed arrays and
compare the three histograms byte for byte: every orientation, gap edge and overlap, every reason a site does not count,
the pair index up to 64 motifs, the sizes around a wave and a block, the LDS and the global bins, contention on one bin,
accumulation and splits.  Then planted pairs through the real best-site scan, and the CLI's TSV against the model, beside
the other outputs, with a sequence above the length limit and over several ranks."""
import json
import os

import numpy as np
import pytest

import peng_motif_amd as pk
import motif_centrality_model as mc
import motif_score_model as ms
import motif_sites_model as mst
import motif_spacing_model as sp
from oracle import oracle as po
from test_gpu_multirank import run_plain, run_ranks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
# The bins live in LDS when a pair's 4 (G + 1) + 2 + max_len + 1 bins number at most 16000 and the call has at least
# LDS_MIN_SEQ sequences; otherwise in global memory.
LDS_MIN_SEQ = 16384
# (s_a, s_b, side) -> orientation class, written out: side 0 = b to the right of a in + coordinates
CLASS_OF = {(0, 0, 0): 0, (0, 0, 1): 1, (0, 1, 0): 2, (0, 1, 1): 3, (1, 0, 0): 3, (1, 0, 1): 2, (1, 1, 0): 1, (1, 1, 1): 0}


@pytest.fixture(scope="module")
def ctx():
    c = pk.Context(0)
    yield c
    c.close()


def device_hists(ctx, best, site, lens, widths, thr, G, min_len, max_len, into=None):
    """the three histograms (host) of host arrays best / site (n_motifs x n_seq) and lens"""
    best = np.ascontiguousarray(best, np.int32).reshape(len(widths), -1)
    site = np.ascontiguousarray(site, np.uint64).reshape(len(widths), -1)
    n_seq = best.shape[1]
    d = [ctx.to_device(best), ctx.to_device(site), ctx.to_device(np.ascontiguousarray(lens, np.uint32))]
    out = ctx.spacing_histograms(d[0], d[1], d[2], n_seq, widths, thr, G, min_len, max_len, *(into or ()))
    ctx.synchronize()  # (the inputs are freed on return)
    return out


def assert_equals_model(ctx, best, site, lens, widths, thr, G, min_len, max_len, tag=None):
    dev = device_hists(ctx, best, site, lens, widths, thr, G, min_len, max_len)
    want = sp.histograms(best, site, lens, widths, thr, G, min_len, max_len)
    for name, g, w in zip(("gaps", "lengths", "motifs"), dev, want):
        assert g.to_host().tobytes() == w.tobytes(), (name, tag)
    return want


def configurations(wa, wb, G):
    """(L, p_a, s_a, p_b, s_b, bin, apart) of every orientation at the gaps around G, and the overlaps"""
    out = []
    G1 = G + 1
    for (sa, sb, side), c in CLASS_OF.items():
        for g in sorted({0, 1, G - 1, G, G + 1} - {-1}):
            for off in (0, 3):
                pa, pb = (off, off + wa + g) if side == 0 else (off + wb + g, off)
                L = wa + wb + g + off + (0 if off == 0 else 2)  # (off = 0: the right site ends the sequence)
                out.append((L, pa, sa, pb, sb, c * G1 + g if g <= G else 4 * G1 + 1, True))
    short, long_ = min(wa, wb), max(wa, wb)
    for sa in (0, 1):
        for sb in (0, 1):
            L = wa + wb + 4
            out.append((L, 2, sa, 2 + wa - 1, sb, 4 * G1, False))        # a's last base is b's first
            out.append((L, 2 + wb - 1, sa, 2, sb, 4 * G1, False))        # b's last base is a's first
            out.append((L, 2, sa, 2, sb, 4 * G1, False))                 # the same start
            pl, ps = 2, 2 + (long_ - short) // 2                         # the short one inside the long one
            out.append((L, pl if wa == long_ else ps, sa, ps if wa == long_ else pl, sb, 4 * G1, False))
    # a sequence too short to hold both side by side: overlap is the only outcome
    out.append((wa + wb - 1, 0, 0, wa - 1, 1, 4 * G1, False))
    return out


@pytest.mark.parametrize("G", [0, 1, 150, 1024])
@pytest.mark.parametrize("wa,wb", [(1, 1), (3, 8), (64, 64), (10, 64)])
def test_every_configuration(ctx, wa, wb, G):
    cfg = configurations(wa, wb, G)
    min_len = max(wa, wb)
    cfg = [c for c in cfg if c[0] >= min_len]
    lens = np.array([c[0] for c in cfg])
    max_len = int(lens.max())
    site = np.array([[2 * c[1] + c[2] for c in cfg], [2 * c[3] + c[4] for c in cfg]], np.uint64)
    best = np.zeros(site.shape, np.int32)
    # the expected bins, from the table above
    B = sp.n_bins(G)
    hg = np.zeros(B, np.uint64)
    hl = np.zeros(max_len + 1, np.uint64)
    for L, _, _, _, _, b, apart in cfg:
        hg[b] += 1
        if apart:
            hl[L] += 1
    want = assert_equals_model(ctx, best, site, lens, [wa, wb], [0, 0], G, min_len, max_len)  # (global bins: a small call)
    assert want[0][0].tobytes() == hg.tobytes() and want[1][0].tobytes() == hl.tobytes()
    assert want[2].tolist() == [len(cfg), len(cfg)]
    # the same sequences many times over: LDS bins (at G = 1024 a pair has about 5300 of them)
    k = LDS_MIN_SEQ // len(cfg) + 1
    dev = device_hists(ctx, np.tile(best, k), np.tile(site, k), np.tile(lens, k), [wa, wb], [0, 0], G, min_len, max_len)
    assert dev[0].to_host()[0].tobytes() == (hg * np.uint64(k)).tobytes()
    assert dev[1].to_host()[0].tobytes() == (hl * np.uint64(k)).tobytes()
    assert dev[2].to_host().tolist() == [k * len(cfg)] * 2


@pytest.mark.parametrize("copies", [1, 1200], ids=["global", "lds"])
def test_every_exclusion(ctx, copies):
    wa, wb, ta, tb, G = 5, 7, 10, -20, 30
    min_len, max_len = 9, 60
    S = mc.SENTINEL
    # (L, best_a, p_a, best_b, p_b): a has a site?, b has a site?
    cases = [
        (40, ta, 3, tb, 20, True, True),
        (40, S, 0, tb, 20, False, True),          # no window at all
        (40, ta - 1, 3, tb, 20, False, True),     # one below the threshold
        (40, ta, 3, tb - 1, 20, True, False),
        (40, ta + 500, 3, S, 0, True, False),
        (40, ta, 35, tb, 33, True, True),         # both in their last window (they overlap)
        (40, ta, 36, tb, 33, False, True),        # a window that is not one of this sequence
        (40, ta, 0, tb, 34, True, False),
        (min_len - 1, ta, 0, tb, 0, False, False),  # a sequence too short to be considered, whatever it holds
        (min_len, ta, 0, tb, 2, True, True),      # (shorter than w_a + w_b: the two can only overlap)
        (11, ta, 6, tb, 0, True, True),           # L = w_a + w_b - 1: the outermost windows still share a base
        (12, ta, 7, tb, 0, True, True),           # L = w_a + w_b: apart at gap 0, b to the left
        (max_len, ta, 0, tb, max_len - wb, True, True),  # far: gap 48 > G
        (max_len + 1, ta, 0, tb, 20, False, False),
        (max_len + 1000, ta, 0, tb, 20, False, False),
    ]
    lens = np.array([c[0] for c in cases] * copies)
    best = np.array([[c[1] for c in cases] * copies, [c[3] for c in cases] * copies], np.int32)
    site = np.array([[2 * c[2] for c in cases] * copies, [2 * c[4] + 1 for c in cases] * copies], np.uint64)
    hg, hl, hm = assert_equals_model(ctx, best, site, lens, [wa, wb], [ta, tb], G, min_len, max_len, copies)
    assert hm.tolist() == [copies * sum(c[5] for c in cases), copies * sum(c[6] for c in cases)]
    G1 = G + 1
    assert int(hg[0].sum()) == copies * sum(c[5] and c[6] for c in cases) == copies * 6
    assert int(hg[0][4 * G1]) == 3 * copies and int(hg[0][4 * G1 + 1]) == copies  # overlapping; far
    assert int(hg[0][2 * G1 + 12]) == copies  # a + at 3, b - at 20: opposite_downstream, gap 12
    assert int(hg[0][3 * G1 + 0]) == copies   # a + at 7, b - at 0: opposite_upstream, gap 0
    assert int(hl[0][40]) == copies and int(hl[0][12]) == copies and int(hl[0][max_len]) == copies and int(hl[0].sum()) == 3 * copies
    # thresholds above every score (hi + 1 of a motif of these widths): nothing counts
    dev = device_hists(ctx, best, site, lens, [wa, wb], [2000 * wa + 1, 2000 * wb + 1], G, min_len, max_len)
    assert not any(h.to_host().any() for h in dev)


def random_sites(rng, n_motifs, n_seq, widths, max_L, share=0.6):
    """random best / site / lens: sites inside and (a few) outside their sequence, scores around the threshold 0"""
    lens = rng.integers(0, max_L + 1, n_seq)
    best = rng.integers(-2, 3, (n_motifs, n_seq)).astype(np.int32)
    best[rng.random(best.shape) > share] = -5
    best[rng.random(best.shape) < 0.03] = mc.SENTINEL
    site = np.zeros((n_motifs, n_seq), np.uint64)
    for m in range(n_motifs):
        room = np.maximum(lens - widths[m] + 2, 1)  # (one window past the last: skipped)
        site[m] = 2 * (rng.random(n_seq) * room).astype(np.int64) + rng.integers(0, 2, n_seq)
    return best, site, lens


@pytest.mark.parametrize("n_motifs", [1, 2, 3, 17, 64])
def test_motif_counts_and_the_pair_index(ctx, n_motifs):
    rng = np.random.default_rng(100 + n_motifs)
    widths = rng.integers(1, 13, n_motifs).tolist()
    best, site, lens = random_sites(rng, n_motifs, 300, widths, 90)
    thr = rng.integers(-1, 2, n_motifs).tolist()
    hg, hl, hm = assert_equals_model(ctx, best, site, lens, widths, thr, 20, max(widths), 80, n_motifs)
    assert hm.sum() > 30 * n_motifs
    if n_motifs == 1:
        # no pair: the other two arrays are not needed at all
        d = [ctx.to_device(best), ctx.to_device(site), ctx.to_device(lens.astype(np.uint32)), ctx.to_device(np.zeros(1, np.uint64))]
        w, t = np.array(widths, np.int32), np.array(thr, np.int32)
        pk._check(pk.lib().pengk_spacing_histograms(ctx.h, 1, d[0].ptr, d[1].ptr, d[2].ptr, 300, w.ctypes.data, t.ctypes.data, 20,
                                                    max(widths), 80, None, None, d[3].ptr))
        assert d[3].to_host().tolist() == hm.tolist()
        return
    assert hg.sum() > 10 * (n_motifs - 1)
    # one sequence in which only motifs 1 and n - 1 have a site: the pair's row and no other
    b = n_motifs - 1
    a = min(1, b - 1)
    best1 = np.full((n_motifs, 1), mc.SENTINEL, np.int32)
    best1[[a, b], 0] = 5
    site1 = np.zeros((n_motifs, 1), np.uint64)
    site1[b, 0] = 2 * (widths[a] + 4)
    dev = device_hists(ctx, best1, site1, [70], widths, [0] * n_motifs, 20, max(widths), 80)
    g, l = dev[0].to_host(), dev[1].to_host()
    q = b * (b - 1) // 2 + a
    assert g.shape[0] == n_motifs * (n_motifs - 1) // 2
    if n_motifs == 64:
        assert g.shape[0] == 2016 and q == 1954  # (63 * 62 / 2 + 1)
    assert g[q][4] == 1 and g.sum() == 1 and l[q][70] == 1 and l.sum() == 1  # same_downstream, gap 4


def test_bad_arguments_are_refused(ctx):
    rng = np.random.default_rng(7)

    def call(n_motifs=2, widths=None, G=20, min_len=12, max_len=80):
        widths = widths or [12] * n_motifs
        best, site, lens = random_sites(rng, n_motifs, 50, widths, 60)
        return device_hists(ctx, best, site, lens, widths, [0] * n_motifs, G, min_len, max_len)

    call()
    for kw, word in [(dict(n_motifs=65), "65 motifs"), (dict(G=1025), "max_gap 1025"), (dict(max_len=0), "max_len 0"),
                     (dict(max_len=65537), "max_len 65537"), (dict(widths=[12, 0]), "width 0"), (dict(widths=[65, 3], min_len=65), "width 65"),
                     (dict(min_len=11), "min_len 11")]:
        with pytest.raises(pk.PengkError) as e:
            call(**kw)
        assert e.value.code == pk.ERR_ARG and "pengk_spacing_histograms" in str(e.value) and word in str(e.value), kw
    call(n_motifs=64, G=1024, widths=[64] * 64, min_len=64)  # the limits themselves
    call(max_len=65536)


# around a wave (64), the centrality kernels' block (256), this kernel's block (1024) and the first call with LDS bins
@pytest.mark.parametrize("n_seq", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, LDS_MIN_SEQ - 1, LDS_MIN_SEQ, LDS_MIN_SEQ + 1])
def test_sizes(ctx, n_seq):
    rng = np.random.default_rng(n_seq)
    widths = [4, 9, 6]
    best, site, lens = random_sites(rng, 3, n_seq, widths, 70, share=0.9)
    hg, hl, hm = assert_equals_model(ctx, best, site, lens, widths, [0, -1, 1], 12, 9, 64, n_seq)
    if n_seq >= 63:
        assert hg.sum() > n_seq // 4


# LDS bins: 20000 sequences and max_len = 120 (exact) or 200, at G = 150 (5 pairs' bins fit: one row per motif) and at
# G = 1024 (3 pairs' bins fit: the fifth motif has two rows).  Global bins: max_len = 40000 (a pair's bins do not fit),
# and 300 sequences whatever the rest.
@pytest.mark.parametrize("n_seq", [300, 20000])
@pytest.mark.parametrize("G", [150, 1024])
@pytest.mark.parametrize("max_len", [120, 200, 40000])
def test_both_paths(ctx, max_len, G, n_seq):
    rng = np.random.default_rng(G + n_seq)
    widths = [10, 3, 12, 8, 5]
    best, site, lens = random_sites(rng, 5, n_seq, widths, 120, share=0.8)
    lens[::97] = 40000  # (considered only under max_len = 40000)
    site[:, ::97] = 2 * (39000 + 20 * np.arange(5, dtype=np.uint64))[:, None]  # (apart from each other)
    hg, hl, hm = assert_equals_model(ctx, best, site, lens, widths, [0] * 5, G, 12, max_len, (max_len, G, n_seq))
    assert hg.sum() > n_seq and hl.shape[1] == max_len + 1
    if max_len == 40000:
        assert hl[:, 40000].sum() > 0


@pytest.fixture(scope="module")
def synth(ctx):
    """200 000 synthetic sequences of 200 bases, four motifs through the real best-site scan, thresholds at the median:
    many blocks, LDS bins and one hot length bin"""
    n, L = 200000, 200
    scan = ctx.synth_scan(3, 0, n, L)
    rng = np.random.default_rng(61)
    widths = [10, 12, 14, 1]
    S = [rng.integers(-300, 301, (w, 4)).astype(np.int32) for w in widths[:3]] + [np.zeros((1, 4), np.int32)]
    best, site = ctx.motif_best_sites(scan, S, widths, True)
    gb, gs = best.to_host(), site.to_host()
    thr = [int(np.median(gb[m])) for m in range(4)]
    return dict(n=n, L=L, scan=scan, widths=widths, best=best, site=site, gb=gb, gs=gs, thr=thr, lens=np.full(n, L))


def test_many_blocks_equal_the_model_and_accumulate(ctx, synth):
    s = synth
    n, L, G = s["n"], s["L"], 150
    dev = ctx.spacing_histograms(s["best"], s["site"], s["scan"][3], n, s["widths"], s["thr"], G, 14, L)
    want = sp.histograms(s["gb"], s["gs"], s["lens"], s["widths"], s["thr"], G, 14, L)
    for g, w in zip(dev, want):
        assert g.to_host().tobytes() == w.tobytes()
    assert all(int(x) > n // 3 for x in want[2]) and int(want[1][:, L].sum()) == int(want[1].sum()) > n // 2
    # a second call adds the same again
    ctx.spacing_histograms(s["best"], s["site"], s["scan"][3], n, s["widths"], s["thr"], G, 14, L, *dev)
    for g, w in zip(dev, want):
        assert g.to_host().tobytes() == (w * np.uint64(2)).tobytes()


def test_every_sequence_in_one_bin(ctx, synth):
    s = synth
    n, L, G = s["n"], s["L"], 150
    # every site of motif m at 40 m on +: pair (a, b) at gap 40 (b - a) - w_a, same_downstream
    gs = np.repeat((2 * 40 * np.arange(4, dtype=np.uint64))[:, None], n, axis=1)
    dev = device_hists(ctx, s["gb"], gs, s["lens"], s["widths"], s["thr"], G, 14, L)
    hg, hl, hm = [d.to_host() for d in dev]
    has = [s["gb"][m] >= s["thr"][m] for m in range(4)]
    for b in range(1, 4):
        for a in range(b):
            q = b * (b - 1) // 2 + a
            k = int((has[a] & has[b]).sum())
            assert k > n // 8
            g = 40 * (b - a) - s["widths"][a]
            assert int(hg[q][g]) == k == int(hg[q].sum()) and int(hl[q][L]) == k == int(hl[q].sum()), (a, b)
    assert hm.tolist() == [int(h.sum()) for h in has]


@pytest.mark.parametrize("k", [1, 29, -1])
def test_split_records_sum_to_the_whole(ctx, synth, k):
    s = synth
    n, L, G = s["n"], s["L"], 150
    k = k % n
    into = None
    for lo, hi in [(0, k), (k, n)]:
        into = device_hists(ctx, s["gb"][:, lo:hi], s["gs"][:, lo:hi], s["lens"][lo:hi], s["widths"], s["thr"], G, 14, L, into)
    want = sp.histograms(s["gb"], s["gs"], s["lens"], s["widths"], s["thr"], G, 14, L)
    for g, w in zip(into, want):
        assert g.to_host().tobytes() == w.tobytes()


MOTIF_A, MOTIF_B = "GCTGAGTCAT", "TTCCGGTACA"


def planted(seed, together, n=3000, L=200):
    """two 10-mers in 30 % of the sequences: together (B 7 bases after A's end, both on +) or each on its own, uniformly"""
    rng = np.random.default_rng(seed)
    seqs = [rng.integers(1, 5, L).astype(np.uint8) for _ in range(n)]
    ma, mb = [np.array(["ACGT".index(c) + 1 for c in m], np.uint8) for m in (MOTIF_A, MOTIF_B)]
    if together:
        for i in np.nonzero(rng.random(n) < 0.3)[0]:
            p = int(rng.integers(0, L - 26))
            seqs[i][p:p + 10] = ma
            seqs[i][p + 17:p + 27] = mb
    else:
        for mot in (ma, mb):
            for i in np.nonzero(rng.random(n) < 0.3)[0]:
                p = int(rng.integers(0, L - 9))
                seqs[i][p:p + 10] = mot
    return seqs


def planted_motifs():
    bg = np.full(4, 0.25, np.float32)
    Ss, ts = [], []
    for word in (MOTIF_A, MOTIF_B):
        pwm = np.full((10, 4), 0.01, np.float32)
        for j, ch in enumerate(word):
            pwm[j, "ACGT".index(ch)] = 0.97
        S = ms.log_odds(pwm, bg)
        lo, tail = pk.score_tail_pvalues(S, bg)
        Ss.append(S)
        ts.append(pk.score_threshold(tail, lo, 1e-4))
    return Ss, ts


@pytest.mark.parametrize("together", [True, False], ids=["together", "independent"])
def test_planted_pair(ctx, together):
    seqs = planted(1, together)
    n, L, G = len(seqs), 200, 150
    Ss, ts = planted_motifs()
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    best, site = ctx.motif_best_sites(scan, Ss, [10, 10], True)
    hg, hl, hm = [h.to_host() for h in ctx.spacing_histograms(best, site, scan[3], n, [10, 10], ts, G, 10, L)]
    got = pk.spacing_summary(hg[0], hl[0], G, L, 10, 10, 4, n, hm[0], hm[1], 1)
    bs = [mc.best_sites(seqs, S, True, m) for m, S in enumerate(Ss)]
    whg, whl, whm = sp.histograms(np.stack([b for b, _ in bs]), np.stack([c for _, c in bs]), np.full(n, L), [10, 10], ts, G, 10, L)
    assert hg.tobytes() == whg.tobytes() and hl.tobytes() == whl.tobytes() and hm.tobytes() == whm.tobytes()
    want = sp.summary(whg[0], whl[0], G, L, 10, 10, 4, n, int(whm[0]), int(whm[1]), 1)
    for r in (got, want):
        print(together, {k: r[k] for k in ("both", "apart", "orientation", "gap", "count", "log10_pvalue_both", "log10_evalue")})
        assert r["both"] > 200
        if together:
            assert pk.SPACING_CLASSES[r["orientation"]] == "same_downstream" and r["gap"] == 7 and r["log10_evalue"] < -50
            assert r["log10_pvalue_both"] < -50  # (900 sequences where 9 % of 3000 are expected)
        else:
            assert r["log10_evalue"] > -1.3  # (E > 0.05)
    assert abs(got["log10_evalue"] - want["log10_evalue"]) <= 1e-9 * abs(want["log10_evalue"]) + 1e-9


def read_scores(path):
    """the integer log-odds matrices a run with --sites scanned with (PENGK_SITES_SCORES; tests/test_gpu_motif_qvalue.py)"""
    rows = [[int(x) for x in l.split()] for l in open(path)]
    out, k = [], 0
    while k < len(rows):
        w = rows[k][1]
        out.append(np.array(rows[k + 1:k + 1 + w], np.int32))
        k += 1 + w
    return out


def model_tsv(fa, js, P, both, G=150, n_motifs=16, scores=None):
    """the model's TSV from the JSON's PWMs -- or, with `scores`, from the integer matrices the run itself used -- and the
    input's order-0 background (the CLI's default background set)"""
    seqs = ms.read_fasta_codes(fa)
    codes, offs = ms.flatten(seqs)
    bg = np.asarray(po.bg_V(po.bg_counts(codes, offs, 2), 2), np.float32)[0:4]
    pats = json.loads(js)["patterns"]
    Ss = read_scores(scores) if scores else [ms.log_odds(np.array(p["pwm"], np.float32), bg) for p in pats]
    assert [len(S) for S in Ss] == [len(p["pwm"]) for p in pats]
    ts = []
    for S in Ss:
        lo, tail = mst.tail_pvalues(S, bg)
        ts.append(mst.threshold(lo, tail, P))
    return sp.render(seqs, [p["iupac_motif"] for p in pats], Ss, ts, both, G, n_motifs)


def assert_tsv_near_model(got, want):
    """line by line.  The JSON holds each PWM rounded to 8 decimals, so a log-odds entry of the model can be one unit
    off the run's (tests/test_gpu_motif_centrality.py, assert_tsv_near_model): a few best sites then differ, and with
    them the counts and the statistics, a little.  Everything else is equal."""
    g, w = got.splitlines(), want.splitlines()
    assert g[0] + "\n" == sp.HEADER and len(g) == len(w)
    same = 0
    for a, b in zip(g[1:], w[1:]):
        same += a == b
        fa, fb = a.split("\t"), b.split("\t")
        assert len(fa) == len(fb) == 21
        assert fa[:5] == fb[:5], (fa[:8], fb[:8])
        for j in (5, 6, 7, 10, 11, 12):  # sites_a, sites_b, both, overlapping, apart, far
            assert abs(int(fa[j]) - int(fb[j])) <= 3 + 0.01 * int(fb[j]), (j, fa[:13], fb[:13])
        assert abs(float(fa[9]) - float(fb[9])) <= 1.0 + 0.05 * abs(float(fb[9])), (fa[:13], fb[:13])
        if fa[13:15] == fb[13:15] and fa[13] != "NA":  # the same bin reported
            ha, hb = np.array(fa[20].split(","), np.int64), np.array(fb[20].split(","), np.int64)
            assert np.abs(ha - hb).sum() <= 4 + 0.02 * int(fb[11])
            assert abs(float(fa[18]) - float(fb[18])) <= 1.0 + 0.05 * abs(float(fb[18])), (fa[:20], fb[:20])
    assert same >= (len(g) - 1) / 2, (same, len(g) - 1)


def test_cli_spacing_equals_the_model_and_leaves_everything_else_alone(tmp_path):
    fa = os.path.join(GOLD, "MafK.fasta")
    rc, so0, se, meme0, js0 = run_plain([fa, "-w", "10"], tmp_path, tag="plain")
    assert rc == 0, se.decode()[-2000:]
    out = tmp_path / "sp.tsv"
    rc, so1, se, meme1, js1 = run_plain([fa, "-w", "10", "--spacing", str(out)], tmp_path, tag="sp")
    assert rc == 0, se.decode()[-2000:]
    assert (so1, meme1, js1) == (so0, meme0, js0)
    text = out.read_text()
    M = min(len(json.loads(js0)["patterns"]), 16)
    assert M >= 2 and text.count("\n") == M * (M - 1) // 2 + 1
    assert_tsv_near_model(text, model_tsv(fa, js1, 1e-4, True))
    # the two top motifs are pieces of one site (README, "Motif refinement"): they overlap, or keep one distance
    top = text.splitlines()[1].split("\t")
    assert top[0] == "1" and top[2] == "2"
    assert int(top[10]) > int(top[7]) / 2 or (top[19] != "NA" and float(top[19]) < -10), top[:20]
    # beside --score-motifs, --sites and --centrality: their outputs unchanged, the same motifs' TSV in their order
    names = ["s", "c", "s2", "c2", "sp2"]
    s, c, s2, c2, sp2 = [tmp_path / (x + ".tsv") for x in names]
    rc, so2, se, meme2, js2 = run_plain([fa, "-w", "10", "--score-motifs", "--sites", str(s), "--centrality", str(c)], tmp_path, tag="s")
    assert rc == 0, se.decode()[-2000:]
    rc, so3, se, meme3, js3 = run_plain([fa, "-w", "10", "--score-motifs", "--sites", str(s2), "--centrality", str(c2), "--spacing",
                                         str(sp2), "--spacing-pvalue", "1e-3", "--spacing-max-gap", "40"], tmp_path, tag="s2",
                                        extra_env={"PENGK_SITES_SCORES": str(tmp_path / "scores.txt")})
    assert rc == 0, se.decode()[-2000:]
    assert (so3, meme3, js3) == (so2, meme2, js2) and s2.read_bytes() == s.read_bytes() and c2.read_bytes() == c.read_bytes()
    # (with one pair there is one line, and at p = 1e-3 a single best site that the JSON's rounded PWMs move makes it
    # another line: here the model scores with the integer matrices of the run itself)
    assert_tsv_near_model(sp2.read_text(), model_tsv(fa, js3, 1e-3, True, G=40, scores=tmp_path / "scores.txt"))


def test_cli_motif_limit_and_a_bad_gap(tmp_path):
    fa = os.path.join(GOLD, "MafK.fasta")
    out = tmp_path / "two.tsv"
    rc, _, se, _, js = run_plain([fa, "-w", "10", "--spacing", str(out), "--spacing-motifs", "2"], tmp_path)
    assert rc == 0, se.decode()[-2000:]
    text = out.read_text()
    assert text.count("\n") == 2
    assert_tsv_near_model(text, model_tsv(fa, js, 1e-4, True, n_motifs=2))
    bad = tmp_path / "bad.tsv"
    rc, _, se, _, _ = run_plain([fa, "-w", "10", "--spacing", str(bad), "--spacing-max-gap", "1025"], tmp_path, tag="bad")
    assert rc == 4 and b"--spacing-max-gap" in se and not bad.exists()


def test_cli_plus_strand_and_a_sequence_above_the_limit(tmp_path):
    seqs = ms.read_fasta_codes(os.path.join(GOLD, "MafK.fasta"))[:400]
    rng = np.random.default_rng(71)
    long_seq = rng.integers(1, 5, 70000).astype(np.uint8)
    fa = tmp_path / "long.fa"
    with open(fa, "w") as fh:
        for i, c in enumerate(seqs[:200] + [long_seq] + seqs[200:]):
            fh.write(">r%d\n%s\n" % (i, "".join("NACGT"[x] for x in c)))
    out = tmp_path / "long.tsv"
    rc, _, se, _, js = run_plain([str(fa), "-w", "8", "--strand", "PLUS", "--spacing", str(out), "--spacing-pvalue", "1e-3"], tmp_path)
    assert rc == 0, se.decode()[-2000:]
    text = out.read_text()
    rows = [l.split("\t") for l in text.splitlines()[1:]]
    assert rows and all(r[4] == "400" for r in rows)  # (the 70 kb record is not considered)
    assert all(r[13] in ("NA", "same_downstream", "same_upstream") for r in rows)
    assert_tsv_near_model(text, model_tsv(str(fa), js, 1e-3, False))


@pytest.mark.parametrize("world", [2, 3])
def test_cli_ranks_write_what_one_process_writes(tmp_path, world):
    fa = os.path.join(GOLD, "MafK.fasta")
    one = tmp_path / "one.tsv"
    rc, so, se, meme, js = run_plain([fa, "-w", "10", "--spacing", str(one)], tmp_path)
    assert rc == 0, se.decode()[-2000:]
    many = tmp_path / "many.tsv"
    res = run_ranks([fa, "-w", "10", "--spacing", str(many)], world, tmp_path)
    for rank, (rrc, rso, rse, rmeme, rjs) in enumerate(res):
        assert rrc == 0, (rank, rse.decode()[-2000:])
        if rank == 0:
            assert rmeme == meme and rjs == js and rso == so
    assert many.read_bytes() == one.read_bytes()
