"""Central enrichment on the device (--centrality; include/pengk.h, "central enrichment") against the numpy model of
tests/motif_centrality_model.py: the best site of every motif on every sequence bit for bit (ties included, under any
split of the records), the histograms, a planted central motif against a planted uniform one, and the CLI's TSV against
the model, beside the other outputs, with a sequence above the length limit and over several ranks."""
import json
import os

import numpy as np
import pytest

import peng_motif_amd as pk
import motif_centrality_model as mc
import motif_score_model as ms
import motif_sites_model as mst
from oracle import oracle as po
from test_gpu_multirank import run_plain, run_ranks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
WIDTHS = [1, 2, 3, 4, 5, 8, 10, 13, 16, 21, 31, 33, 48, 64, 7, 12]


@pytest.fixture(scope="module")
def ctx():
    c = pk.Context(0)
    yield c
    c.close()


def random_S(rng, w):
    S = rng.integers(-300, 301, (w, 4)).astype(np.int32)
    S[rng.random((w, 4)) < 0.05] = -2000
    S[rng.random((w, 4)) < 0.02] = 2000
    return S


def random_seqs(rng):
    lens = [0, 1, 31, 32, 33, 64, 65, 200] + rng.integers(0, 400, 60).tolist()
    seqs = []
    for n in lens:
        c = rng.integers(1, 5, n).astype(np.uint8)
        for _ in range(int(rng.integers(0, 3))):  # N runs
            if n:
                a = int(rng.integers(0, n))
                c[a:a + int(rng.integers(1, 20))] = 0
        seqs.append(c)
    return seqs


def motifs(rng):
    """random motifs of every width, then tie-heavy ones: all zero (every window ties), constant rows, two values"""
    widths = WIDTHS + [1, 6, 10, 13, 64]
    S = [random_S(rng, w) for w in WIDTHS]
    S.append(np.zeros((1, 4), np.int32))
    S.append(np.zeros((6, 4), np.int32))
    S.append(np.repeat(rng.integers(-50, 50, (10, 1)), 4, axis=1).astype(np.int32))
    S.append(rng.integers(0, 2, (13, 4)).astype(np.int32))
    S.append(np.full((64, 4), 7, np.int32))
    return S, widths


def model_best(seqs, S, both, seq0=0):
    r = [mc.best_sites(seqs, s, both, m, seq0) for m, s in enumerate(S)]
    return np.stack([b for b, _ in r]), np.stack([c for _, c in r])


def sub_scan(scan, i0, i1):
    """records [i0, i1) of a device scan layout (the words stay shared)"""
    return scan[0], scan[1], scan[2].ptr + 8 * i0, scan[3].ptr + 4 * i0, i1 - i0


@pytest.mark.parametrize("both", [True, False], ids=["both", "plus"])
def test_best_sites_equal_the_model(ctx, both):
    rng = np.random.default_rng(31 + both)
    seqs = random_seqs(rng)
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    S, widths = motifs(rng)
    best, site = ctx.motif_best_sites(scan, S, widths, both)
    wb, ws = model_best(seqs, S, both)
    gb, gs = best.to_host(), site.to_host()
    assert gb.tobytes() == wb.tobytes()
    assert gs.tobytes() == ws.tobytes()
    if not both:
        assert np.all(gs % 2 == 0)
    # the tie-heavy motifs tie on every window: the key, not the scan order, chooses (not always the first window)
    n_ok = sum(len(c) >= 6 for c in seqs)
    assert np.count_nonzero(gs[len(WIDTHS) + 1] > 1) > n_ok // 2


def test_split_records_give_the_same_arrays(ctx):
    rng = np.random.default_rng(41)
    seqs = random_seqs(rng)
    n = len(seqs)
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    S, widths = motifs(rng)
    whole = [a.to_host() for a in ctx.motif_best_sites(scan, S, widths, True)]
    for k in [1, 29, n - 1]:
        a = [x.to_host()[:, :k] for x in ctx.motif_best_sites(sub_scan(scan, 0, k), S, widths, True, seq0=0)]
        b = [x.to_host()[:, :n - k] for x in ctx.motif_best_sites(sub_scan(scan, k, n), S, widths, True, seq0=k)]
        for j in range(2):
            assert np.concatenate([a[j], b[j]], axis=1).tobytes() == whole[j].tobytes(), k
    # and the model under a shifted global index: a different tie-break, the same scores
    b5, s5 = [x.to_host() for x in ctx.motif_best_sites(scan, S, widths, True, seq0=5)]
    wb, ws = model_best(seqs, S, True, seq0=5)
    assert b5.tobytes() == wb.tobytes() == whole[0].tobytes() and s5.tobytes() == ws.tobytes()


def device_hists(ctx, best, site, lens_dev, n_seq, widths, thr, max_len):
    hd, hl = ctx.centrality_histograms(best, site, lens_dev, n_seq, widths, thr, max_len)
    return hd.to_host().reshape(len(widths), -1), hl.to_host().reshape(len(widths), -1)


def test_histograms_equal_the_model_small_input(ctx):
    rng = np.random.default_rng(51)
    seqs = random_seqs(rng)
    lens = np.array([len(c) for c in seqs])
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    S, widths = motifs(rng)
    best, site = ctx.motif_best_sites(scan, S, widths, True)
    gb, gs = best.to_host(), site.to_host()
    thr = [int(np.percentile(gb[m][gb[m] > mc.SENTINEL], 30)) if np.any(gb[m] > mc.SENTINEL) else 0 for m in range(len(S))]
    for max_len in [int(lens.max()), 200, 40000]:  # (the global bins: a small input, or too many bins for LDS)
        hd, hl = device_hists(ctx, best, site, scan[3], len(seqs), widths, thr, max_len)
        for m in range(len(S)):
            wd, wl = mc.histograms(gb[m], gs[m], lens, widths[m], thr[m], max_len)
            assert hd[m].tobytes() == wd.tobytes() and hl[m].tobytes() == wl.tobytes(), (max_len, m)
        assert hl[:, :].sum() > 100


def test_histograms_equal_the_model_lds_bins(ctx):
    n, L = 200000, 200
    scan = ctx.synth_scan(3, 0, n, L)
    rng = np.random.default_rng(61)
    widths = [10, 12, 14, 1]
    S = [random_S(rng, w) for w in widths[:3]] + [np.zeros((1, 4), np.int32)]
    best, site = ctx.motif_best_sites(scan, S, widths, True)
    gb, gs = best.to_host(), site.to_host()
    thr = [int(np.median(gb[m])) for m in range(len(S))]
    hd, hl = device_hists(ctx, best, site, scan[3], n, widths, thr, L)
    lens = np.full(n, L)
    for m in range(len(S)):
        wd, wl = mc.histograms(gb[m], gs[m], lens, widths[m], thr[m], L)
        assert hd[m].tobytes() == wd.tobytes() and hl[m].tobytes() == wl.tobytes(), m
        assert int(hl[m].sum()) > n // 3
    # the all-zero motif of width 1: every window ties and the key spreads the chosen site uniformly
    d = hd[3][L - 199:L + 200:2].astype(np.float64)
    e = n / 200
    assert np.all(np.abs(d - e) < 6 * np.sqrt(e))


def planted(seed, central, n=2000, L=200):
    rng = np.random.default_rng(seed)
    seqs = [rng.integers(1, 5, L).astype(np.uint8) for _ in range(n)]
    mot = np.array(["ACGT".index(c) + 1 for c in "GCTGAGTCAT"], np.uint8)
    for i in np.nonzero(rng.random(n) < 0.2)[0]:
        p = L // 2 - 5 + int(rng.integers(-3, 4)) if central else int(rng.integers(0, L - 9))
        seqs[i][p:p + 10] = mot
    return seqs


@pytest.mark.parametrize("central", [True, False], ids=["central", "uniform"])
def test_planted_motif(ctx, central):
    seqs = planted(1, central)
    pwm = np.full((10, 4), 0.01, np.float32)
    for j, ch in enumerate("GCTGAGTCAT"):
        pwm[j, "ACGT".index(ch)] = 0.97
    bg = np.full(4, 0.25, np.float32)
    S = ms.log_odds(pwm, bg)
    lo, tail = pk.score_tail_pvalues(S, bg)
    t = pk.score_threshold(tail, lo, 1e-4)
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    best, site = ctx.motif_best_sites(scan, [S], [10], True)
    hd, hl = device_hists(ctx, best, site, scan[3], len(seqs), [10], [t], 200)
    got = pk.centrality_summary(hd[0], hl[0], 200, 10, 1)
    assert got["sites"] > 300
    if central:
        assert got["window"] / 2 <= 3 and got["log10_evalue"] < -100
    else:
        assert got["log10_evalue"] > -1.3  # (E > 0.05)


def model_tsv(fa, js, P, both):
    """the model's TSV from the JSON's PWMs and the input's order-0 background (the CLI's default background set)"""
    seqs = ms.read_fasta_codes(fa)
    codes, offs = ms.flatten(seqs)
    bg = np.asarray(po.bg_V(po.bg_counts(codes, offs, 2), 2), np.float32)[0:4]
    pats = json.loads(js)["patterns"]
    Ss = [ms.log_odds(np.array(p["pwm"], np.float32), bg) for p in pats]
    ts = []
    for S in Ss:
        lo, tail = mst.tail_pvalues(S, bg)
        ts.append(mst.threshold(lo, tail, P))
    return mc.render(seqs, [p["iupac_motif"] for p in pats], Ss, ts, both)


def assert_tsv_near_model(got, want):
    """line by line.  The JSON holds each PWM rounded to 8 decimals, so a log-odds entry of the model can be one unit
    off the run's (tests/test_gpu_motif_sites.py, assert_cli_equals_model): a few best sites then differ, and with them
    the counts and the statistic, a little.  Everything else is equal."""
    g, w = got.splitlines(), want.splitlines()
    assert g[0] + "\n" == mc.HEADER and len(g) == len(w)
    same = 0
    for a, b in zip(g[1:], w[1:]):
        same += a == b
        fa, fb = a.split("\t"), b.split("\t")
        assert fa[:4] == fb[:4], (fa[:5], fb[:5])
        na, nb = int(fa[4]), int(fb[4])
        assert abs(na - nb) <= 3 + 0.01 * nb, (fa[:5], fb[:5])
        if nb == 0 or na == 0:
            continue
        oa, ob = np.array(fa[11].split(","), np.int64), np.array(fb[11].split(","), np.int64)
        if len(oa) == len(ob):
            assert np.abs(oa - ob).sum() <= 4 + 0.02 * nb
        pa, pb = float(fa[9]), float(fb[9])
        assert abs(pa - pb) <= 1.0 + 0.05 * abs(pb), (fa[:11], fb[:11])
    assert same >= (len(g) - 1) / 2, (same, len(g) - 1)


def test_cli_centrality_equals_the_model_and_leaves_everything_else_alone(tmp_path):
    fa = os.path.join(GOLD, "MafK.fasta")
    rc, so0, se, meme0, js0 = run_plain([fa, "-w", "10"], tmp_path, tag="plain")
    assert rc == 0, se.decode()[-2000:]
    cen = tmp_path / "cen.tsv"
    rc, so1, se, meme1, js1 = run_plain([fa, "-w", "10", "--centrality", str(cen)], tmp_path, tag="cen")
    assert rc == 0, se.decode()[-2000:]
    assert (so1, meme1, js1) == (so0, meme0, js0)
    text = cen.read_text()
    assert text.count("\n") == len(json.loads(js0)["patterns"]) + 1
    assert_tsv_near_model(text, model_tsv(fa, js1, 1e-4, True))
    top = min(float(l.split("\t")[10]) for l in text.splitlines()[1:])
    assert top < -100
    # beside --sites and --score-motifs: their outputs unchanged, the same motifs' TSV in their order
    sites, sites2, cen2 = tmp_path / "s.tsv", tmp_path / "s2.tsv", tmp_path / "cen2.tsv"
    rc, so2, se, meme2, js2 = run_plain([fa, "-w", "10", "--score-motifs", "--sites", str(sites)], tmp_path, tag="s")
    assert rc == 0, se.decode()[-2000:]
    rc, so3, se, meme3, js3 = run_plain([fa, "-w", "10", "--score-motifs", "--sites", str(sites2), "--centrality", str(cen2),
                                         "--centrality-pvalue", "1e-3"], tmp_path, tag="s2")
    assert rc == 0, se.decode()[-2000:]
    assert (so3, meme3, js3) == (so2, meme2, js2) and sites2.read_bytes() == sites.read_bytes()
    assert_tsv_near_model(cen2.read_text(), model_tsv(fa, js3, 1e-3, True))


def test_cli_plus_strand_and_a_sequence_above_the_limit(tmp_path):
    seqs = ms.read_fasta_codes(os.path.join(GOLD, "MafK.fasta"))[:400]
    rng = np.random.default_rng(71)
    long_seq = rng.integers(1, 5, 70000).astype(np.uint8)
    fa = tmp_path / "long.fa"
    with open(fa, "w") as fh:
        for i, c in enumerate(seqs[:200] + [long_seq] + seqs[200:]):
            fh.write(">r%d\n%s\n" % (i, "".join("NACGT"[x] for x in c)))
    cen = tmp_path / "long.tsv"
    rc, _, se, _, js = run_plain([str(fa), "-w", "8", "--strand", "PLUS", "--centrality", str(cen), "--centrality-pvalue", "1e-3"],
                                 tmp_path)
    assert rc == 0, se.decode()[-2000:]
    text = cen.read_text()
    rows = [l.split("\t") for l in text.splitlines()[1:]]
    assert rows and all(r[3] == "400" for r in rows)  # (the 70 kb record is not considered)
    assert all(int(r[4]) <= 400 for r in rows)
    assert_tsv_near_model(text, model_tsv(str(fa), js, 1e-3, False))


@pytest.mark.parametrize("world", [2, 3])
def test_cli_ranks_write_what_one_process_writes(tmp_path, world):
    fa = os.path.join(GOLD, "MafK.fasta")
    one = tmp_path / "one.tsv"
    rc, so, se, meme, js = run_plain([fa, "-w", "10", "--centrality", str(one)], tmp_path)
    assert rc == 0, se.decode()[-2000:]
    many = tmp_path / "many.tsv"
    res = run_ranks([fa, "-w", "10", "--centrality", str(many)], world, tmp_path)
    for rank, (rrc, rso, rse, rmeme, rjs) in enumerate(res):
        assert rrc == 0, (rank, rse.decode()[-2000:])
        if rank == 0:
            assert rmeme == meme and rjs == js and rso == so
    assert many.read_bytes() == one.read_bytes()
