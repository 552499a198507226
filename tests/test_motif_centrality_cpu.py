"""CPU checks of the central-enrichment test (--centrality): the null f(L, w, r) against enumeration, the library's
summary against the numpy model on random histograms of equal and mixed lengths, the log-space binomial tail against a
math.lgamma term sum and scipy, its range far below double's, the edge cases, and the CLI's flags.  No device compute."""
import math
import os
import subprocess

import numpy as np
import pytest

import peng_motif_amd as pk
import motif_centrality_model as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "peng-motif_amd", "host", "peng_motif")
GOLD = os.path.join(ROOT, "tests", "golden")


def test_null_equals_enumeration():
    for L in range(1, 40):
        for w in range(1, L + 1):
            for r in range(0, L - w + 3):
                n = sum(1 for p in range(L - w + 1) if abs(2 * p + w - L) <= r)
                assert mc.f(L, w, r) == n / (L - w + 1), (L, w, r)


def random_hists(rng, lens, w, max_len, central):
    """the histograms of one site per sequence (a share `central` of them within +-3 bases of the centre)"""
    lens = np.asarray(lens, np.int64)
    best = np.zeros(len(lens), np.int32)
    site = np.zeros(len(lens), np.uint64)
    for i, L in enumerate(lens):
        D = int(L) - w
        if D < 0:
            best[i] = mc.SENTINEL
            continue
        p = int(rng.integers(0, D + 1))
        if rng.random() < central:
            p = min(max(D // 2 + int(rng.integers(-3, 4)), 0), D)
        site[i] = 2 * p + int(rng.integers(0, 2))
    best[rng.random(len(lens)) < 0.3] = -1  # (below the threshold 0: no site)
    return mc.histograms(best, site, lens, w, 0, max_len)


def check_against_model(hd, hl, max_len, w, M):
    got = pk.centrality_summary(hd, hl, max_len, w, M)
    want = mc.summary(hd, hl, max_len, w, M)
    assert got["sites"] == want["sites"] and got["max_offset"] == want["max_offset"]
    if want["sites"] == 0:
        return got
    K, e, lp = mc.window(hd, hl, max_len, w, got["window"])
    assert got["in_window"] == K
    assert abs(got["expected"] - e) <= 1e-12 * e
    assert abs(got["log10_pvalue"] - lp) <= 1e-9 * abs(lp) + 1e-9
    assert abs(lp - want["log10_pvalue"]) <= 1e-9 * abs(want["log10_pvalue"]) + 1e-12  # (the model's minimum)
    assert abs(got["log10_evalue"] - (got["log10_pvalue"] + math.log10(got["max_offset"] + 1) + math.log10(M))) < 1e-9
    return got


@pytest.mark.parametrize("central", [0.0, 0.05, 0.5])
@pytest.mark.parametrize("seed", range(3))
def test_summary_equal_lengths(seed, central):
    rng = np.random.default_rng(seed)
    w = int(rng.integers(1, 20))
    L = int(rng.integers(w, 260))
    hd, hl = random_hists(rng, [L] * int(rng.integers(1, 3000)), w, 300, central)
    got = check_against_model(hd, hl, 300, w, 7)
    if got["sites"] and central == 0.5 and got["sites"] > 200 and L - w > 20:
        assert got["window"] <= 7 and got["log10_pvalue"] < -10


@pytest.mark.parametrize("central", [0.0, 0.3])
@pytest.mark.parametrize("seed", range(4))
def test_summary_mixed_lengths(seed, central):
    rng = np.random.default_rng(100 + seed)
    w = int(rng.integers(1, 30))
    lens = rng.integers(0, 400, int(rng.integers(1, 2000)))
    check_against_model(*random_hists(rng, lens, w, 400, central), 400, w, 3)


def test_log_tail_equals_lgamma_sum():
    rng = np.random.default_rng(9)
    for _ in range(300):
        N = int(rng.integers(1, 5001))
        K = int(rng.integers(0, N + 1))
        p = float(rng.choice([rng.random(), rng.random() * 1e-3, 1 - rng.random() * 1e-3, K / N]))
        got, want = pk.binomial_log10_sf(N, K, p), mc.log10_sf(N, K, p)
        assert abs(got - want) <= 1e-9 * abs(want) + 1e-9, (N, K, p, got, want)
    assert pk.binomial_log10_sf(10, 0, 0.3) == 0.0 and pk.binomial_log10_sf(10, 4, 1.0) == 0.0
    assert pk.binomial_log10_sf(10, 4, 0.0) == -math.inf
    assert pk.binomial_log10_sf(10, 10, 0.5) == pytest.approx(10 * math.log10(0.5), rel=1e-14)


def test_log_tail_equals_scipy_where_finite():
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(10)
    n_cmp = 0
    for _ in range(300):
        N = int(10 ** rng.uniform(0, 7))
        K = int(rng.integers(0, N + 1))
        p = float(rng.random() ** 3)
        want = float(stats.binom.logsf(K - 1, N, p)) / math.log(10.0)
        if not math.isfinite(want) or want < -300:
            continue
        got = pk.binomial_log10_sf(N, K, p)
        assert abs(got - want) <= 1e-7 * abs(want) + 1e-9, (N, K, p, got, want)
        n_cmp += 1
    assert n_cmp > 100


def test_ten_million_sites_far_below_double():
    # 1e7 sequences of 205 bases, w = 10: every best site next to the centre (d = +-1, D = 195 is odd)
    max_len, w, N = 205, 10, 10 ** 7
    hd, hl = np.zeros(2 * max_len + 1, np.uint64), np.zeros(max_len + 1, np.uint64)
    hl[205] = N
    hd[max_len - 1] = N // 2
    hd[max_len + 1] = N - N // 2
    got = pk.centrality_summary(hd, hl, max_len, w, 16)
    assert got["window"] == 1 and got["in_window"] == N and got["expected"] == pytest.approx(N * 2 / 196, rel=1e-12)
    assert math.isfinite(got["log10_pvalue"]) and got["log10_pvalue"] < -1e5
    assert got["log10_pvalue"] == pytest.approx(N * math.log10(2 / 196), rel=1e-9)  # (K = N: P = p^N)
    # a central motif at 1e7 sequences, half of them near the centre: still finite
    hd[:] = 0
    rng = np.random.default_rng(3)
    d = 2 * rng.integers(0, 196, N // 2) - 195
    hd += np.bincount(d + max_len, minlength=2 * max_len + 1).astype(np.uint64)
    hd[max_len + 1] += np.uint64(N - N // 2)
    got = pk.centrality_summary(hd, hl, max_len, w, 16)
    assert got["window"] == 1 and math.isfinite(got["log10_pvalue"]) and got["log10_pvalue"] < -1e5


def test_edge_cases():
    max_len = 50
    z = np.zeros(2 * max_len + 1, np.uint64), np.zeros(max_len + 1, np.uint64)
    assert pk.centrality_summary(*z, max_len, 5, 1)["sites"] == 0 and mc.summary(*z, max_len, 5, 1)["sites"] == 0
    assert mc.line(1, "ACGT", 4, 9, z[0], max_len, mc.summary(*z, max_len, 4, 1)) == "1\tACGT\t4\t9\t0" + "\tNA" * 7
    # Dm = 0: every sequence as long as the motif
    hd, hl = np.zeros(2 * max_len + 1, np.uint64), np.zeros(max_len + 1, np.uint64)
    hl[8], hd[max_len] = 30, 30
    got = check_against_model(hd, hl, max_len, 8, 4)
    assert (got["max_offset"], got["window"], got["in_window"], got["expected"], got["log10_pvalue"]) == (0, 0, 30, 30.0, 0.0)
    assert got["log10_evalue"] == pytest.approx(math.log10(4))
    # K = 0 below the edges: every site at d = +-D, D = 11 odd -- the first window that can hold a site is r = 1
    hd, hl = np.zeros(2 * max_len + 1, np.uint64), np.zeros(max_len + 1, np.uint64)
    hl[21], hd[max_len - 11], hd[max_len + 11] = 20, 10, 10
    got = check_against_model(hd, hl, max_len, 10, 1)
    assert (got["window"], got["in_window"], got["log10_pvalue"]) == (1, 0, 0.0)
    assert mc.line(1, "X", 10, 20, hd, max_len, got).split("\t")[5:9] == ["0.5", "0", "3.33", "0.000"]


def test_summary_refuses_inconsistent_histograms():
    max_len = 20
    hd, hl = np.zeros(2 * max_len + 1, np.uint64), np.zeros(max_len + 1, np.uint64)
    hl[15], hd[max_len] = 3, 2
    with pytest.raises(pk.PengkError):  # (totals differ)
        pk.centrality_summary(hd, hl, max_len, 5, 1)
    hd[max_len], hd[max_len + 12] = 2, 1
    with pytest.raises(pk.PengkError):  # (an offset beyond L - w)
        pk.centrality_summary(hd, hl, max_len, 5, 1)


def clean_env():
    return {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PENGK_COMM_TRANSPORT")}


def test_help_lists_the_centrality_flags():
    r = subprocess.run([CLI, "-h"], stdout=subprocess.PIPE, env=clean_env(), timeout=60)
    assert r.returncode == 0
    assert b"--centrality FILE" in r.stdout and b"--centrality-pvalue" in r.stdout


@pytest.mark.parametrize("bad", ["0", "-1e-4", "1.5", "abc", "nan", "1e-4x"])
def test_bad_centrality_pvalue_is_refused(tmp_path, bad):
    r = subprocess.run([CLI, os.path.join(GOLD, "MafK.fasta"), "--centrality", str(tmp_path / "c.tsv"), "--centrality-pvalue", bad],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=clean_env(), timeout=60)
    assert r.returncode == 4, (bad, r.returncode, r.stderr[-500:])
    assert b"--centrality-pvalue" in r.stderr
    assert not (tmp_path / "c.tsv").exists()
