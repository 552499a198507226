"""CPU checks of the motif pair test (--spacing): the orientation classes and the null p(g) against enumeration of every
placement, their invariance under reverse complement, the library's summary against the numpy model on random
histograms, the edge cases, and the CLI's flags.  No device compute."""
import math
import os
import subprocess

import numpy as np
import pytest

import peng_motif_amd as pk
import motif_centrality_model as mc
import motif_spacing_model as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "peng-motif_amd", "host", "peng_motif")
GOLD = os.path.join(ROOT, "tests", "golden")


def near(got, want, rel, absolute=0.0):
    return abs(got - want) <= rel * abs(want) + absolute


def enumerate_placements(L, wa, wb, G, strands):
    """the gap bins over every (p_a, p_b, s_a, s_b) of one sequence, each once"""
    h = np.zeros(sp.n_bins(G), np.int64)
    for pa in range(L - wa + 1):
        for pb in range(L - wb + 1):
            for sa in range(strands):
                for sb in range(strands):
                    h[sp.classify(pa, sa, wa, pb, sb, wb, G)[0]] += 1
    return h


@pytest.mark.parametrize("strands", [1, 2])
def test_classes_and_gaps_are_proportional_to_the_placements(strands):
    C = 2 * strands
    for L, wa, wb in [(24, 3, 8), (24, 8, 3), (20, 1, 1), (12, 6, 6), (13, 6, 6), (24, 10, 13), (9, 4, 6)]:
        G = L  # (every gap has a bin)
        h = enumerate_placements(L, wa, wb, G, strands)
        T = L - wa - wb + 1
        apart = 0
        for c in range(4):
            for g in range(G + 1):
                # a class holds one side for each strand of a: strands * k(L, g) placements
                want = strands * sp.placements(L, wa, wb, g) if c < C else 0
                assert h[c * (G + 1) + g] == want, (L, wa, wb, c, g)
                apart += want
        assert h[4 * (G + 1) + 1] == 0 and h.sum() == strands * strands * (L - wa + 1) * (L - wb + 1)
        if T < 1:
            assert apart == 0
            continue
        assert apart == strands * C * T * (T + 1) // 2
        # p(g) of the model is the share of the apart placements in one (class, gap), and they sum to one
        hl = np.zeros(L + 1, np.int64)
        hl[L] = 5
        total = 0.0
        for g in range(G + 1):
            p = sp.gap_probability(hl, wa, wb, g, C)
            assert near(p, h[g] / apart, 1e-14)
            total += C * p
        assert near(total, 1.0, 1e-13)


def test_reverse_complement_changes_no_bin():
    rng = np.random.default_rng(5)
    for _ in range(4000):
        wa, wb = int(rng.integers(1, 9)), int(rng.integers(1, 9))
        L = int(rng.integers(max(wa, wb), 25))
        pa, pb = int(rng.integers(0, L - wa + 1)), int(rng.integers(0, L - wb + 1))
        sa, sb = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        G = int(rng.integers(0, 12))
        assert sp.classify(pa, sa, wa, pb, sb, wb, G) == sp.classify(L - wa - pa, 1 - sa, wa, L - wb - pb, 1 - sb, wb, G)


def random_pair(rng, n, lens, wa, wb, G, strands, planted=0.0):
    """(hg, hl, n, n_a, n_b) of one pair from random sites (a share `planted` of them: b right after a at gap 2)"""
    lens = np.asarray(lens, np.int64)
    best = np.zeros((2, n), np.int32)
    site = np.zeros((2, n), np.uint64)
    for i, L in enumerate(lens):
        for m, w in enumerate((wa, wb)):
            if L < w:
                best[m, i] = mc.SENTINEL
                continue
            site[m, i] = 2 * int(rng.integers(0, L - w + 1)) + int(rng.integers(0, strands))
        if rng.random() < planted and L >= wa + wb + 2:
            pa = int(rng.integers(0, L - wa - wb - 1))
            site[0, i], site[1, i] = 2 * pa, 2 * (pa + wa + 2)
    best[rng.random((2, n)) < 0.3] = -1  # (below the threshold 0: no site)
    max_len = int(max(lens.max(), 1))
    wmax = max(wa, wb)
    hg, hl, hm = sp.histograms(best, site, lens, [wa, wb], [0, 0], G, wmax, max_len)
    return hg[0], hl[0], int((lens >= wmax).sum()), int(hm[0]), int(hm[1]), max_len


def check_against_model(hg, hl, G, max_len, wa, wb, C, n, n_a, n_b, n_pairs):
    got = pk.spacing_summary(hg, hl, G, max_len, wa, wb, C, n, n_a, n_b, n_pairs)
    want = sp.summary(hg, hl, G, max_len, wa, wb, C, n, n_a, n_b, n_pairs)
    for k in ("both", "overlapping", "apart", "far", "tested_gaps"):
        assert got[k] == want[k], k
    assert near(got["expected_both"], want["expected_both"], 1e-12)
    assert near(got["log10_pvalue_both"], want["log10_pvalue_both"], 1e-9, 1e-9)
    if want["apart"] == 0:
        assert (got["orientation"], got["gap"], got["count"], got["expected"], got["log10_pvalue"], got["log10_evalue"]) == \
            (0, 0, 0, 0.0, 0.0, 0.0)
        return got
    # the reported bin holds what the model computes for it, and it is the model's minimum
    c, g = got["orientation"], got["gap"]
    assert c < C and g <= G
    H = int(np.asarray(hg)[c * (G + 1) + g])
    p = sp.gap_probability(hl, wa, wb, g, C)
    assert got["count"] == H and p > 0.0
    assert near(got["expected"], want["apart"] * p, 1e-12)
    assert near(got["log10_pvalue"], mc.log10_sf(want["apart"], H, min(1.0, p)), 1e-9, 1e-9)
    assert near(got["log10_pvalue"], want["log10_pvalue"], 1e-9, 1e-9)
    assert near(got["log10_evalue"], got["log10_pvalue"] + math.log10(C * got["tested_gaps"]) + math.log10(n_pairs), 1e-9, 1e-9)
    return got


@pytest.mark.parametrize("strands", [1, 2])
@pytest.mark.parametrize("planted", [0.0, 0.3])
@pytest.mark.parametrize("seed", range(3))
def test_summary_equals_the_model(seed, planted, strands):
    rng = np.random.default_rng(1000 * strands + seed)
    wa, wb = int(rng.integers(1, 15)), int(rng.integers(1, 15))
    n = int(rng.integers(1, 1500))
    if seed == 0:
        lens = np.full(n, int(rng.integers(wa + wb, 120)))
    else:
        lens = rng.integers(0, 150, n)
    G = int(rng.choice([0, 1, 7, 40, 200]))
    hg, hl, nc, n_a, n_b, max_len = random_pair(rng, n, lens, wa, wb, G, strands, planted)
    got = check_against_model(hg, hl, G, max_len, wa, wb, 2 * strands, nc, n_a, n_b, 6)
    if planted and got["apart"] > 150 and G >= 7:
        assert (got["orientation"], got["gap"]) == (0, 2) and got["log10_evalue"] < -10


def test_edge_cases():
    G, max_len, wa, wb = 5, 40, 4, 6
    B = sp.n_bins(G)
    z = np.zeros(B, np.uint64), np.zeros(max_len + 1, np.uint64)
    # Na = 0, nothing at all
    got = check_against_model(*z, G, max_len, wa, wb, 4, 100, 10, 20, 3)
    assert got["both"] == 0 and got["expected_both"] == pytest.approx(2.0) and got["log10_pvalue_both"] == 0.0
    assert sp.line(0, "AC", 1, "GT", 100, 10, 20, z[0], G, sp.summary(*z, G, max_len, wa, wb, 4, 100, 10, 20, 3)).endswith(
        "\t0\t2.00\t0.000\t0\t0\t0" + "\tNA" * 8)
    # Na = 0 with overlapping pairs only; no considered sequence at all
    hg = z[0].copy()
    hg[4 * (G + 1)] = 7
    got = check_against_model(hg, z[1], G, max_len, wa, wb, 4, 50, 7, 7, 1)
    assert (got["both"], got["overlapping"], got["apart"], got["tested_gaps"]) == (7, 7, 0, 0)
    got = check_against_model(*z, G, max_len, wa, wb, 4, 0, 0, 0, 1)
    assert got["expected_both"] == 0.0 and got["log10_pvalue_both"] == 0.0
    # one sequence, L = 12: T = 3, K = 6; its gap 1 in class 3
    hg, hl = z[0].copy(), z[1].copy()
    hg[3 * (G + 1) + 1], hl[12] = 1, 1
    got = check_against_model(hg, hl, G, max_len, wa, wb, 4, 1, 1, 1, 1)
    assert (got["orientation"], got["gap"], got["count"], got["tested_gaps"]) == (3, 1, 1, 3)
    assert got["expected"] == pytest.approx(2 / 24, rel=1e-12)
    assert got["log10_pvalue"] == pytest.approx(math.log10(2 / 24), rel=1e-12)
    assert got["log10_evalue"] == pytest.approx(math.log10(2 / 24) + math.log10(12), rel=1e-12, abs=1e-12)
    assert got["log10_pvalue_both"] == 0.0  # (p_co = 1)
    # K = Na in one bin: P = p^Na in closed form, far below double's range
    Na = 10 ** 5
    hg, hl = z[0].copy(), z[1].copy()
    hg[1 * (G + 1) + 0], hl[40] = Na, Na  # T = 31, K = 496, k(40, 0) = 31
    got = check_against_model(hg, hl, G, max_len, wa, wb, 4, 2 * Na, Na, Na, 10)
    assert (got["orientation"], got["gap"], got["count"]) == (1, 0, Na)
    assert got["log10_pvalue"] == pytest.approx(Na * math.log10(31 / (4 * 496)), rel=1e-9)
    # far pairs count as apart and in the length bins, and get no test of their own
    hg, hl = z[0].copy(), z[1].copy()
    hg[4 * (G + 1) + 1], hl[30] = 9, 9
    got = check_against_model(hg, hl, G, max_len, wa, wb, 4, 20, 9, 9, 1)
    assert (got["apart"], got["far"], got["count"], got["log10_pvalue"], got["tested_gaps"]) == (9, 9, 0, 0.0, G + 1)


def test_ties_go_to_the_smaller_class_then_the_smaller_gap():
    G, max_len, wa, wb = 6, 30, 3, 3
    hg, hl = np.zeros(sp.n_bins(G), np.uint64), np.zeros(max_len + 1, np.uint64)
    # nothing but far pairs: every bin has log10 P = 0 -- (0, 0) is reported
    hg[4 * (G + 1) + 1], hl[30] = 4, 4
    got = pk.spacing_summary(hg, hl, G, max_len, wa, wb, 4, 10, 5, 5, 1)
    assert (got["orientation"], got["gap"], got["count"]) == (0, 0, 0)
    # the same count at the same gap in classes 3, 1 and 2: the same p(g), the same tail -- class 1 is reported
    hg[:] = 0
    hg[3 * (G + 1) + 2], hg[1 * (G + 1) + 2], hg[2 * (G + 1) + 2] = 5, 5, 5
    hl[30] = 15
    got = check_against_model(hg, hl, G, max_len, wa, wb, 4, 40, 20, 20, 1)
    assert (got["orientation"], got["gap"], got["count"]) == (1, 2, 5)
    # (two gaps of one class tie only with a count of zero in both, p(g) falling with g: the first case above)


def test_two_classes():
    G, max_len, wa, wb = 4, 20, 2, 5
    hg, hl = np.zeros(sp.n_bins(G), np.uint64), np.zeros(max_len + 1, np.uint64)
    hg[1 * (G + 1) + 3], hg[0], hl[20] = 30, 2, 32  # T = 14, K = 105, k(20, 3) = 11
    got = check_against_model(hg, hl, G, max_len, wa, wb, 2, 60, 40, 35, 3)
    assert (got["orientation"], got["gap"], got["count"], got["tested_gaps"]) == (1, 3, 30, 5)
    assert got["expected"] == pytest.approx(32 * 11 / (2 * 105), rel=1e-12)
    assert got["log10_evalue"] == pytest.approx(got["log10_pvalue"] + math.log10(10) + math.log10(3), rel=1e-12)
    # a count in an opposite-strand class cannot come from a + only run
    hg[2 * (G + 1)], hl[20] = 1, 33
    with pytest.raises(pk.PengkError):
        pk.spacing_summary(hg, hl, G, max_len, wa, wb, 2, 60, 40, 35, 3)
    assert pk.spacing_summary(hg, hl, G, max_len, wa, wb, 4, 60, 40, 35, 3)["apart"] == 33


def test_summary_refuses_bad_arguments():
    G, max_len, wa, wb = 4, 20, 2, 5
    hg, hl = np.zeros(sp.n_bins(G), np.uint64), np.zeros(max_len + 1, np.uint64)
    hg[0], hl[20] = 3, 3
    ok = dict(max_gap=G, max_len=max_len, w_a=wa, w_b=wb, n_classes=4, n=10, n_a=5, n_b=5, n_pairs=1)
    assert pk.spacing_summary(hg, hl, **ok)["apart"] == 3
    for bad in [dict(n_classes=3), dict(n_classes=1), dict(w_a=0), dict(w_b=65), dict(n_pairs=0), dict(n_a=11), dict(n_b=2),
                dict(n_a=2)]:
        with pytest.raises(pk.PengkError) as e:
            pk.spacing_summary(hg, hl, **dict(ok, **bad))
        assert e.value.code == pk.ERR_ARG and "pengk_spacing_summary" in str(e.value), bad
    hl2 = hl.copy()
    hl2[20] = 2
    with pytest.raises(pk.PengkError):  # (totals differ)
        pk.spacing_summary(hg, hl2, **ok)
    hl2[:] = 0
    hl2[6] = 3
    with pytest.raises(pk.PengkError):  # (apart on a sequence shorter than w_a + w_b)
        pk.spacing_summary(hg, hl2, **ok)
    hg2, hl2 = np.zeros(sp.n_bins(G), np.uint64), np.zeros(max_len + 1, np.uint64)
    hg2[4], hl2[8] = 1, 1
    with pytest.raises(pk.PengkError):  # (gap 4 needs 11 bases)
        pk.spacing_summary(hg2, hl2, **ok)


def clean_env():
    return {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PENGK_COMM_TRANSPORT")}


def test_help_lists_the_spacing_flags():
    r = subprocess.run([CLI, "-h"], stdout=subprocess.PIPE, env=clean_env(), timeout=60)
    assert r.returncode == 0
    for flag in (b"--spacing FILE", b"--spacing-pvalue", b"--spacing-max-gap", b"--spacing-motifs"):
        assert flag in r.stdout


@pytest.mark.parametrize("flag,bad", [("--spacing-pvalue", "0"), ("--spacing-pvalue", "1.5"), ("--spacing-pvalue", "abc"),
                                      ("--spacing-pvalue", "nan"), ("--spacing-max-gap", "-1"), ("--spacing-max-gap", "1025"),
                                      ("--spacing-max-gap", "1e2"), ("--spacing-motifs", "1"), ("--spacing-motifs", "65"),
                                      ("--spacing-motifs", "x")])
def test_bad_spacing_values_are_refused(tmp_path, flag, bad):
    r = subprocess.run([CLI, os.path.join(GOLD, "MafK.fasta"), "--spacing", str(tmp_path / "s.tsv"), flag, bad],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=clean_env(), timeout=60)
    assert r.returncode == 4, (flag, bad, r.returncode, r.stderr[-500:])
    assert flag.encode() in r.stderr
    assert not (tmp_path / "s.tsv").exists()
