"""CPU checks of the motif sites (--sites): the numpy model's tail p-values against brute force, its thresholds at the
edges, the library's tail and threshold entries against the model bit for bit, the TSV rendering, and the CLI's flags.
No device compute here."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import peng_motif_amd as pk
import motif_sites_model as mst

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "peng-motif_amd", "host", "peng_motif")
GOLD = os.path.join(ROOT, "tests", "golden")


def random_S(rng, w, lo=-300, hi=300):
    S = rng.integers(lo, hi + 1, (w, 4)).astype(np.int32)
    S[rng.random((w, 4)) < 0.05] = -2000
    return S


def random_bg(rng):
    return rng.dirichlet(np.ones(4) * 3).astype(np.float32)


def brute_tail(S, bg):
    """P(score >= t) by enumerating all 4^w windows"""
    w = S.shape[0]
    b = bg.astype(np.float64)
    idx = np.array(list(itertools.product(range(4), repeat=w)), np.int64)
    sc = S[np.arange(w)[None, :], idx].sum(axis=1)
    pr = np.prod(b[idx], axis=1)
    lo, hi = int(S.min(axis=1).sum()), int(S.max(axis=1).sum())
    mass = np.zeros(hi - lo + 1)
    np.add.at(mass, sc - lo, pr)
    return lo, np.cumsum(mass[::-1])[::-1]


@pytest.mark.parametrize("w", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("seed", range(3))
def test_model_tail_equals_brute_force(w, seed):
    rng = np.random.default_rng(100 * w + seed)
    S, bg = random_S(rng, w), random_bg(rng)
    lo, tail = mst.tail_pvalues(S, bg)
    blo, btail = brute_tail(S, bg)
    assert lo == blo and len(tail) == len(btail)
    ok = btail > 0
    assert np.all(np.abs(tail[ok] - btail[ok]) <= 1e-12 * btail[ok])
    assert np.all(tail[~ok] == 0.0)
    assert abs(tail[0] - float(np.sum(bg.astype(np.float64))) ** w) < 1e-12  # (float32 frequencies sum to 1 only roughly)


@pytest.mark.parametrize("w", [1, 4, 10, 21, 64])
@pytest.mark.parametrize("seed", range(3))
def test_library_tail_equals_model_bits(w, seed):
    rng = np.random.default_rng(7 * w + seed)
    S = random_S(rng, w, -400, 400)
    S[rng.random((w, 4)) < 0.02] = 2000
    bg = random_bg(rng)
    lo, tail = pk.score_tail_pvalues(S, bg)
    mlo, mtail = mst.tail_pvalues(S, bg)
    assert lo == mlo and tail.tobytes() == mtail.tobytes()


def test_threshold_is_the_smallest_qualifying_integer():
    rng = np.random.default_rng(5)
    for _ in range(30):
        w = int(rng.integers(1, 12))
        S, bg = random_S(rng, w), random_bg(rng)
        lo, tail = mst.tail_pvalues(S, bg)
        hi = lo + len(tail) - 1
        for p in [1.0, 0.5, 1e-2, 1e-4, 1e-9, float(tail[-1]), float(tail[-1]) * 0.5, float(tail[len(tail) // 2])]:
            t = mst.threshold(lo, tail, p)
            assert pk.score_threshold(tail, lo, p) == t
            if t <= hi:
                assert tail[t - lo] <= p and (t == lo or tail[t - 1 - lo] > p)
            else:
                assert t == hi + 1 and tail[-1] > p  # (below the smallest tail: no site)


def test_threshold_edges():
    S = np.array([[100, -2000, 0, -2000], [-2000, -2000, 50, -2000]], np.int32)
    bg = np.array([0.25, 0.25, 0.25, 0.25], np.float32)
    lo, tail = mst.tail_pvalues(S, bg)
    assert lo == -4000
    # P = 1: the lowest score qualifies (its tail is the whole mass, 1 exactly for these powers of two)
    assert mst.threshold(lo, tail, 1.0) == lo == pk.score_threshold(tail, lo, 1.0)
    # the top score 150 (A then G) has P = 1/16, and so has every t in (50, 150]: the smallest of them is 51
    assert tail[150 - lo] == 1 / 16 and tail[51 - lo] == 1 / 16 and tail[50 - lo] > 1 / 16
    assert mst.threshold(lo, tail, 1 / 16) == 51 == pk.score_threshold(tail, lo, 1 / 16)
    assert mst.threshold(lo, tail, 0.01) == 151 == pk.score_threshold(tail, lo, 0.01)
    # -2000 entries are scores like any other: P(>= 50) = P(C in column 2) * P(A or G in column 1)
    assert tail[50 - lo] == 1 / 8
    assert tail[-1900 - lo] == 5 / 16  # (150, 50 and A followed by a -2000 base)


@pytest.mark.parametrize("p", [0.0, -1e-4, 1.5, float("nan")])
def test_library_threshold_refuses_bad_p(p):
    with pytest.raises(pk.PengkError):
        pk.score_threshold(np.ones(3), 0, p)


def test_render_orders_and_formats():
    seqs = [np.array([1, 2, 3, 4, 1, 2, 3, 4], np.uint8), np.array([4, 4, 0, 1, 1], np.uint8)]
    S = np.array([[100, -100, -100, -100], [-100, 100, -100, -100]], np.int32)  # "AC"; its reverse complement is "GT"
    bg = np.full(4, 0.25, np.float32)
    txt = mst.render(seqs, ["s1", "s2"], ["AC"], [S], bg, 1.0, True)
    lines = txt.splitlines()
    assert lines[0] + "\n" == mst.HEADER
    rows = [l.split("\t") for l in lines[1:]]
    # every valid window of both strands at P = 1: 7 + 7 on s1, 2 + 2 on s2 (the windows over the N skipped)
    assert len(rows) == 18
    assert rows[0] == ["1", "AC", "s1", "1", "2", "+", "2.00", "0.0625", "AC"]
    assert rows[1][:6] == ["1", "AC", "s1", "1", "2", "-"] and rows[1][8] == "GT"
    assert [r[3] for r in rows[:14]] == [str(1 + k // 2) for k in range(14)]
    assert rows[-1][2:6] == ["s2", "4", "5", "-"] and rows[-1][8] == "TT"
    assert mst.fmt_score(-5) == "-0.05" and mst.fmt_score(-150) == "-1.50" and mst.fmt_score(0) == "0.00"


def clean_env():
    return {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PENGK_COMM_TRANSPORT")}


def test_help_lists_the_sites_flags():
    r = subprocess.run([CLI, "-h"], stdout=subprocess.PIPE, env=clean_env(), timeout=60)
    assert r.returncode == 0
    assert b"--sites FILE" in r.stdout and b"--sites-pvalue" in r.stdout


@pytest.mark.parametrize("bad", ["0", "-1e-4", "1.5", "abc", "nan", "1e-4x"])
def test_bad_sites_pvalue_is_refused(tmp_path, bad):
    r = subprocess.run([CLI, os.path.join(GOLD, "MafK.fasta"), "--sites", str(tmp_path / "s.tsv"), "--sites-pvalue", bad],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=clean_env(), timeout=60)
    assert r.returncode == 4, (bad, r.returncode, r.stderr[-500:])
    assert b"--sites-pvalue" in r.stderr
    assert not (tmp_path / "s.tsv").exists()
