"""The CPU half of the motif refinement (--refine; include/pengk.h, "motif refinement"): pengk_profile_refine against the
numpy model of tests/motif_refine_model.py on random count tables and at its edges, the model's rounds on a small planted
input, and the flags."""
import os
import subprocess

import numpy as np
import pytest

import peng_motif_amd as pk
import motif_refine_model as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CLI = os.path.join(ROOT, "peng-motif_amd", "host", "peng_motif")
BG = np.array([0.302456, 0.19647, 0.197165, 0.303909], np.float32)


def assert_equal(a, b):
    """to the last bit, matrix included: the model takes log2 from the C library (math.log2), one entry at a time in the
    library's order, so there is no second implementation of it to differ by an ulp (numpy's vectorised log2 may)"""
    assert (a["first"], a["last"], a["sites"]) == (b["first"], b["last"], b["sites"])
    assert a["q"].tobytes() == b["q"].tobytes()
    assert a["ic"].tobytes() == b["ic"].tobytes()
    assert a["pwm"].dtype == np.float32 and a["pwm"].tobytes() == b["pwm"].tobytes()
    assert a["pwm"].shape == (a["last"] - a["first"], 4)


def test_random_count_tables_equal_the_model():
    rng = np.random.default_rng(5)
    kept = 0
    for _ in range(1500):
        w = int(rng.integers(1, 65))
        flank = int(rng.choice([0, 1, 8, 40]))
        n = w + 2 * mr.clamp_flank(w, flank)
        counts = np.zeros((64, 5), np.uint64)
        counts[:n] = rng.integers(0, int(rng.choice([1, 3, 50, 100000, 2 ** 40])) + 1, (n, 5))
        if rng.random() < 0.3:
            counts[rng.random(64) < 0.3] = 0
        bg = rng.dirichlet([5, 5, 5, 5]).astype(np.float32)
        min_ic = float(rng.choice([0, 0.1, 0.25, 1, 2]))
        got = pk.profile_refine(counts, w, flank, bg, min_ic)
        assert_equal(got, mr.profile_refine(counts, w, flank, bg, min_ic))
        kept += got["last"] > got["first"]
    assert kept > 500


def test_no_sites_keeps_nothing():
    counts = np.zeros((64, 5), np.uint64)
    got = pk.profile_refine(counts, 10, 8, BG, 0.25)
    assert_equal(got, mr.profile_refine(counts, 10, 8, BG, 0.25))
    assert (got["first"], got["last"], got["sites"]) == (0, 0, 0) and got["pwm"].shape == (0, 4)
    assert np.all(got["ic"] == 0.0)
    assert got["q"].tobytes() == np.tile(BG.astype(np.float64), (26, 1)).tobytes()  # (the pseudocount alone: bg)


def test_no_column_reaches_the_bound():
    counts = np.zeros((64, 5), np.uint64)
    counts[:26, :4] = [30, 20, 20, 30]  # the background's own composition: ~0 bits everywhere
    got = pk.profile_refine(counts, 10, 8, BG, 0.25)
    assert_equal(got, mr.profile_refine(counts, 10, 8, BG, 0.25))
    assert (got["first"], got["last"]) == (0, 0) and got["sites"] == 100 and got["ic"].max() < 0.01


def test_only_flank_columns_reach_the_bound():
    counts = np.zeros((64, 5), np.uint64)
    counts[:26, :4] = [30, 20, 20, 30]
    counts[2, :4] = [0, 0, 100, 0]
    counts[5, :4] = [0, 100, 0, 0]
    counts[21, :4] = [90, 0, 0, 10]
    got = pk.profile_refine(counts, 10, 8, BG, 0.25)
    assert_equal(got, mr.profile_refine(counts, 10, 8, BG, 0.25))
    assert (got["first"], got["last"]) == (2, 22)  # the motif's own columns 8..17 lie between them and are kept
    left_only = counts.copy()
    left_only[21, :4] = [30, 20, 20, 30]
    got = pk.profile_refine(left_only, 10, 8, BG, 0.25)
    assert_equal(got, mr.profile_refine(left_only, 10, 8, BG, 0.25))
    assert (got["first"], got["last"]) == (2, 6)  # the motif moves wholly into its left flank
    assert [int(np.argmax(r)) for r in got["pwm"][[0, 3]]] == [2, 1]


def test_a_column_with_only_the_fifth_bin():
    """beyond every sequence's end (or all N): no base seen, the background, 0 bits; inside the kept range it stays"""
    counts = np.zeros((64, 5), np.uint64)
    counts[:26, :4] = [0, 0, 100, 0]
    counts[0] = [0, 0, 0, 0, 100]
    counts[12] = [0, 0, 0, 0, 100]
    got = pk.profile_refine(counts, 10, 8, BG, 0.25)
    assert_equal(got, mr.profile_refine(counts, 10, 8, BG, 0.25))
    assert (got["first"], got["last"], got["sites"]) == (1, 26, 100)
    assert got["ic"][0] == 0.0 and got["ic"][12] == 0.0
    assert got["pwm"][11].tobytes() == BG.tobytes()


def test_flank_clamped_at_width_60():
    assert pk.clamp_flank(60, 8) == mr.clamp_flank(60, 8) == 2 and pk.clamp_flank(64, 8) == 0 and pk.clamp_flank(61, 8) == 1
    rng = np.random.default_rng(9)
    counts = np.zeros((64, 5), np.uint64)
    counts[:, :4] = rng.integers(0, 50, (64, 4))
    counts[:, 0] += 200
    got = pk.profile_refine(counts, 60, 8, BG, 0.25)
    assert_equal(got, mr.profile_refine(counts, 60, 8, BG, 0.25))
    assert got["q"].shape == (64, 4) and (got["first"], got["last"]) == (0, 64) and got["pwm"].shape == (64, 4)
    assert got["sites"] == int(counts[2].sum())
    for w in (0, 65):
        with pytest.raises(pk.PengkError):
            pk.profile_refine(counts, w, 8, BG, 0.25)
    with pytest.raises(pk.PengkError):
        pk.profile_refine(counts, 10, 8, np.array([0.5, 0.5, 0.0, 0.0], np.float32), 0.25)


def test_model_rounds_on_a_planted_input():
    """the model's own rounds (site profiles included) on a small input: a 12-column motif regrown from 6 columns"""
    rng = np.random.default_rng(3)
    word = "TGCTGAGTCAGC"
    mot = np.array(["ACGT".index(c) + 1 for c in word], np.uint8)
    seqs = [rng.integers(1, 5, 60).astype(np.uint8) for _ in range(300)]
    for i in range(0, 300, 2):
        p = int(rng.integers(0, 49))
        seqs[i][p:p + 12] = mot
    start = np.full((6, 4), 0.02, np.float32)
    for j, ch in enumerate(word[3:9]):
        start[j, "ACGT".index(ch)] = 0.94
    bg = np.full(4, 0.25, np.float32)
    r = mr.refine(seqs, [start], bg, False, pvalue=1e-3)[0]
    assert (r["left"], r["right"]) == (3, 3) and 1 <= r["rounds"] <= 3 and r["sites"] >= 150
    assert "".join("ACGT"[int(np.argmax(x))] for x in r["pwm"]) == word
    # the rounds stop once a round repeats the last one's range and counts
    again = mr.refine(seqs, [start], bg, False, pvalue=1e-3, iterations=10)[0]
    assert again["rounds"] < 10 and again["pwm"].shape == (12, 4)
    # no site at all: the found matrix, no round
    none = mr.refine([s for s in seqs[1::2]], [start], bg, False, pvalue=1e-9)[0]
    assert none["rounds"] == 0 and none["sites"] == 0 and none["pwm"].tobytes() == start.tobytes()


def clean_env():
    return {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PENGK_COMM_TRANSPORT")}


def test_help_lists_the_refine_flags():
    r = subprocess.run([CLI, "-h"], stdout=subprocess.PIPE, env=clean_env(), timeout=60)
    assert r.returncode == 0
    for flag in [b"--refine FILE", b"--refine-pvalue", b"--refine-flank", b"--refine-iterations", b"--refine-min-ic"]:
        assert flag in r.stdout, flag


@pytest.mark.parametrize("bad", ["0", "-1e-4", "1.5", "abc", "nan", "1e-4x"])
def test_bad_refine_pvalue_is_refused(tmp_path, bad):
    """as --sites-pvalue and --centrality-pvalue: the help, the flag named in an error line, exit status 4, no file"""
    r = subprocess.run([CLI, os.path.join(GOLD, "MafK.fasta"), "--refine", str(tmp_path / "r.meme"), "--refine-pvalue", bad],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=clean_env(), timeout=60)
    assert r.returncode == 4, (bad, r.returncode, r.stderr[-500:])
    assert b"--refine-pvalue must be a number in (0, 1]" in r.stderr
    assert not (tmp_path / "r.meme").exists()


@pytest.mark.parametrize("flag,bad", [("--refine-flank", "-1"), ("--refine-flank", "x"), ("--refine-flank", "2.5"),
                                      ("--refine-iterations", "0"), ("--refine-iterations", "3x"), ("--refine-min-ic", "-0.1"),
                                      ("--refine-min-ic", "nan"), ("--refine-min-ic", "bits")])
def test_bad_refine_settings_are_refused(tmp_path, flag, bad):
    r = subprocess.run([CLI, os.path.join(GOLD, "MafK.fasta"), "--refine", str(tmp_path / "r.meme"), flag, bad],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=clean_env(), timeout=60)
    assert r.returncode == 4, (flag, bad, r.returncode, r.stderr[-500:])
    assert flag.encode() in r.stderr
    assert not (tmp_path / "r.meme").exists()
