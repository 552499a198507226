"""The GC-stratified null on the CPU (tests/strata_stats_model.py): the constructed cases hold the classes they were built
for, one non-empty stratum gives the plain sweep's bits, the strata's counters sum to the oracle's on inputs without invalid
bases, and the definition does what it is for on the scenario of the README's table -- 20 000 x 100 bp, half at 30 % and
half at 70 % GC: against one Markov model every seed is composition, against the stratified null none is, and a planted
motif keeps its seeds.  (Figures of the model at G = 10, W = 8, both strands, order 2, seeds 1 / 2 / 3 -- README,
"--stratified-background".)"""
import os
import subprocess

import numpy as np
import pytest

import control_stats_model as cm
import strata_stats_model as sm
import table_edges_model as tm
import peng_motif_amd as pk
from oracle import oracle as po


def test_symbols_and_bindings():
    for name in ("pengk_strata_bg_count", "pengk_pattern_stats_strata"):
        assert hasattr(pk.lib(), name) and name in pk.EXPORTS


# ---- the counters -----------------------------------------------------------------------------------------------------------
def random_seqs(seed, lengths, invalid=0.0):
    rng = np.random.default_rng(seed)
    out = []
    for L in lengths:
        c = rng.integers(1, 5, L).astype(np.uint8)
        if invalid:
            c[rng.random(L) < invalid] = 0
        out.append(c)
    return out


def test_counters_of_the_strata_sum_to_the_oracles_on_inputs_without_invalid_bases():
    seqs = random_seqs(1, [0, 1, 2, 3, 31, 32, 33, 64, 65, 200] * 30)
    for G in (1, 4, 10, 16):
        s = sm.gc_strata(seqs, G)
        assert (s[np.array([len(c) for c in seqs]) == 0] == sm.NONE).all()
        bg, win = sm.bg_count(seqs, s, G, 8)
        assert np.array_equal(bg.sum(axis=0).astype(np.int64), po.bg_counts(*sm._flatten(seqs), 2))
        assert int(win.sum()) == sum(max(len(c) - 7, 0) for c in seqs)
        assert G == 1 or (bg[:, :4].sum(axis=1) > 0).sum() > 1


def test_counters_by_hand():
    # ACGNTTA: A C G | T T A -- the base behind the N starts over at order 0
    c = cm.encode("ACG") .tolist() + [0] + cm.encode("TTA").tolist()
    bg, win = sm.bg_count([np.array(c, np.uint8)], [0], 1, 2)
    assert bg[0, :4].tolist() == [2, 1, 1, 2]
    two = {4 + 0 * 4 + 1: 1, 4 + 1 * 4 + 2: 1, 4 + 3 * 4 + 3: 1, 4 + 3 * 4 + 0: 1}      # AC CG TT TA
    three = {20 + 0 * 16 + 1 * 4 + 2: 1, 20 + 3 * 16 + 3 * 4 + 0: 1}                    # ACG TTA
    want = np.zeros(84, np.uint64)
    want[:4] = [2, 1, 1, 2]
    for k, v in {**two, **three}.items():
        want[k] = v
    assert np.array_equal(bg[0], want)
    assert int(win[0]) == 4  # AC CG | TT TA
    # all_valid: the N is a valid A
    bg, win = sm.bg_count([np.array(c, np.uint8)], [0], 1, 2, all_valid=True)
    assert bg[0, :4].tolist() == [3, 1, 1, 2] and int(win[0]) == 6 and int(bg[0, 20:].sum()) == 5
    # a stratum out of range, and 0xFFFF, count nowhere
    bg, win = sm.bg_count([np.array(c, np.uint8)] * 2, [3, sm.NONE], 3, 2)
    assert not bg.any() and not win.any()


# ---- the mixture ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("both", [False, True], ids=["plus", "both"])
def test_one_non_empty_stratum_gives_the_plain_sweeps_bits(both):
    W = 6
    Vs = sm.stratum_V(3)
    p = sm.markov_tables(W, Vs, both, 2)
    counts = tm.edge_counts(W, mirrored=bool(both), salt=5)
    for s in range(3):
        for w in sm.WEIGHTS[1:] + (2 ** 64 - 1,):
            windows = [0, 0, 0]
            windows[s] = w
            m, e, lp, z = sm.sweep(W, counts, 12345, p, windows, 2)
            e0, lp0, z0 = po.stats(W, counts.astype(np.uint64), p[s][2], 12345)
            for o in range(3):
                assert m[o].tobytes() == p[s][o].tobytes(), (s, w, o)
            assert e.tobytes() == e0.tobytes() and z.tobytes() == z0.tobytes() and lp.tobytes() == lp0.tobytes()


def test_mixture_is_a_weighted_mean_rounded_once():
    a = np.array([0.25, 1e-30, 0.5], np.float32)
    b = np.array([0.75, 3e-30, 0.5], np.float32)
    m = sm.mixture([a, b], [1, 3])
    assert m[0] == np.float32(0.625) and m[2] == np.float32(0.5)
    assert m[1] ==np.float32((np.float64(a[1]) + np.float64(3) * np.float64(b[1])) / np.float64(4))
    assert sm.mixture([a, b], [0, 7]).tobytes() == b.tobytes()
    with pytest.raises(AssertionError):
        sm.mixture([a, b], [0, 0])


@pytest.mark.parametrize("both", [False, True], ids=["plus", "both"])
@pytest.mark.parametrize("W", [2, 4, 8])
def test_constructed_cases_hold_their_classes(W, both):
    """over a pattern length: every S, every weight value, a case with one non-zero weight, cases whose mixture differs from
    every stratum's own table, and under a control the classes of tests/control_stats_model.py against the MIXED null"""
    specs = sm.small_cases(W, both)
    assert {sp[0] for sp in specs} == set(sm.N_STRATA)
    assert {int(v) for sp in specs for v in sp[1]} == set(sm.WEIGHTS)
    assert any(np.count_nonzero(sp[1]) == 1 and sp[0] > 1 for sp in specs)
    assert {(sp[3], sp[4]) for sp in specs} == set(tm.legal_orders(W))
    seen = set()
    mixed_differs = False
    for sp in specs:
        c = sm.case(W, both, sp)
        S, w, k = c["S"], c["windows"], c["k"]
        assert c["V"].shape == (S, 84) and len(w) == S and any(int(v) for v in w)
        p = sm._markov(W, both, S)
        if np.count_nonzero(w) > 1:
            mixed_differs |= all(c["plain"][k].tobytes() != p[s][k].tobytes() for s in range(S))
        for name, mask in tm.count_classes(c).items():
            if mask.any():
                seen.add(name)
        if c["ctrl"] is not None:
            for name, mask in cm.class_masks(c["plain"], k, c["ctrl"], c["Lc"], c["a"]).items():
                if mask.any():
                    seen.add(name)
    assert mixed_differs
    assert {"n == 0", "0 < n <= 5", "n == 2^32 - 1", "c = 0", "c = 2^32 - 1", "control wins at order k", "Markov wins at order k",
            "q_k differs from p_k"} <= seen
    if W >= 4:
        assert {"n > 5, (float)n > mu", "n > 5, (float)n <= mu", "share == p_k in fp64"} <= seen


# ---- the report -------------------------------------------------------------------------------------------------------------
def test_report_names_the_strata_that_fall_back_to_the_global_model():
    seqs = sm.mixed(5, 400)
    st = sm.stratified(seqs, seqs, 8, G=10, min_bases=10_000)
    lines = sm.report(st).splitlines()
    assert lines[0] == sm.REPORT_HEADER.rstrip("\n") and len(lines) == 11
    used = [l.split("\t")[6] for l in lines[1:]]
    assert "own" in used and "global" in used
    assert sum(int(l.split("\t")[3]) for l in lines[1:]) == 400
    assert sum(int(l.split("\t")[4]) for l in lines[1:]) == 400 * 93
    g = po.bg_V(po.bg_counts(*sm._flatten(seqs), 2), 2)
    for s in range(10):
        assert st["own"][s] == (st["model_bases"][s] >= 10_000)
        if not st["own"][s]:
            assert st["V"][s].tobytes() == g.tobytes()


# ---- the scenario -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nothing_planted():
    return {seed: sm.seeds(sm.mixed(seed)) for seed in (1, 2, 3)}


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_mixed_composition_seeds_are_composition_and_the_stratified_null_has_none(nothing_planted, seed):
    markov, strat, (z0, z1) = nothing_planted[seed]
    print("seed %d, nothing planted: Markov null %d seeds, stratified null %d; largest z %.1f -> %.1f" % (
        seed, len(markov), len(strat), z0, z1))
    assert len(markov) >= 50
    assert all(sm.gc_fraction(w) <= 0.25 or sm.gc_fraction(w) >= 0.75 for w in markov)
    assert len(strat) == 0


def test_a_planted_motif_keeps_its_seeds_and_loses_the_composition():
    markov, strat, (z0, z1) = sm.seeds(sm.mixed(1, planted=True))
    of_motif = [w for w in markov if cm.shares_6mer(w, sm.MOTIF)]
    print("seed 1, %s in 5 %%: Markov null %d seeds, %d of the motif; stratified null %d seeds; largest z %.0f -> %.0f" % (
        sm.MOTIF, len(markov), len(of_motif), len(strat), z0, z1))
    assert strat and all(cm.shares_6mer(w, sm.MOTIF) for w in strat)
    assert len(strat) >= len(of_motif)


def test_a_single_composition_gives_no_seed_either_way():
    markov, strat, (z0, z1) = sm.seeds(sm.mixed(1, gc=(0.5, 0.5)))
    print("seed 1, 50 %% GC throughout: largest z %.1f (Markov), %.1f (stratified)" % (z0, z1))
    assert not markov and not strat


# ---- the CLI's flags ---------------------------------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "peng-motif_amd", "host", "peng_motif")
GOLD = os.path.join(ROOT, "tests", "golden")


def clean_env():
    return {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PENGK_COMM_TRANSPORT")}


def test_help_lists_the_stratified_flags():
    r = subprocess.run([CLI, "-h"], stdout=subprocess.PIPE, env=clean_env(), timeout=60)
    assert r.returncode == 0
    for flag in (b"--stratified-background", b"--stratified-gc-bins INT", b"--stratified-min-bases INT", b"--stratified-report FILE"):
        assert flag in r.stdout, flag


@pytest.mark.parametrize("extra,message", [
    (["--stratified-background", "--stratified-gc-bins", "0"], b"--stratified-gc-bins must be an integer in [1, 16]"),
    (["--stratified-background", "--stratified-gc-bins", "17"], b"--stratified-gc-bins must be an integer in [1, 16]"),
    (["--stratified-background", "--stratified-gc-bins", "4x"], b"--stratified-gc-bins must be"),
    (["--stratified-background", "--stratified-min-bases", "-1"], b"--stratified-min-bases must be"),
    (["--stratified-background", "--stratified-min-bases", "many"], b"--stratified-min-bases must be"),
    (["--stratified-gc-bins", "4"], b"--stratified-gc-bins requires --stratified-background"),
    (["--stratified-min-bases", "5"], b"--stratified-min-bases requires --stratified-background"),
    (["--stratified-report", "x.tsv"], b"--stratified-report requires --stratified-background"),
], ids=["bins_0", "bins_17", "bins_not_a_number", "min_bases_negative", "min_bases_not_a_number", "bins_alone", "min_bases_alone",
        "report_alone"])
def test_flag_errors_exit_with_4_before_the_input_is_read(tmp_path, extra, message):
    r = subprocess.run([CLI, os.path.join(GOLD, "MafK.fasta"), "-o", str(tmp_path / "o.meme")] + extra, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, env=clean_env(), timeout=60)
    assert r.returncode == 4 and message in r.stderr and b"ERROR" in r.stderr, (r.returncode, r.stderr.decode()[-500:])
    assert not (tmp_path / "o.meme").exists()
