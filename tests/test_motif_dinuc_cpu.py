"""The first-order motif model on the CPU (pengk_dinuc_model; include/pengk.h, "first-order motif models") against the numpy
model of tests/motif_dinuc_model.py bit for bit, the model's two versions of the counts and of the scan against each other,
and the planted dependency on the model alone (tests/test_gpu_motif_dinuc.py asks the device for the same)."""
import numpy as np
import pytest

import peng_motif_amd as pk
import motif_centrality_model as mc
import motif_dinuc_model as md
import motif_refine_model as mr
import motif_score_model as ms

UNIFORM = np.full(4, 0.25, np.float32)


def random_bg(rng):
    g0 = rng.dirichlet(np.full(4, 20.0)).astype(np.float32)
    g1 = rng.dirichlet(np.full(4, 20.0), 4).astype(np.float32).reshape(16)
    return g0, g1


def consistent_counts(rng, W, scale, outside=True):
    """W x 5 and W x 17 counts as sites give them: the pair counts of column c have the single counts of column c as
    their column sums wherever both letters are bases"""
    k2 = rng.integers(0, scale, (W, 17)).astype(np.uint64)
    if not outside:
        k2[:, 16] = 0
    k2[0] = 0
    k1 = np.zeros((W, 5), np.uint64)
    k1[:, :4] = k2[:, :16].reshape(W, 4, 4).sum(axis=1)
    k1[:, 4] = k2[:, 16]
    k1[0] = rng.integers(0, scale, 5)
    return k1, k2


def assert_equal_bitwise(got, want):
    for k in ("q0", "q1", "mi", "S0", "D1", "D0"):
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
    assert got["sites"] == want["sites"] and got["flank"] == want["flank"]


def both_models(k1, k2, w, flank, g0, g1, alpha):
    got, want = pk.dinuc_model(k1, k2, w, flank, g0, g1, alpha), md.dinuc_model(k1, k2, w, flank, g0, g1, alpha)
    assert_equal_bitwise(got, want)
    return got


@pytest.mark.parametrize("alpha", [1e-3, 1.0, 20.0, 1e6])
def test_model_equals_the_numpy_model_on_random_counts(alpha):
    rng = np.random.default_rng(7)
    for w, flank, scale in [(2, 0, 50), (10, 0, 1000), (10, 3, 1000), (13, 40, 5), (30, 40, 100000), (64, 0, 3), (1, 0, 10)]:
        g0, g1 = random_bg(rng)
        F = md.clamp_flank(w, flank)
        k1, k2 = consistent_counts(rng, w + 2 * F, scale)
        r = both_models(k1, k2, w, flank, g0, g1, alpha)
        assert r["flank"] == F and r["q0"].shape == (w + 2 * F, 4)
        # every conditional row is a distribution, row 0 repeats q0[0]
        assert np.allclose(r["q1"].reshape(-1, 4, 4).sum(axis=2), 1.0, atol=1e-12)
        assert np.array_equal(r["q1"][0].reshape(4, 4), np.repeat(r["q0"][0][None], 4, axis=0))
        assert not r["D1"][0].any() and not r["D0"][0].any() and r["mi"][0] == 0.0
        assert np.all(np.abs(r["D1"]) <= 2000) and np.all(np.abs(r["D0"]) <= 2000)


def test_model_edges():
    rng = np.random.default_rng(8)
    g0, g1 = random_bg(rng)
    W = 8
    # all-zero counts: the background itself, no information, no sites
    z = both_models(np.zeros((W, 5), np.uint64), np.zeros((W, 17), np.uint64), W, 0, g0, g1, 20.0)
    assert z["sites"] == 0 and not z["mi"].any() and not z["S0"].any()
    assert np.array_equal(z["q0"], np.repeat(g0.astype(np.float64)[None], W, axis=0))
    # a column whose pair counts sit in one cell: no information there (one row, one column), and a sharp conditional
    k1, k2 = consistent_counts(rng, W, 500, outside=False)
    k2[3] = 0
    k2[3, 4 * 2 + 1] = 1234
    k1[3] = [0, 1234, 0, 0, 0]
    r = both_models(k1, k2, W, 0, g0, g1, 1e-3)
    assert r["mi"][3] == 0.0 and r["q1"][3, 4 * 2 + 1] > 0.999
    # n2 = 0 for one a: that row of the conditionals is q0 itself (alpha cancels up to rounding)
    k1, k2 = consistent_counts(rng, W, 500, outside=False)
    k2[5, 4:8] = 0
    k1[5, :4] = k2[5, :16].reshape(4, 4).sum(axis=0)
    r = both_models(k1, k2, W, 0, g0, g1, 20.0)
    assert np.allclose(r["q1"][5, 4:8], r["q0"][5], rtol=1e-15, atol=0)
    # counts near 2^40: the integer sums are exact, the products of the mutual information are taken in double
    k1, k2 = consistent_counts(rng, W, 7, outside=False)
    k2[1:] += np.uint64(2 ** 40)
    k2[:, 16] = 0
    k1[:, :4] = k2[:, :16].reshape(W, 4, 4).sum(axis=1)
    k1[0] = [2 ** 40 + 1, 2 ** 40, 2 ** 40 + 5, 3, 0]
    r = both_models(k1, k2, W, 0, g0, g1, 20.0)
    assert r["sites"] == int(k1[0].sum()) and np.all(np.abs(r["mi"]) < 1e-9)
    # a perfect dependency carries two bits at four equally likely pairs
    k2 = np.zeros((2, 17), np.uint64)
    for a in range(4):
        k2[1, 4 * a + (3 - a)] = 100
    k1 = np.array([[100] * 4 + [0], [100] * 4 + [0]], np.uint64)
    r = both_models(k1, k2, 2, 0, UNIFORM, np.full(16, 0.25, np.float32), 20.0)
    assert r["mi"][1] == 2.0 and r["sites"] == 400


def test_zeroth_order_scores_do_not_depend_on_the_letter_before_under_a_zeroth_order_background():
    rng = np.random.default_rng(9)
    g0, _ = random_bg(rng)
    k1, k2 = consistent_counts(rng, 12, 300)
    r = both_models(k1, k2, 12, 0, g0, np.tile(g0, 4), 20.0)
    D0 = r["D0"].reshape(12, 4, 4)
    assert np.array_equal(D0, np.repeat(D0[:, :1], 4, axis=1))
    assert not np.array_equal(r["D1"], r["D0"])


def test_argument_errors():
    k1, k2 = np.zeros((4, 5), np.uint64), np.zeros((4, 17), np.uint64)
    g1 = np.full(16, 0.25, np.float32)
    for w, flank, g0, gg1, alpha in [(0, 0, UNIFORM, g1, 20.0), (65, 0, UNIFORM, g1, 20.0), (4, -1, UNIFORM, g1, 20.0),
                                     (4, 0, UNIFORM, g1, 0.0), (4, 0, UNIFORM, g1, -1.0), (4, 0, UNIFORM, g1, float("nan")),
                                     (4, 0, np.array([0.5, 0.5, 0, 0], np.float32), g1, 20.0),
                                     (4, 0, UNIFORM, np.zeros(16, np.float32), 20.0)]:
        q0 = np.zeros((64, 4))
        rc = pk.lib().pengk_dinuc_model(k1.ctypes.data, k2.ctypes.data, w, flank, np.ascontiguousarray(g0).ctypes.data,
                                        np.ascontiguousarray(gg1).ctypes.data, alpha, q0.ctypes.data, None, None, None, None,
                                        None, None)
        assert rc == pk.ERR_ARG, (w, flank, alpha)
    # every output may be NULL
    assert pk.lib().pengk_dinuc_model(k1.ctypes.data, k2.ctypes.data, 4, 0, UNIFORM.ctypes.data, g1.ctypes.data, 20.0, None, None,
                                      None, None, None, None, None) == pk.PENGK_OK


# ---- the model's own two versions ------------------------------------------------------------------------------------------
def random_model(rng, w):
    S0 = rng.integers(-300, 301, 4).astype(np.int32)
    D = rng.integers(-300, 301, (w, 16)).astype(np.int32)
    D[rng.random((w, 16)) < 0.04] = -2000
    D[rng.random((w, 16)) < 0.02] = 2000
    D[0] = 0
    return S0, D


def equal_length_codes(rng, n, L):
    codes = rng.integers(1, 5, (n, L)).astype(np.uint8)
    codes[rng.random((n, L)) < 0.01] = 0
    return codes


@pytest.mark.parametrize("both", [True, False], ids=["both", "plus"])
def test_scan_models_agree_and_the_degenerate_model_is_the_pwm_scan(both):
    rng = np.random.default_rng(21 + both)
    for w, L in [(1, 9), (2, 40), (5, 33), (9, 64), (17, 70), (33, 100), (64, 130), (12, 7)]:
        codes = equal_length_codes(rng, 23, L)
        seqs = list(codes)
        S0, D = random_model(rng, w)
        want = md.best_scores(seqs, S0, D, both)
        assert np.array_equal(md.best_scores_batch(codes, S0, D, both), want)
        flat, offs = ms.flatten(seqs)
        assert np.array_equal(md.best_scores_mixed(flat, offs, S0, D, both), want)
        # the definition itself, window by window, on one sequence
        c = codes[0].astype(np.int64)
        sc = []
        for p in range(L - w + 1):
            x = c[p:p + w] - 1
            if np.all(x >= 0):
                sc.append(md.window_score(x, S0, D))
                if both:
                    sc.append(md.window_score(3 - x[::-1], S0, D))
        assert want[0] == (max(sc) if sc else md.SENTINEL)
        S = rng.integers(-300, 301, (w, 4)).astype(np.int32)
        assert np.array_equal(md.best_scores(seqs, *md.degenerate(S), both), ms.best_scores(seqs, S, both))
        lo, hi = md.score_range(S0, D)
        ok = want != md.SENTINEL
        assert np.all(want[ok] >= lo) and np.all(want[ok] <= hi)


def test_pair_profile_models_agree_and_sum_to_the_single_profile():
    rng = np.random.default_rng(31)
    n, L = 300, 60
    codes = equal_length_codes(rng, n, L)
    seqs = list(codes)
    for w, flank in [(2, 0), (7, 3), (10, 40), (30, 40)]:
        S = rng.integers(-300, 301, (w, 4)).astype(np.int32)
        best, site = mc.best_sites(seqs, S, True, 3)
        t = int(np.percentile(best[best > ms.SENTINEL], 40))
        k2 = md.pair_profile(seqs, best, site, w, t, flank)
        assert k2.tobytes() == md.pair_profile_batch(codes, best, site, w, t, flank).tobytes()
        flat, offs = ms.flatten(seqs)
        assert k2.tobytes() == md.pair_profile_mixed(flat, offs, best, site, w, t, flank).tobytes()
        k1 = mr.site_profile(seqs, best, site, w, t, flank)
        W = w + 2 * md.clamp_flank(w, flank)
        assert not k2[0].any() and not k2[W:].any()
        assert np.all(k2[1:W].sum(axis=1) == k1[0].sum())
        # where both letters are bases the pair counts' margins are the single counts
        assert np.all(k2[1:W, :16].reshape(-1, 4, 4).sum(axis=1) <= k1[1:W, :4])
        assert np.all(k2[1:W, :16].reshape(-1, 4, 4).sum(axis=2) <= k1[0:W - 1, :4])
        inner = slice(md.clamp_flank(w, flank) + 1, md.clamp_flank(w, flank) + w)
        assert not k2[inner, 16].any()
        assert np.array_equal(k2[inner, :16].reshape(-1, 4, 4).sum(axis=1), k1[inner, :4])


# ---- a planted dependency --------------------------------------------------------------------------------------------------
PLANT_CONSENSUS = "TGCA??CTGA"  # columns 5|6 (1-based) are AT or GC, half each
PLANT_PAIR = 6                  # the pair's second member, 1-based


def planted_seqs(seed, dependent, n=2000, L=100):
    """2000 x 100 bp of uniform background, every sequence planted once on a random strand: eight fixed columns, each
    the consensus with probability 0.7, else one of the three other bases at random; columns 5|6 AT or GC, half each
    (dependent), or A/G and T/C drawn independently, half each: the same marginals and no dependency (the control)"""
    rng = np.random.default_rng(seed)
    seqs = [rng.integers(1, 5, L).astype(np.uint8) for _ in range(n)]
    for c in seqs:
        mot = np.empty(10, np.uint8)
        for j, ch in enumerate(PLANT_CONSENSUS):
            if ch == "?":
                continue
            b = "ACGT".index(ch)
            mot[j] = b + 1 if rng.random() < 0.7 else 1 + (b + 1 + int(rng.integers(0, 3))) % 4
        first = int(rng.integers(0, 2))
        second = first if dependent else int(rng.integers(0, 2))
        mot[4] = (1, 3)[first]   # A or G
        mot[5] = (4, 2)[second]  # T or C
        p = int(rng.integers(0, L - 9))
        c[p:p + 10] = mot if rng.random() < 0.5 else 5 - mot[::-1]
    return seqs


def planted_start_pwm():
    pwm = np.full((10, 4), 0.1, np.float32)
    for j, ch in enumerate(PLANT_CONSENSUS):
        if ch != "?":
            pwm[j, "ACGT".index(ch)] = 0.7
    pwm[4] = [0.45, 0.05, 0.45, 0.05]
    pwm[5] = [0.05, 0.45, 0.05, 0.45]
    return pwm


def planted_negatives(seqs, seed=1):
    """as many uniform sequences of the same lengths: the order-0 sample of the scoring step, as byte codes"""
    return [x + 1 for x in ms.sample([len(s) for s in seqs], seed, 0, 0, ms.thresholds([UNIFORM], 0))]


PLANT_SEED = 1


def planted_analysis(dependent, seed=PLANT_SEED):
    seqs = planted_seqs(seed, dependent)
    S = ms.log_odds(planted_start_pwm(), UNIFORM)
    return md.analyse(seqs, planted_negatives(seqs), S, 0, UNIFORM, np.full(16, 0.25, np.float32), True, pvalue=1e-3, flank=0,
                      alpha=20.0)


def test_the_step_by_the_vectorised_versions_is_the_step():
    seqs = planted_seqs(3, True, n=300, L=60)
    seqs[5] = seqs[5][:41]  # (a second length class)
    seqs[7][10:14] = 0
    S = ms.log_odds(planted_start_pwm(), UNIFORM)
    g0, g1 = random_bg(np.random.default_rng(5))
    for both, flank in [(True, 0), (False, 4)]:
        a = md.analyse(seqs, planted_negatives(seqs), S, 2, g0, g1, both, 1e-3, flank, 20.0)
        b = md.analyse(seqs, planted_negatives(seqs), S, 2, g0, g1, both, 1e-3, flank, 20.0, batch=True)
        assert a["sites"] > 20 and sorted(a) == sorted(b)
        for k in a:
            assert (a[k].tobytes() == b[k].tobytes()) if isinstance(a[k], np.ndarray) else a[k] == b[k], k
        assert md.report_line("X", 3, a) == md.report_line("X", 3, b) and md.models_block("X", a) == md.models_block("X", b)


def assert_planted_conditions(dep, ctl):
    """the issue's conditions: a planted site carries exactly 1 bit at the pair and the control 0; the margins cover the
    sites that are not planted ones"""
    assert dep["mi_max_pair"] == PLANT_PAIR
    assert dep["mi_max"] >= 0.5 and ctl["mi_max"] <= 0.1
    assert dep["gain"] > 0
    assert dep["gain"] > ctl["gain"]


def test_planted_dependency_on_the_model():
    dep, ctl = planted_analysis(True), planted_analysis(False)
    print("dependent: sites %d mi_max %.4f pair %d auc0 %.6f auc1 %.6f gain %+.6f" % (
        dep["sites"], dep["mi_max"], dep["mi_max_pair"], dep["auc0"], dep["auc1"], dep["gain"]))
    print("control:   sites %d mi_max %.4f pair %d auc0 %.6f auc1 %.6f gain %+.6f" % (
        ctl["sites"], ctl["mi_max"], ctl["mi_max_pair"], ctl["auc0"], ctl["auc1"], ctl["gain"]))
    assert dep["sites"] > 50 and ctl["sites"] > 50
    assert_planted_conditions(dep, ctl)
