"""CPU checks of the motif scoring's numpy model (tests/motif_score_model.py) and of the library's host-side pieces:
the scan layout builder and pengk_score_summary (zoops_score / occur) against the model.  No device compute here."""
import itertools

import numpy as np
import pytest

import peng_motif_amd as pk
import motif_score_model as ms


def brute_auc(pos, neg):
    """P(pos > neg) + P(pos == neg) / 2 over all pairs"""
    gt = sum(1 for a, b in itertools.product(pos, neg) if a > b)
    eq = sum(1 for a, b in itertools.product(pos, neg) if a == b)
    return (gt + 0.5 * eq) / (len(pos) * len(neg))


@pytest.mark.parametrize("seed", range(12))
def test_auc_equals_pair_count_with_ties_and_sentinels(seed):
    rng = np.random.default_rng(seed)
    lo, hi = -7, 5
    pos = rng.integers(lo, hi + 1, rng.integers(1, 40))
    neg = rng.integers(lo, hi + 1, rng.integers(1, 40))
    pos[rng.random(len(pos)) < 0.15] = ms.SENTINEL
    neg[rng.random(len(neg)) < 0.15] = ms.SENTINEL
    P, N = ms.histogram(pos, lo, hi), ms.histogram(neg, lo, hi)
    assert P.sum() == len(pos) and N.sum() == len(neg)
    want = brute_auc(pos.tolist(), neg.tolist())
    assert abs(ms.auc(P, N) - want) < 1e-12
    z, o = pk.score_summary(P, N)
    assert z == ms.auc(P, N) and o == ms.occur(P, N)


def test_identical_sets_give_one_half():
    rng = np.random.default_rng(3)
    x = rng.integers(-50, 50, 1000)
    P = ms.histogram(x, -50, 50)
    assert ms.auc(P, P) == 0.5
    assert pk.score_summary(P, P)[0] == 0.5
    assert ms.occur(P, P) == 0.0


def test_occur_of_a_planted_mixture():
    # 1000 negatives on 0..99 uniformly, positives: 30 % at 200, the rest like the negatives
    neg = np.arange(1000) % 100
    pos = np.concatenate([np.full(300, 200), np.arange(700) % 100])
    P, N = ms.histogram(pos, 0, 200), ms.histogram(neg, 0, 200)
    # t* = 99: 100 * 10 <= 1000; FPR = 0.01, TPR = (300 + 7) / 1000
    assert abs(ms.occur(P, N) - (0.307 - 0.01) / 0.99) < 1e-12
    assert pk.score_summary(P, N) == (ms.auc(P, N), ms.occur(P, N))


def test_summary_refuses_counts_above_2_62():
    P = np.array([0, 1 << 61], np.uint64)
    N = np.array([1 << 61, 0], np.uint64)
    with pytest.raises(pk.PengkError) as e:
        pk.score_summary(P, N)
    assert e.value.code == pk.ERR_RANGE


@pytest.mark.parametrize("K", [0, 1, 2])
def test_sampler_frequencies_converge_to_V(K):
    rng = np.random.default_rng(K)
    V = [rng.dirichlet(np.ones(4), 4 ** k).astype(np.float32).reshape(-1) for k in range(3)]
    th = ms.thresholds(V, K)
    seqs = ms.sample([400] * 500, 11, 0, K, th)
    x = np.stack(seqs).astype(np.int64)
    if K == 0:
        f = np.bincount(x.reshape(-1), minlength=4) / x.size
        assert np.abs(f - V[0]).max() < 0.01
    else:
        ctx = x[:, K - 1:-1] if K == 1 else x[:, :-2] * 4 + x[:, 1:-1]
        nxt = x[:, K:]
        c = np.zeros((4 ** K, 4))
        np.add.at(c, (ctx.reshape(-1), nxt.reshape(-1)), 1)
        f = c / c.sum(axis=1, keepdims=True)
        assert np.abs(f - V[K].reshape(-1, 4)).max() < 0.03


def test_sampler_depends_on_global_index_only():
    th = ms.thresholds([np.full(4, 0.25, np.float32)] + [np.full(4 ** k, 0.25, np.float32) for k in (2, 3)], 2)
    a = ms.sample([50, 60, 70], 5, 0, 2, th)
    b = ms.sample([60, 70], 5, 1, 2, th)
    assert np.array_equal(a[1], b[0]) and np.array_equal(a[2], b[1])


def test_reverse_complement_matrix():
    rng = np.random.default_rng(1)
    S = rng.integers(-100, 100, (7, 4))
    R = ms.revcomp_S(S)
    for j in range(7):
        for a in range(4):
            assert R[j, a] == S[6 - j, 3 - a]
    # a sequence scored with S_rc = its reverse complement scored with S
    seq = rng.integers(1, 5, 30).astype(np.uint8)
    rc = (5 - seq[::-1]).astype(np.uint8)
    assert ms.best_scores([seq], R, False)[0] == ms.best_scores([rc], S, False)[0]
    assert ms.best_scores([seq], S, True)[0] == max(ms.best_scores([seq], S, False)[0], ms.best_scores([rc], S, False)[0])


def test_log_odds_quantization():
    pwm = np.array([[0.25, 0.5, 0.0, 0.25], [1.0, 0.0, 0.0, 0.0]], np.float32)
    S = ms.log_odds(pwm, np.full(4, 0.25, np.float32))
    assert S.tolist() == [[0, 100, -2000, 0], [200, -2000, -2000, -2000]]


def test_scan_layout_builder():
    rng = np.random.default_rng(5)
    seqs = [rng.integers(0, 6, n).astype(np.uint8) for n in (0, 1, 31, 32, 33, 100)]
    codes, offs = ms.flatten(seqs)
    lay = pk.ScanLayout(codes, offs)
    at = 0
    for i, s in enumerate(seqs):
        assert lay.offs[i] == 32 * at and lay.lens[i] == len(s)
        for p, c in enumerate(s):
            g = int(lay.offs[i]) + p
            ok = 1 <= c <= 4
            assert (int(lay.valid[g >> 5]) >> (g & 31)) & 1 == ok
            if ok:
                assert (int(lay.words[g >> 5]) >> (2 * (g & 31))) & 3 == c - 1
        at += (len(s) + 31) // 32
    assert lay.words.size >= at
