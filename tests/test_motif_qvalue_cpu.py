"""CPU checks of the sites' q-values (--sites-qvalue): the library's pengk_sites_qvalues and pengk_qvalue_threshold
against the numpy model bit for bit, the model against a textbook Benjamini-Hochberg over an explicit p-value list, the
model's histogram against its batch form, the rendering, and the CLI's flags.  No device compute here."""
import os
import subprocess

import numpy as np
import pytest

import peng_motif_amd as pk
import motif_qvalue_model as mq
import motif_sites_model as mst

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "peng-motif_amd", "host", "peng_motif")
GOLD = os.path.join(ROOT, "tests", "golden")


def random_tail(rng, nb):
    """a tail as pengk_score_tail_pvalues gives it: positive masses summed from the top down (runs of equal values
    where a score cannot occur)"""
    mass = rng.random(nb) ** 8 * (rng.random(nb) < 0.7)
    mass[-1] = max(mass[-1], 1e-12)
    tail = np.cumsum(mass[::-1])[::-1]
    return tail / tail[0] * rng.random()


def cases():
    rng = np.random.default_rng(2024)
    out = {}
    for k in range(20):
        nb = int(rng.integers(1, 400))
        h = rng.integers(0, 50, nb).astype(np.uint64) * (rng.random(nb) < 0.6)
        out["random%d" % k] = (h.astype(np.uint64), int(rng.integers(1, 10 ** 7)), random_tail(rng, nb))
    out["empty"] = (np.zeros(0, np.uint64), 1000, np.zeros(0))
    top = np.zeros(50, np.uint64)
    top[-1] = 7
    out["top_only"] = (top, 5 * 10 ** 6, random_tail(rng, 50))
    gaps = np.zeros(64, np.uint64)  # zeros between filled bins, and above the highest filled one (r = +inf there)
    gaps[[0, 1, 9, 10, 30, 55]] = [1000, 3, 40, 1, 5, 2]
    out["gaps"] = (gaps, 10 ** 6, random_tail(rng, 64))
    out["all_zero"] = (np.zeros(17, np.uint64), 10 ** 6, random_tail(rng, 17))
    out["no_tests"] = (rng.integers(0, 9, 30).astype(np.uint64), 0, random_tail(rng, 30))
    big = rng.integers(0, 2 ** 34, 40).astype(np.uint64)
    big[5] = np.uint64(2 ** 40 + 12345)
    out["above_2^32"] = (big, 2 ** 45 + 977, random_tail(rng, 40))
    out["above_2^53"] = (np.array([2 ** 60 + 1, 0, 2 ** 54 + 3, 1], np.uint64), 2 ** 62 + 12345, random_tail(rng, 4))
    # a rising r below a falling one: the running minimum is what keeps q from rising
    out["rising_r"] = (np.array([1000, 0, 5, 0, 1], np.uint64), 10 ** 4, np.array([1e-3, 9e-4, 8e-4, 7e-4, 1e-9]))
    return out


CASES = cases()


@pytest.mark.parametrize("name", list(CASES))
def test_library_qvalues_and_threshold_equal_the_model_bits(name):
    h, N, tail = CASES[name]
    q = pk.sites_qvalues(h, N, tail)
    want = mq.qvalues(h, N, tail)
    assert q.dtype == np.float64 and q.shape == want.shape
    assert np.all(q == want) and q.tobytes() == want.tobytes()
    assert np.all(q <= 1.0) and np.all(q >= 0.0) and np.all(np.diff(q) <= 0)  # never rises with the score, never above 1
    for t in [-700, 0, 13]:
        for Q in [1.0, 0.5, 0.05, 1e-3, 1e-30, 0.0] + [float(x) for x in q[:5]]:
            assert pk.qvalue_threshold(q, t, Q) == mq.qvalue_threshold(q, t, Q)
            k = mq.qvalue_threshold(q, t, Q) - t
            assert (k == len(q) or q[k] <= Q) and np.all(q[:k] > Q)


def test_the_special_histograms_are_what_the_definition_says():
    h, N, tail = CASES["gaps"]
    q = mq.qvalues(h, N, tail)
    # bins 56.. hold no site at or above them: r = +inf, and q there is the minimum so far
    assert np.all(q[56:] == q[55])
    h, N, tail = CASES["all_zero"]
    assert np.all(mq.qvalues(h, N, tail) == 1.0) and np.all(pk.sites_qvalues(h, N, tail) == 1.0)
    h, N, tail = CASES["no_tests"]
    q = pk.sites_qvalues(h, N, tail)
    assert h.sum() > 0 and np.all(q == 0.0)  # N = 0: the ratio of bin 0 is 0, and the minimum keeps it
    h, N, tail = CASES["rising_r"]
    q = mq.qvalues(h, N, tail)
    # ranks 1006, 6, 6, 1, 1: r = 0.0099, 1.5, 1.3, 7, 1e-5 -- bins 1..3 keep bin 0's ratio
    assert np.all(q[:4] == 1e4 * 1e-3 / 1006) and q[4] == 1e4 * 1e-9 / 1
    assert len(pk.sites_qvalues(np.zeros(0, np.uint64), 5, np.zeros(0))) == 0
    assert pk.qvalue_threshold(np.zeros(0), 42, 0.5) == 42


def textbook_bh(p, N):
    """Benjamini-Hochberg adjusted p-values of the reported p-values p out of N tests: sort ascending, p_(i) N / i, then
    the minimum over every rank at or above i, capped at 1; ties share the largest rank among them"""
    p = np.asarray(p, np.float64)
    order = np.argsort(p, kind="stable")
    adj = p[order] * N / np.arange(1, len(p) + 1)
    adj = np.minimum(1.0, np.minimum.accumulate(adj[::-1])[::-1])
    out = np.empty(len(p))
    out[order] = adj
    return out


@pytest.mark.parametrize("seed", range(6))
def test_qvalues_equal_textbook_bh_over_the_expanded_list(seed):
    rng = np.random.default_rng(50 + seed)
    nb = int(rng.integers(5, 60))
    h = (rng.integers(0, 30, nb) * (rng.random(nb) < 0.7)).astype(np.uint64)
    # a strictly falling tail: one p-value per score, as the definition assumes of ranks by score
    tail = np.sort(rng.random(nb) * 1e-3)[::-1].copy()
    N = int(rng.integers(10 ** 3, 10 ** 6))
    q = mq.qvalues(h, N, tail)
    bins = np.repeat(np.arange(nb), h.astype(np.int64))
    rng.shuffle(bins)
    bh = textbook_bh(tail[bins], N)
    assert len(bins) > 0
    # the same numbers up to the order of the operations (p N / i here, N p / n there)
    assert np.all(np.abs(bh - q[bins]) <= 4 * np.finfo(np.float64).eps * q[bins])


def random_S(rng, w):
    S = rng.integers(-300, 301, (w, 4)).astype(np.int32)
    S[rng.random((w, 4)) < 0.05] = -2000
    return S


@pytest.mark.parametrize("both", [True, False])
def test_model_histogram_equals_its_batch_form_and_the_sites(both):
    rng = np.random.default_rng(9 + both)
    n, L = 40, 37
    codes = rng.integers(1, 5, (n, L)).astype(np.uint8)
    codes[rng.random((n, L)) < 0.03] = 0
    seqs = [codes[i] for i in range(n)]
    bg = np.full(4, 0.25, np.float32)
    for w in [1, 4, 9, 38]:
        S = random_S(rng, w)
        lo, tail = mst.tail_pvalues(S, bg)
        for t in [mst.threshold(lo, tail, 0.05), lo, mq.score_hi(S) + 1]:
            h, N = mq.histogram(seqs, S, t, both)
            hb, Nb = mq.histogram_batch(codes, S, t, both)
            assert N == Nb and h.tobytes() == hb.tobytes()
            assert len(h) == max(0, mq.score_hi(S) - t + 1)
            assert int(h.sum()) == len(mst.sites(seqs, S, t, both))
            if t == lo:  # P = 1: every scored strand is a site
                assert int(h.sum()) == N


def test_render_adds_one_column_and_filters_by_q():
    rng = np.random.default_rng(3)
    seqs = [rng.integers(1, 5, 80).astype(np.uint8) for _ in range(30)]
    cons = [1, 1, 2, 2, 3, 4, 1, 3]  # AACCGTAG, planted in 20 of the 30 sequences
    for s in seqs[:20]:
        s[10:18] = cons
    names = ["s%d" % i for i in range(len(seqs))]
    S = np.full((8, 4), -150, np.int32)
    S[np.arange(8), np.array(cons) - 1] = 120
    bg = np.full(4, 0.25, np.float32)
    P = 0.01  # (up to two mismatches)
    plain = mst.render(seqs, names, ["AACCGTAG"], [S], bg, P, True)
    txt = mq.render(seqs, names, ["AACCGTAG"], [S], bg, P, True)
    lines = txt.splitlines(True)
    assert lines[0] == mq.HEADER and mq.HEADER.split("\t")[8] == "q_value"
    assert "".join("\t".join(l.split("\t")[:8] + l.split("\t")[9:]) for l in lines) == plain
    qs = [float(l.split("\t")[8]) for l in lines[1:]]
    assert len(qs) > 25 and min(qs) < 0.05 < max(qs)
    sub = mq.render(seqs, names, ["AACCGTAG"], [S], bg, P, True, Q=0.05).splitlines(True)
    lo, tail, t, h, N, q = mq.motif_qvalues(seqs, S, bg, P, True)
    t2 = mq.qvalue_threshold(q, t, 0.05)
    keep = [l for l in lines[1:] if round(float(l.split("\t")[6]) * 100) >= t2]
    assert sub[1:] == keep and 0 < len(keep) < len(lines) - 1
    assert all(q[round(float(l.split("\t")[6]) * 100) - t] <= 0.05 for l in keep)


def clean_env():
    return {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PENGK_COMM_TRANSPORT")}


def test_help_lists_the_qvalue_flags():
    r = subprocess.run([CLI, "-h"], stdout=subprocess.PIPE, env=clean_env(), timeout=60)
    assert r.returncode == 0
    assert b"--sites-qvalue " in r.stdout and b"--sites-qvalue-max FLOAT" in r.stdout


@pytest.mark.parametrize("bad", ["0", "2", "x", "-0.1", "nan", "0.05x"])
def test_bad_sites_qvalue_max_is_refused(tmp_path, bad):
    r = subprocess.run([CLI, os.path.join(GOLD, "MafK.fasta"), "--sites", str(tmp_path / "s.tsv"), "--sites-qvalue-max", bad],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=clean_env(), timeout=60)
    assert r.returncode == 4, (bad, r.returncode, r.stderr[-500:])
    assert b"--sites-qvalue-max" in r.stderr
    assert not (tmp_path / "s.tsv").exists()
