"""CPU checks of the hold-out test (--holdout): the library's pengk_holdout_summary against the numpy model of
tests/motif_holdout_model.py on constructed histograms; the split model's class counts against the binomial they follow;
the CLI's flags; and the scenario behind the README's table -- an input with nothing in it and the same input with a
planted word, found on the training share and judged on both shares -- through the oracle and the numpy models.  No device
compute."""
import math
import os
import subprocess

import numpy as np
import pytest

import peng_motif_amd as pk
import motif_dust_model as md
import motif_enrich_model as me
import motif_erase_model as mer
import motif_holdout_model as mh
import motif_score_model as ms
import motif_shuffle_model as msh
from oracle import oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "peng-motif_amd", "host", "peng_motif")


def close(got, want):
    """the bound tests/test_motif_enrich_cpu.py holds pengk_enrich_summary's logs to"""
    if math.isinf(want) or math.isinf(got):
        return got == want
    return abs(got - want) <= 1e-9 * abs(want) + 1e-9


def check_summary(tp, tn, hp, hn, thr, n):
    got = pk.holdout_summary(tp, tn, hp, hn, thr, *n)
    want = mh.summary(tp, tn, hp, hn, thr, *n)
    print(got)
    for k in ("threshold", "n_thresholds", "train_pos_hits", "train_neg_hits", "hold_pos_hits", "hold_neg_hits"):
        assert got[k] == want[k], (k, got, want)
    for k in ("train_log10_adj_pvalue", "hold_log10_pvalue"):
        assert close(got[k], want[k]), (k, got, want)
    assert abs(got["hold_enrichment"] - want["hold_enrichment"]) <= 1e-14 * want["hold_enrichment"]
    # the training side is pengk_enrich_summary's, field for field
    tr = pk.enrich_summary(tp, tn, thr, n[0], n[1])
    assert (got["threshold"], got["n_thresholds"], got["train_pos_hits"], got["train_neg_hits"], got["train_log10_adj_pvalue"]) == \
        (tr["threshold"], tr["n_thresholds"], tr["pos_hits"], tr["neg_hits"], tr["log10_adj_pvalue"])
    return got


def u64(*x):
    return np.array(x, np.uint64)


# ---- pk.holdout_summary --------------------------------------------------------------------------------------------------------
def test_summary_when_training_tried_no_threshold():
    z = np.zeros(7, np.uint64)
    hp = u64(0, 0, 3, 0, 0, 1, 0)  # (hold-out hits there are: without a threshold they are not counted)
    got = check_summary(z, z, hp, z, 120, (40, 60, 9, 11))
    assert got == dict(threshold=127, n_thresholds=0, train_pos_hits=0, train_neg_hits=0, train_log10_adj_pvalue=0.0,
                       hold_pos_hits=0, hold_neg_hits=0, hold_log10_pvalue=0.0, hold_enrichment=(1.0 / 10.0) / (1.0 / 12.0))
    e = np.zeros(0, np.uint64)
    got = check_summary(e, e, e, e, -5, (0, 0, 0, 0))
    assert (got["threshold"], got["n_thresholds"], got["hold_enrichment"]) == (-5, 0, 1.0)


def test_summary_with_the_threshold_at_the_top_bin():
    tp, tn = u64(0, 0, 0, 30), u64(4, 0, 0, 1)
    hp, hn = u64(5, 2, 1, 6), u64(1, 1, 0, 0)
    got = check_summary(tp, tn, hp, hn, 500, (50, 50, 20, 20))
    assert (got["threshold"], got["hold_pos_hits"], got["hold_neg_hits"]) == (503, 6, 0)
    assert close(got["hold_log10_pvalue"], me.exact_log10_sf(40, 6, 20, 6))


def test_summary_with_equal_p_at_two_thresholds_takes_the_higher():
    """(a, b) = (1, 2) at the top bin and (2, 2) below it, both negatives among the hits: both tails are exactly 1 and the
    higher threshold wins, as in tests/test_motif_enrich_cpu.py; the hold-out bins between the two must not be counted"""
    tp, tn = u64(0, 1, 0, 1), u64(0, 0, 0, 2)
    hp, hn = u64(9, 4, 2, 1), u64(9, 0, 1, 1)
    got = check_summary(tp, tn, hp, hn, 10, (5, 2, 20, 20))
    assert (got["threshold"], got["n_thresholds"], got["hold_pos_hits"], got["hold_neg_hits"]) == (13, 2, 1, 1)


def test_summary_of_an_empty_holdout():
    tp, tn = u64(1, 2, 20, 9), u64(3, 2, 1, 0)
    z = np.zeros(4, np.uint64)
    got = check_summary(tp, tn, z, z, -40, (40, 40, 0, 0))
    assert got["n_thresholds"] == 4 and got["train_log10_adj_pvalue"] < -3
    assert (got["hold_pos_hits"], got["hold_neg_hits"], got["hold_log10_pvalue"], got["hold_enrichment"]) == (0, 0, 0.0, 1.0)
    # sequences but none scored above the bins' floor
    got = check_summary(tp, tn, z, z, -40, (40, 40, 7, 5))
    assert got["hold_log10_pvalue"] == 0.0 and got["hold_enrichment"] == pytest.approx(6.0 / 8.0)


def test_summary_when_no_holdout_input_sequence_hits():
    tp, tn = u64(1, 2, 20, 9), u64(3, 2, 1, 0)
    hp, hn = u64(6, 1, 0, 0), u64(0, 1, 2, 1)
    got = check_summary(tp, tn, hp, hn, 0, (40, 40, 10, 10))
    assert got["threshold"] == 2 and (got["hold_pos_hits"], got["hold_neg_hits"]) == (0, 3)
    assert got["hold_log10_pvalue"] == 0.0 and got["hold_enrichment"] == pytest.approx(0.25)


@pytest.mark.parametrize("seed", range(4))
def test_summary_equals_the_model_on_random_histograms(seed):
    rng = np.random.default_rng(70 + seed)
    nb = int(rng.integers(1, 90))
    hs = [(rng.poisson(rng.uniform(0.05, 4.0), nb) * (rng.random(nb) < 0.7)).astype(np.uint64) for _ in range(4)]
    hs[0][nb // 2:] += rng.poisson(3.0, nb - nb // 2).astype(np.uint64)
    hs[2][nb // 2:] += rng.poisson(1.0, nb - nb // 2).astype(np.uint64)
    n = tuple(int(h.sum()) + int(rng.integers(0, 300)) for h in hs)
    check_summary(hs[0], hs[1], hs[2], hs[3], int(rng.integers(-3000, 3000)), n)


def test_summary_refuses_more_hits_than_scored_sequences():
    h = u64(3, 4)
    for n in [(6, 7, 7, 7), (7, 6, 7, 7), (7, 7, 6, 7), (7, 7, 7, 6)]:
        with pytest.raises(pk.PengkError) as e:
            pk.holdout_summary(h, h, h, h, 0, *n)
        assert e.value.code == pk.ERR_ARG
    assert pk.holdout_summary(h, h, h, h, 0, 7, 7, 7, 7)["n_thresholds"] == 2


# ---- the split model -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_split_class_counts_follow_the_binomial(seed):
    """the classes are n independent-looking draws at p = threshold / 2^32: the hold-out count of a sound hash lies within
    five standard deviations of n p (a chance of 6e-7 per seed for a true binomial), on the whole and on either half"""
    n, F = 100000, 0.1
    t = mh.threshold_of(F)
    assert t == 429496729
    c = mh.classes(seed, 0, n, t)
    for part in (c, c[:n // 2], c[n // 2:]):
        m, got = len(part), int(part.sum())
        print("seed %d: %d of %d held out" % (seed, got, m))
        assert abs(got - m * F) <= 5.0 * math.sqrt(m * F * (1.0 - F))
    # a shard sees what the whole sees, and an index list stands for the indices it names
    assert np.array_equal(mh.classes(seed, 777, n - 777, t), c[777:])
    idx = np.arange(5, n, 7)
    assert np.array_equal(mh.classes(seed, 0, len(idx), t, idx), c[idx])
    i0, i1 = mh.split(seed, 0, n, t)
    assert len(i0) + len(i1) == n and not c[i0].any() and c[i1].all()
    assert not mh.classes(seed, 0, 1000, 0).any() and mh.classes(seed, 0, 1000, 1 << 32).all()


# ---- the CLI's flags -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra,message", [
    (["--holdout", "F", "--holdout-fraction", "0"], b"--holdout-fraction must be"),
    (["--holdout", "F", "--holdout-fraction", "0.51"], b"--holdout-fraction must be"),
    (["--holdout", "F", "--holdout-fraction", "1e-12"], b"--holdout-fraction must be"),
    (["--holdout", "F", "--holdout-fraction", "x"], b"--holdout-fraction must be"),
    (["--holdout", "F", "--holdout-pvalue", "0"], b"--holdout-pvalue must be"),
    (["--holdout-fraction", "0.1"], b"--holdout-fraction requires --holdout"),
    (["--holdout-seed", "3"], b"--holdout-seed requires --holdout"),
    (["--holdout-pvalue", "0.001"], b"--holdout-pvalue requires --holdout"),
], ids=["fraction_0", "fraction_above_half", "fraction_rounds_to_0", "fraction_not_a_number", "pvalue_0", "fraction_alone",
        "seed_alone", "pvalue_alone"])
def test_flag_errors_exit_with_4(tmp_path, extra, message):
    fa = tmp_path / "in.fa"
    fa.write_text(">a\nACGTACGTACGTACGTACGT\n")
    args = [str(tmp_path / "holdout.tsv") if a == "F" else a for a in extra]
    r = subprocess.run([CLI, str(fa), "-w", "8"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=str(tmp_path))
    assert r.returncode == 4 and message in r.stderr, (r.returncode, r.stderr.decode()[-500:])
    assert not (tmp_path / "holdout.tsv").exists()


# ---- the scenario of the README's table --------------------------------------------------------------------------------------
W, F, P, TOP = 8, 0.1, 1e-3, 5
Z_MODEL = 3.0  # the model's seed threshold (see found_on)
WORD = "TGACTCAGCA"
# the seeds on which the model shows the contrast, of 1, 2, 3 (see the test's docstring)
CONTRAST_SEEDS = (1, 2, 3)


def found_on(train, whole):
    """The motifs a run reports, as far as the oracle goes: the TOP best seeds of the training share (both strands, the
    order-2 model of the WHOLE input, as the CLI keeps it), each run through the oracle's EM from the usual 0.7 / 0.1
    start, as integer log-odds.  At the default z-score threshold of 10 an input of 2 000 x 100 bp with nothing in it has no
    seed at all and the comparison would be empty; the model takes every word from z = 3 on, so that the largest of the 4^8
    draws are there to be judged."""
    counts, ltot = po.count(*ms.flatten(train), W, True)
    V = po.bg_V(po.bg_counts(*ms.flatten(whole), 2), 2)
    bgp = po.bgprob(W, 2, V, True)
    _, _, z = po.stats(W, counts, bgp, ltot)
    seeds = po.select(W, z, counts, z_thr=Z_MODEL)[:TOP]
    out = []
    for s in seeds.tolist():
        pwm = np.full((W, 4), 0.1, np.float32)
        for q in range(W):
            pwm[q, (s >> (2 * q)) & 3] = 0.7
        pwm, _, _ = po.em(W, counts, bgp, pwm, 1e4, 0.08, 10)
        out.append(ms.log_odds(pwm, V[:4]))
    return out, V[:4]


def run_scenario(seed, planted):
    """(smallest train_log10_adj_p, smallest hold_log10_E, results, Ss) of the motifs found on the training share"""
    seqs = md.tracts(seed, f_word=0.3 if planted else 0.0, f_tract=0.0)
    i0, i1 = mh.split(1, 0, len(seqs), mh.threshold_of(F))
    neg = [np.asarray(msh.shuffle(np.where(c >= 1, c - 1, 4), 1, g), np.uint8) + 1 for g, c in enumerate(seqs)]  # (no N here: codes 1..4)
    Ss, bg0 = found_on([seqs[i] for i in i0], seqs)
    sets = [[seqs[i] for i in i0], [neg[i] for i in i0], [seqs[i] for i in i1], [neg[i] for i in i1]]
    res = mh.analyse(sets, Ss, bg0, P, True)
    n = len(res)
    return (min([r["summary"]["train_log10_adj_pvalue"] for r in res], default=0.0),
            min([mh.log10_evalue(r["summary"], n) for r in res], default=0.0), res, Ss)


@pytest.fixture(scope="module")
def table():
    return {(seed, planted): run_scenario(seed, planted) for seed in (1, 2, 3) for planted in (False, True)}


def test_the_holdout_tells_a_planted_motif_from_the_best_of_many_draws(table):
    """2 000 x 100 bp uniform, nothing planted or TGACTCAGCA in 30 %, shuffled negatives, W = 8, F = 0.1, split and shuffle
    seed 1.  Per run: the smallest train_log10_adj_p and the smallest hold_log10_E among the reported motifs (the README's
    table).  On the seeds named in CONTRAST_SEEDS: the planted word's hold_log10_E is at most -5 (E <= 1e-5: "far below
    0"), and on the empty input no motif's is below log10 0.05 -- whatever the training figure says."""
    for (seed, planted), (tr, ho, res, Ss) in sorted(table.items()):
        print("seed %d %s: %d motifs, min train_log10_adj_p %.2f, min hold_log10_E %.2f   %s" % (
            seed, "planted" if planted else "empty  ", len(res), tr, ho, [mh.consensus(S) for S in Ss]))
    for seed in CONTRAST_SEEDS:
        tr, ho, res, Ss = table[(seed, True)]
        of_word = [m for m, S in enumerate(Ss) if mer.shares_kmer(mh.consensus(S), WORD)]  # (six letters of it, on either strand)
        assert of_word, [mh.consensus(S) for S in Ss]
        assert min(mh.log10_evalue(res[m]["summary"], len(res)) for m in of_word) <= -5.0
        tr, ho, res, Ss = table[(seed, False)]
        assert len(res) >= 1
        assert ho >= math.log10(0.05), (seed, ho)
