"""CPU checks of the database enrichment (--enrich): the log-space hypergeometric tail against the exact tail in Python
integers and, where that cannot reach, against its own complement; the library's summary against the numpy model of
tests/motif_enrich_model.py; the model's fast best-score scan against motif_score_model's; the CLI's flags; and the planted
case the README quotes, on the model alone.  No device compute."""
import math
import os
import subprocess

import numpy as np
import pytest

import peng_motif_amd as pk
import motif_compare_model as mc
import motif_enrich_model as me
import motif_score_model as ms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "peng-motif_amd", "host", "peng_motif")
GOLD = os.path.join(ROOT, "tests", "golden")


def close(got, want):
    """the bound tests/test_motif_centrality_cpu.py holds pengk_binomial_log10_sf to"""
    if math.isinf(want) or math.isinf(got):
        return got == want
    return abs(got - want) <= 1e-9 * abs(want) + 1e-9


# ---- pk.hypergeom_log10_sf -----------------------------------------------------------------------------------------------------
def test_tail_at_and_beyond_both_ends_of_the_support():
    for N, K, n in [(50, 20, 10), (50, 45, 30), (10, 10, 4), (10, 0, 4), (10, 3, 0), (10, 3, 10), (1, 1, 1), (0, 0, 0),
                    (20000, 15000, 12000)]:
        lo, hi = me.support(N, K, n)
        assert pk.hypergeom_log10_sf(N, K, n, lo) == 0.0
        if lo:
            assert pk.hypergeom_log10_sf(N, K, n, lo - 1) == 0.0 and pk.hypergeom_log10_sf(N, K, n, 0) == 0.0
        assert pk.hypergeom_log10_sf(N, K, n, hi + 1) == -math.inf and pk.hypergeom_log10_sf(N, K, n, hi + 1000) == -math.inf
        for k in {lo + 1, hi} - {lo}:
            if lo < k <= hi:
                got, want = pk.hypergeom_log10_sf(N, K, n, k), me.exact_log10_sf(N, K, n, k)
                assert close(got, want), (N, K, n, k, got, want)
    for bad in [(10, 11, 3, 1), (10, 3, 11, 1)]:
        with pytest.raises(pk.PengkError) as e:
            pk.hypergeom_log10_sf(*bad)
        assert e.value.code == pk.ERR_ARG


def test_tail_equals_the_exact_tail_on_random_cases():
    rng = np.random.default_rng(21)
    worst = 0.0
    for _ in range(400):
        N = int(10 ** rng.uniform(0, 4.3))
        K, n = int(rng.integers(0, N + 1)), int(rng.integers(0, N + 1))
        lo, hi = me.support(N, K, n)
        k = int(rng.integers(lo, hi + 2))
        got, want = pk.hypergeom_log10_sf(N, K, n, k), me.exact_log10_sf(N, K, n, k)
        assert close(got, want), (N, K, n, k, got, want)
        if math.isfinite(want):
            worst = max(worst, abs(got - want) / (1e-9 * abs(want) + 1e-9))
    print("largest error, in units of the bound: %.3g" % worst)


def test_tails_far_below_the_smallest_double():
    # every one of 2 000 marked among the 3 000 drawn of 200 000: C(198000, 1000) / C(200000, 3000)
    N, K, n = 200000, 2000, 3000
    for k in (1500, 1990, 2000):
        got, want = pk.hypergeom_log10_sf(N, K, n, k), me.exact_log10_sf(N, K, n, k)
        assert want < -400 and close(got, want), (k, got, want)
    # the falling-factorial form at the size of a run: 4e7 sequences, a motif in 1 500 of them, 1 400 of those in the input
    N, K, n = 40000000, 1500, 20000000
    for k in (1, 700, 750, 800, 1400, 1500):
        got, want = pk.hypergeom_log10_sf(N, K, n, k), me.exact_log10_sf(N, K, n, k)
        assert close(got, want), (k, got, want)
    assert me.exact_log10_sf(N, K, n, 1500) < -400


def test_the_model_tail_equals_the_exact_tail():
    """(what the summary is compared with: the model's own log-space tail, held to the exact one here)"""
    rng = np.random.default_rng(22)
    for _ in range(150):
        N = int(10 ** rng.uniform(0, 4))
        K, n = int(rng.integers(0, N + 1)), int(rng.integers(0, N + 1))
        lo, hi = me.support(N, K, n)
        k = int(rng.integers(lo, hi + 2))
        assert close(me.log10_sf(N, K, n, k), me.exact_log10_sf(N, K, n, k)), (N, K, n, k)
    N, K, n = 40000000, 1500, 20000000
    for k in (700, 800, 1500):
        assert close(me.log10_sf(N, K, n, k), me.exact_log10_sf(N, K, n, k)), k


def test_large_counts_with_a_tail_near_one_through_the_complement():
    """N = 4e7, K about N / 4: no exact tail is feasible.  X' = K - X counts the marked among the N - n that were not
    drawn, so P(X >= k | N, K, n) + P(X' >= K - k + 1 | N, K, N - n) = 1"""
    N, K, n = 40000000, 10000019, 19999993
    mean = K * n // N
    sd = int(math.sqrt(K * (n / N) * (1 - n / N) * (N - K) / N))
    seen_near_one = False
    for k in (mean - 8 * sd, mean - 3 * sd, mean - sd, mean - 1, mean, mean + 1, mean + sd, mean + 3 * sd, mean + 8 * sd):
        a = pk.hypergeom_log10_sf(N, K, n, k)
        b = pk.hypergeom_log10_sf(N, K, N - n, K - k + 1)
        assert abs(10.0 ** a + 10.0 ** b - 1.0) <= 1e-9, (k, a, b)
        seen_near_one |= a > -1e-3
        # and against the model's tail, whose point mass comes from 50-digit logarithms
        assert close(a, me.log10_sf(N, K, n, k)), (k, a)
    assert seen_near_one
    # far out: finite, below double's range, and the model's
    got = pk.hypergeom_log10_sf(N, K, n, mean + 400 * sd)
    assert got < -400 and close(got, me.log10_sf(N, K, n, mean + 400 * sd))


# ---- pk.enrich_summary ---------------------------------------------------------------------------------------------------------
def check_summary(h_pos, h_neg, thr, n_pos, n_neg):
    got = pk.enrich_summary(h_pos, h_neg, thr, n_pos, n_neg)
    want = me.summary(h_pos, h_neg, thr, n_pos, n_neg)
    assert got["n_thresholds"] == want["n_thresholds"]
    if want["n_thresholds"] == 0:
        assert got == dict(want, enrichment=got["enrichment"]) and got["enrichment"] == (n_neg + 1.0) / (n_pos + 1.0)
        return got
    k = got["threshold"] - thr
    assert (k, got["pos_hits"], got["neg_hits"]) in me.tried(h_pos, h_neg)
    lp = me.log10_p_at(h_pos, h_neg, k, n_pos, n_neg)
    assert close(got["log10_pvalue"], lp), (got, lp)
    assert abs(lp - want["log10_pvalue"]) <= 1e-9 * abs(want["log10_pvalue"]) + 1e-9  # (the model's minimum)
    assert close(got["log10_adj_pvalue"], min(0.0, got["log10_pvalue"] + math.log10(got["n_thresholds"])))
    e = me.enrichment(got["pos_hits"], got["neg_hits"], n_pos, n_neg)
    assert abs(got["enrichment"] - e) <= 1e-14 * e
    return got


@pytest.mark.parametrize("seed", range(6))
def test_summary_equals_the_model_on_random_histograms(seed):
    rng = np.random.default_rng(40 + seed)
    nb = int(rng.integers(1, 120))
    h_pos = (rng.poisson(rng.uniform(0.05, 4.0), nb) * (rng.random(nb) < 0.7)).astype(np.uint64)
    h_neg = (rng.poisson(rng.uniform(0.05, 4.0), nb) * (rng.random(nb) < 0.7)).astype(np.uint64)
    if seed % 2:
        h_pos[nb // 2:] += rng.poisson(3.0, nb - nb // 2).astype(np.uint64)  # (enriched at the top)
    n_pos, n_neg = int(h_pos.sum()) + int(rng.integers(0, 500)), int(h_neg.sum()) + int(rng.integers(0, 500))
    check_summary(h_pos, h_neg, int(rng.integers(-3000, 3000)), n_pos, n_neg)


def test_summary_of_empty_histograms_and_of_no_bins():
    z = np.zeros(7, np.uint64)
    got = check_summary(z, z, 120, 40, 60)
    assert got == dict(threshold=127, n_thresholds=0, pos_hits=0, neg_hits=0, enrichment=61.0 / 41.0, log10_pvalue=0.0,
                       log10_adj_pvalue=0.0)
    e = np.zeros(0, np.uint64)
    got = check_summary(e, e, -5, 0, 0)
    assert (got["threshold"], got["n_thresholds"], got["enrichment"]) == (-5, 0, 1.0)


def test_summary_when_only_the_negatives_have_hits():
    h_pos, h_neg = np.zeros(10, np.uint64), np.zeros(10, np.uint64)
    h_neg[[2, 7]] = [5, 3]
    got = check_summary(h_pos, h_neg, 0, 100, 100)
    # a = 0 at both thresholds: both tails are 1, the higher threshold wins the tie
    assert (got["threshold"], got["n_thresholds"], got["pos_hits"], got["neg_hits"]) == (7, 2, 0, 3)
    assert got["log10_pvalue"] == 0.0 and got["log10_adj_pvalue"] == 0.0 and got["enrichment"] == pytest.approx(0.25)


def test_summary_of_a_single_filled_bin():
    h_pos, h_neg = np.zeros(30, np.uint64), np.zeros(30, np.uint64)
    h_pos[11], h_neg[11] = 40, 2
    got = check_summary(h_pos, h_neg, 500, 50, 50)
    assert (got["threshold"], got["n_thresholds"], got["pos_hits"], got["neg_hits"]) == (511, 1, 40, 2)
    assert got["log10_adj_pvalue"] == got["log10_pvalue"] < -10
    assert close(got["log10_pvalue"], me.exact_log10_sf(100, 42, 50, 40))


def test_summary_tie_between_two_thresholds_goes_to_the_higher():
    """Two thresholds tie exactly where both tails are exactly 1: a = 0 (above), or every negative among the hits, b = n_neg,
    so that a <= n_pos + K - N is the lower end of the support.  Here (a, b) = (1, 2) at the top bin and (2, 2) below it."""
    h_pos, h_neg = np.array([0, 1, 0, 1], np.uint64), np.array([0, 0, 0, 2], np.uint64)
    got = check_summary(h_pos, h_neg, 10, 5, 2)
    assert (got["threshold"], got["n_thresholds"], got["pos_hits"], got["neg_hits"], got["log10_pvalue"]) == (13, 2, 1, 2, 0.0)
    # a third, lower threshold that is strictly better takes it from both
    h_pos, h_neg = np.array([30, 1, 0, 1], np.uint64), np.array([0, 0, 0, 2], np.uint64)
    got = check_summary(h_pos, h_neg, 10, 40, 2)
    assert (got["threshold"], got["n_thresholds"]) == (13, 3) and got["log10_pvalue"] == 0.0  # (b = n_neg there too)
    h_pos, h_neg = np.array([30, 1, 0, 1], np.uint64), np.array([0, 0, 0, 2], np.uint64)
    got = check_summary(h_pos, h_neg, 10, 40, 30)
    assert got["threshold"] == 10 and got["log10_pvalue"] < -5
    # the rule on the model's own values: the highest of the thresholds that reach the minimum
    vals = {k: me.log10_p_at(h_pos, h_neg, k, 40, 30) for k, _, _ in me.tried(h_pos, h_neg)}
    assert got["threshold"] - 10 == max(k for k, v in vals.items() if v == min(vals.values()))


def test_summary_with_counts_above_2_to_the_32():
    big = 2 ** 32
    # (ten million more input sequences than negatives at the third bin, of 2^33 each: hundreds of standard deviations)
    h_pos = np.array([3 * big, 0, 2 * big + 10 ** 7, 7], np.uint64)
    h_neg = np.array([3 * big + 99, 5, 2 * big, 1], np.uint64)
    n_pos, n_neg = 6 * big, 6 * big + 1000
    got = check_summary(h_pos, h_neg, -40, n_pos, n_neg)
    assert got["n_thresholds"] == 4 and got["pos_hits"] > big and got["threshold"] in (-40, -38)
    assert got["log10_pvalue"] < -1000


def test_summary_refuses_more_hits_than_scored_sequences():
    h = np.array([3, 4], np.uint64)
    for n_pos, n_neg in [(6, 7), (7, 6)]:
        with pytest.raises(pk.PengkError) as e:
            pk.enrich_summary(h, h, 0, n_pos, n_neg)
        assert e.value.code == pk.ERR_ARG and "pengk_enrich_summary" in str(e.value)
    assert pk.enrich_summary(h, h, 0, 7, 7)["n_thresholds"] == 2


# ---- the model's scan ------------------------------------------------------------------------------------------------------
def random_seqs(rng, n):
    lens = [0, 1, 3, 4, 5, 12, 13, 31, 32, 33, 63, 64, 65, 120] + rng.integers(0, 121, n - 14).tolist()
    seqs = []
    for L in lens:
        c = rng.integers(1, 5, L).astype(np.uint8)
        for _ in range(int(rng.integers(0, 3))):
            if L:
                a = int(rng.integers(0, L))
                c[a:a + int(rng.integers(1, 20))] = 0
        seqs.append(c)
    return seqs


@pytest.mark.parametrize("both", [True, False], ids=["both", "plus"])
def test_model_scan_equals_the_per_sequence_model(both):
    rng = np.random.default_rng(8)
    seqs = random_seqs(rng, 60)
    packed = me.Packed(seqs)
    for w in (1, 4, 5, 13, 64):
        S = rng.integers(-300, 301, (w, 4)).astype(np.int32)
        assert np.array_equal(me.best_scores(packed, S, both), ms.best_scores(seqs, S, both)), w
    S = rng.integers(-300, 301, (6, 4)).astype(np.int32)
    best = me.best_scores(packed, S, both)
    lo, hi = ms.score_range(S)
    for thr in (lo, (lo + hi) // 2, hi + 1):
        h, scored = me.histogram(best, thr, hi)
        assert len(h) == max(0, hi - thr + 1) and scored == int((best != me.SENTINEL).sum())
        assert int(h.sum()) == int(((best != me.SENTINEL) & (best >= thr)).sum())
    assert np.array_equal(me.best_scores(me.Packed([]), S, both), np.zeros(0, np.int64))


def test_database_log_odds():
    bg = np.array([0.3, 0.2, 0.2, 0.3], np.float32)
    S = me.db_log_odds([[1, 0, 0, 0], [2, 2, 2, 2], [0.97, 0.01, 0.01, 0.01]], bg)
    b = bg.astype(np.float64)
    # a zero entry scores the pseudocount's share, not the clamp: 100 log2((0.01 b / 1.01) / b) = 100 log2(0.01 / 1.01)
    assert S[0, 1] == S[0, 2] == S[0, 3] == round(100 * math.log2(0.01 / 1.01))
    assert S[0, 0] == round(100 * math.log2((1 + 0.01 * b[0]) / 1.01 / b[0]))
    assert S[1].tolist() == [round(100 * math.log2((0.25 + 0.01 * x) / 1.01 / x)) for x in b]
    assert S.dtype == np.int32 and np.abs(S).max() <= 2000


# ---- the CLI's flags -------------------------------------------------------------------------------------------------------
def clean_env():
    return {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PENGK_COMM_TRANSPORT")}


def run_cli(args, tmp_path):
    """the flags under test behind -o / -j, so that a flag without its value is the last argument"""
    r = subprocess.run([CLI, os.path.join(GOLD, "MafK.fasta"), "-w", "10", "-o", str(tmp_path / "e.meme"), "-j", str(tmp_path / "e.json")]
                       + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=clean_env(), timeout=60)
    return r.returncode, r.stdout, r.stderr


def small_db(tmp_path):
    names, rows = mc.planted_database(n_decoys=3)
    db = tmp_path / "db.meme"
    mc.write_meme(db, names, rows)
    return str(db)


def test_help_lists_the_enrich_flags():
    r = subprocess.run([CLI, "-h"], stdout=subprocess.PIPE, env=clean_env(), timeout=60)
    assert r.returncode == 0
    for flag in (b"--enrich FILE", b"--enrich-db FILE", b"--enrich-pvalue FLOAT", b"--enrich-evalue FLOAT"):
        assert flag in r.stdout


@pytest.mark.parametrize("args,message", [
    (["--enrich", "e.tsv"], b"ERROR: --enrich requires --enrich-db"),
    (["--enrich-db", "DB"], b"ERROR: --enrich-db requires --enrich"),
    (["--enrich", "e.tsv", "--enrich-db"], b"ERROR: No expression following --enrich-db"),
    (["--enrich-db", "DB", "--enrich"], b"ERROR: No expression following --enrich"),
    (["--enrich", "e.tsv", "--enrich-db", "DB", "--enrich-pvalue", "0"], b"ERROR: --enrich-pvalue must be a number in (0, 1]"),
    (["--enrich", "e.tsv", "--enrich-db", "DB", "--enrich-pvalue", "1.5"], b"ERROR: --enrich-pvalue must be a number in (0, 1]"),
    (["--enrich", "e.tsv", "--enrich-db", "DB", "--enrich-pvalue", "1e-3x"], b"ERROR: --enrich-pvalue must be a number in (0, 1]"),
    (["--enrich", "e.tsv", "--enrich-db", "DB", "--enrich-pvalue", "nan"], b"ERROR: --enrich-pvalue must be a number in (0, 1]"),
    (["--enrich", "e.tsv", "--enrich-db", "DB", "--enrich-evalue", "0"], b"ERROR: --enrich-evalue must be a number above 0"),
    (["--enrich", "e.tsv", "--enrich-db", "DB", "--enrich-evalue", "-2"], b"ERROR: --enrich-evalue must be a number above 0"),
    (["--enrich", "e.tsv", "--enrich-db", "DB", "--enrich-evalue", "ten"], b"ERROR: --enrich-evalue must be a number above 0"),
], ids=lambda a: "_".join(a).replace("--", "") if isinstance(a, list) else None)
def test_cli_argument_errors_exit_4(tmp_path, args, message):
    """as --compare's: the help, an ERROR line, exit 4, before the input is read (no device is needed for it)"""
    db = small_db(tmp_path)
    args = [str(tmp_path / a) if a.endswith(".tsv") else db if a == "DB" else a for a in args]
    rc, so, se = run_cli(args, tmp_path)
    assert rc == 4 and message in se and b"--enrich FILE" in so, (rc, se[-300:])
    assert not list(tmp_path.glob("*.tsv")) and not (tmp_path / "e.meme").exists()


@pytest.mark.parametrize("text", [None, "MEME version 4\n\n", "MOTIF a\nletter-probability matrix: alength= 4\n1 0 0 0\n",
                                  "MOTIF a\nletter-probability matrix: w= 1\n0 0 0 0\n",
                                  "MOTIF a\nletter-probability matrix: w= 65\n" + "1 0 0 0\n" * 65],
                         ids=["missing", "no_motif", "no_w", "zero_row", "w_65"])
def test_cli_refuses_a_database_it_cannot_use(tmp_path, text):
    db = tmp_path / "bad.meme"
    if text is not None:
        db.write_text(text)
    rc, so, se = run_cli(["--enrich", str(tmp_path / "e.tsv"), "--enrich-db", str(db)], tmp_path)
    assert rc == 4 and b"ERROR: --enrich-db: motif database" in se and b"bad.meme" in se, (rc, se[-300:])
    assert not (tmp_path / "e.tsv").exists() and not (tmp_path / "e.meme").exists()


# ---- a planted case, on the model alone ------------------------------------------------------------------------------------
def planted_case():
    """2 000 x 100 bp sampled from a skewed order-0 background, the 10-mer TGACTCAGCA planted in 30 % of them; a database of
    that word, a word that overlaps its second half, and 48 decoys; dinucleotide-free negatives: every sequence shuffled"""
    rng = np.random.default_rng(77)
    bg = np.array([0.3, 0.2, 0.2, 0.3], np.float32)
    word = np.array(["ACGT".index(c) + 1 for c in "TGACTCAGCA"], np.uint8)
    seqs, negs = [], []
    for i in range(2000):
        s = (rng.choice(4, 100, p=bg.astype(np.float64) / bg.astype(np.float64).sum()) + 1).astype(np.uint8)
        if rng.random() < 0.3:
            p = int(rng.integers(0, 91))
            s[p:p + 10] = word
        seqs.append(s)
        negs.append(rng.permutation(s))
    names = ["planted", "half"] + ["decoy%02d" % d for d in range(48)]
    rows = [mc.word_rows("TGACTCAGCA"), mc.word_rows("CAGCATTGGA")] + [mc.dirichlet_rows(rng, int(rng.integers(6, 20))) for _ in range(48)]
    return names, rows, bg, seqs, negs


def test_planted_word_ranks_first_in_the_model():
    names, rows, bg, seqs, negs = planted_case()
    res = me.analyse(me.Packed(seqs), me.Packed(negs), rows, bg, 1e-3, True)
    sums = [r["summary"] for r in res]
    order = me.order_of(sums)
    text = me.render(names, [""] * len(names), res, E=1e9)
    print(text.split("\n")[0])
    for line in text.split("\n")[1:4]:
        print(line)
    assert names[order[0]] == "planted"
    decoys = [m for m in range(len(names)) if names[m].startswith("decoy")]
    best_decoy = min(sums[m]["log10_adj_pvalue"] for m in decoys)
    print("planted: log10 adj p = %.3f, half: %.3f, best decoy: %.3f" % (sums[0]["log10_adj_pvalue"], sums[1]["log10_adj_pvalue"],
                                                                     best_decoy))
    assert sums[0]["log10_adj_pvalue"] < best_decoy and sums[0]["log10_adj_pvalue"] < -50
    assert all(r["n_pos"] == 2000 and r["n_neg"] == 2000 for r in res)
    # the file: one line per motif at this E, ranks 1 .. 50 in order, q-values never falling with the rank
    lines = [l.split("\t") for l in text.split("\n")[1:] if l]
    assert [int(l[0]) for l in lines] == list(range(1, 51)) and lines[0][1] == "planted"
    q = [float(l[14]) for l in lines]
    assert all(a <= b for a, b in zip(q, q[1:])) and q[-1] <= 1.0
    # and the default E-value of 10 keeps fewer
    assert 1 <= len(me.render(names, [""] * len(names), res).split("\n")) - 2 < 50
