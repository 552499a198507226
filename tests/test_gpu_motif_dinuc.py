"""First-order motif models on the device (--dinuc; include/pengk.h, "first-order motif models") against the numpy model of
tests/motif_dinuc_model.py: the pair profiles bit for bit (sites at both sequence ends, both strands, clamped flanks, split
records, a motif nearly every sequence holds), the first-order scan value by value (every chunk and register boundary, the
order-0 scan as its degenerate case), a planted dependency found and paid for, and the CLI's two files against the model,
beside the other outputs and over several ranks."""
import itertools
import json
import os

import numpy as np
import pytest

import peng_motif_amd as pk
import motif_dinuc_model as md
import motif_score_model as ms
from oracle import oracle as po
from test_gpu_motif_refine import consensus_pwm, found_log_odds, low_thresholds, random_S, random_seqs, sub_scan
from test_gpu_multirank import run_plain, run_ranks
from test_motif_dinuc_cpu import (PLANT_SEED, UNIFORM, assert_planted_conditions, planted_analysis, planted_negatives,
                                  planted_seqs, planted_start_pwm, random_model)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
WIDTHS = [2, 4, 5, 7, 10, 13, 16, 21, 30]
FLANKS = [0, 1, 8, 40]  # (40: clamped for every width, to 17 at w = 30)
SCAN_WIDTHS = [1, 2, 3, 4, 5, 8, 9, 12, 13, 16, 17, 33, 63, 64]  # no pair, one pair, the chunk and register boundaries, the maximum


@pytest.fixture(scope="module")
def ctx():
    c = pk.Context(0)
    yield c
    c.close()


# ---- pair profiles ---------------------------------------------------------------------------------------------------------
def model_pairs(seqs, gb, gs, widths, thr, flank):
    return np.stack([md.pair_profile(seqs, gb[m], gs[m], widths[m], thr[m], flank) for m in range(len(widths))])


@pytest.mark.parametrize("both", [True, False], ids=["both", "plus"])
def test_pair_counts_equal_the_model(ctx, both):
    rng = np.random.default_rng(171 + both)
    seqs = random_seqs(rng)
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    S = [random_S(rng, w) for w in WIDTHS]
    best, site = ctx.motif_best_sites(scan, S, WIDTHS, both)
    gb, gs = best.to_host(), site.to_host()
    thr = low_thresholds(gb)
    for flank in FLANKS:
        got = ctx.site_pair_profiles(scan, best, site, WIDTHS, thr, flank).to_host()
        want = model_pairs(seqs, gb, gs, WIDTHS, thr, flank)
        assert got.tobytes() == want.tobytes(), flank
        single = ctx.site_profiles(scan, best, site, WIDTHS, thr, flank).to_host()
        F = [pk.clamp_flank(w, flank) for w in WIDTHS]
        for m, w in enumerate(WIDTHS):
            n, W = single[m, F[m]].sum(), w + 2 * F[m]
            assert n > 20 and not got[m, 0].any() and not got[m, W:].any()  # (row 0 and the rows beyond stay untouched)
            assert np.all(got[m, 1:W].sum(axis=1) == n)
            assert not got[m, F[m] + 1:F[m] + w, 16].any()  # (a site's own columns are bases)
        if flank >= 8:  # sites at both sequence ends: the outermost flank pairs fall off some sequence
            assert got[:, 1, 16].sum() > 0 and sum(got[m, w + 2 * F[m] - 1, 16] for m, w in enumerate(WIDTHS)) > 0
    if both:
        assert np.count_nonzero(gs & np.uint64(1)) > 50
    # a second call adds to the first
    c = ctx.site_pair_profiles(scan, best, site, WIDTHS, thr, 8)
    ctx.site_pair_profiles(scan, best, site, WIDTHS, thr, 8, counts=c)
    assert c.to_host().tobytes() == (2 * model_pairs(seqs, gb, gs, WIDTHS, thr, 8)).tobytes()


def test_pair_counts_without_validity_words(ctx):
    """d_valid = NULL (the sampled sequences' layout): a letter other than A/C/G/T is stored as A and counts as A"""
    rng = np.random.default_rng(181)
    seqs = random_seqs(rng)
    words, _, offs, lens, n = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    scan = (words, 0, offs, lens, n)
    as_a = [np.where(c == 0, 1, c).astype(np.uint8) for c in seqs]
    S = [random_S(rng, w) for w in WIDTHS]
    best, site = ctx.motif_best_sites(scan, S, WIDTHS, True)
    gb, gs = best.to_host(), site.to_host()
    thr = low_thresholds(gb)
    got = ctx.site_pair_profiles(scan, best, site, WIDTHS, thr, 8, all_valid=True).to_host()
    assert got.tobytes() == model_pairs(as_a, gb, gs, WIDTHS, thr, 8).tobytes()
    assert got[..., 16].any()  # (outside the sequence still is)


def test_pair_counts_of_two_halves_add_up_to_one_call(ctx):
    rng = np.random.default_rng(191)
    seqs = random_seqs(rng)
    n = len(seqs)
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    S = [random_S(rng, w) for w in WIDTHS]
    best, site = ctx.motif_best_sites(scan, S, WIDTHS, True)
    thr = low_thresholds(best.to_host())
    whole = ctx.site_pair_profiles(scan, best, site, WIDTHS, thr, 8).to_host()
    assert whole.any()
    for k in [1, 37, n // 2, n - 1]:
        c = None
        for i0, i1 in [(0, k), (k, n)]:
            part = sub_scan(scan, i0, i1)
            b, s = ctx.motif_best_sites(part, S, WIDTHS, True, seq0=i0)
            c = ctx.site_pair_profiles(part, b, s, WIDTHS, thr, 8, counts=c)
        assert c.to_host().tobytes() == whole.tobytes(), k


def test_pair_counts_of_a_motif_nearly_every_sequence_holds(ctx):
    """96 % of the sequences select the same consensus: whole waves add to one (column, pair) bin, the contended path"""
    rng = np.random.default_rng(201)
    n, L, word = 20000, 100, "TGCTGAGTCAGC"
    mot = np.array(["ACGT".index(c) + 1 for c in word], np.uint8)
    codes = rng.integers(1, 5, (n, L)).astype(np.uint8)
    for i in np.nonzero(rng.random(n) < 0.96)[0]:
        p = int(rng.integers(0, L - len(word) + 1))
        codes[i, p:p + len(word)] = mot if rng.random() < 0.5 else 5 - mot[::-1]
    S = [ms.log_odds(consensus_pwm(word), UNIFORM), random_S(rng, 9)]
    widths = [len(word), 9]
    thr = []
    for s in S:
        lo, tail = pk.score_tail_pvalues(s, UNIFORM)
        thr.append(pk.score_threshold(tail, lo, 1e-4))
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(list(codes))))
    best, site = ctx.motif_best_sites(scan, S, widths, True)
    gb, gs = best.to_host(), site.to_host()
    got = ctx.site_pair_profiles(scan, best, site, widths, thr, 8).to_host()
    want = np.stack([md.pair_profile_batch(codes, gb[m], gs[m], widths[m], thr[m], 8) for m in range(2)])
    assert got.tobytes() == want.tobytes()
    assert got[0, 9].sum() > 0.9 * n
    for j in range(1, len(word)):
        assert got[0, 8 + j, 4 * "ACGT".index(word[j - 1]) + "ACGT".index(word[j])] > 0.9 * n


# ---- the first-order scan ------------------------------------------------------------------------------------------------
def model_best(seqs, models, both):
    return np.stack([md.best_scores(seqs, S0, D, both) for S0, D in models]).astype(np.int32)


@pytest.mark.parametrize("all_valid", [False, True], ids=["validity", "all_valid"])
@pytest.mark.parametrize("both", [True, False], ids=["both", "plus"])
def test_scan_equals_the_model(ctx, both, all_valid):
    rng = np.random.default_rng(211 + 2 * both + all_valid)
    seqs = random_seqs(rng)
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    models = [random_model(rng, w) for w in SCAN_WIDTHS]
    got = ctx.motif_scan_dinuc(scan, [m[0] for m in models], [m[1] for m in models], SCAN_WIDTHS, both, all_valid=all_valid).to_host()
    seen = [np.where(c == 0, 1, c).astype(np.uint8) for c in seqs] if all_valid else seqs
    want = model_best(seen, models, both)
    assert got.dtype == np.int32 and got.tobytes() == want.tobytes()
    lens = np.array([len(c) for c in seqs])
    for m, w in enumerate(SCAN_WIDTHS):
        assert np.all(got[m, lens < w] == pk.SCORE_SENTINEL) and np.any(got[m] != pk.SCORE_SENTINEL)
        if all_valid:
            assert np.all(got[m, lens >= w] != pk.SCORE_SENTINEL)
    assert np.any(np.abs(got[got != pk.SCORE_SENTINEL]) > 2000)


@pytest.mark.parametrize("both", [True, False], ids=["both", "plus"])
def test_the_degenerate_model_is_the_order0_scan(ctx, both):
    """D[c][4a + b] = S[c][b], S0 = S[0]: pengk_motif_scan's array, byte for byte -- the new kernel against the old one"""
    rng = np.random.default_rng(221 + both)
    seqs = random_seqs(rng)
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    S = [random_S(rng, w) for w in SCAN_WIDTHS]
    deg = [md.degenerate(s) for s in S]
    old = ctx.motif_scan(scan, S, SCAN_WIDTHS, both).to_host()
    new = ctx.motif_scan_dinuc(scan, [d[0] for d in deg], [d[1] for d in deg], SCAN_WIDTHS, both).to_host()
    assert new.tobytes() == old.tobytes()
    assert np.any(old != pk.SCORE_SENTINEL)


def test_a_palindromic_model_scores_the_same_on_both_strands(ctx):
    """S0 constant and D[c][4a + b] = D[w - c][4 (3 - b) + (3 - a)]: the - strand's score of a window is its + score"""
    rng = np.random.default_rng(231)
    seqs = random_seqs(rng)
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    models = []
    for w in SCAN_WIDTHS:
        _, D = random_model(rng, w)
        D = np.clip(D, -900, 900)
        P = D.copy()
        for c in range(1, w):
            for a in range(4):
                for b in range(4):
                    P[c, 4 * a + b] = D[c, 4 * a + b] + D[w - c, 4 * (3 - b) + (3 - a)]
        models.append((np.full(4, 17, np.int32), P))
    args = ([m[0] for m in models], [m[1] for m in models], SCAN_WIDTHS)
    two = ctx.motif_scan_dinuc(scan, *args, True).to_host()
    one = ctx.motif_scan_dinuc(scan, *args, False).to_host()
    assert two.tobytes() == one.tobytes() == model_best(seqs, models, False).tobytes()


@pytest.mark.parametrize("col", [2, 4, 16], ids=["inside_a_chunk", "chunks_0_1", "registers_15_16"])
def test_one_pair_term_scores_exactly_where_the_dinucleotide_is(ctx, col):
    """the model's only non-zero entries are those of columns col - 1 | col, for the pair CT: a sequence of A with one CT at
    position q scores 1000 on + exactly when a window holds the C at its column col - 1, else 0"""
    w, L = 20, 90
    S0, D = np.zeros(4, np.int32), np.zeros((w, 16), np.int32)
    D[col, 4 * 1 + 3] = 1000
    seqs = []
    for q in range(L - 1):
        c = np.ones(L, np.uint8)
        c[q], c[q + 1] = 2, 4
        seqs.append(c)
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    plus = ctx.motif_scan_dinuc(scan, [S0], [D], [w], False).to_host()[0]
    q = np.arange(L - 1)
    start = q - (col - 1)  # the window that holds the pair at its columns col - 1 | col
    assert np.array_equal(plus, np.where((start >= 0) & (start <= L - w), 1000, 0))
    assert plus.tobytes() == md.best_scores(seqs, S0, D, False).astype(np.int32).tobytes()
    # on -, CT reads AG and the A run reads T: nothing scores; a CT read on - (AG on +) does
    both = ctx.motif_scan_dinuc(scan, [S0], [D], [w], True).to_host()[0]
    assert np.array_equal(both, plus)
    rc = [5 - c[::-1] for c in seqs]
    scan_rc = ctx.upload_scan(pk.ScanLayout(*ms.flatten(rc)))
    got = ctx.motif_scan_dinuc(scan_rc, [S0], [D], [w], True).to_host()[0]
    assert np.array_equal(got, plus) and got.tobytes() == md.best_scores(rc, S0, D, True).astype(np.int32).tobytes()
    assert not ctx.motif_scan_dinuc(scan_rc, [S0], [D], [w], False).to_host()[0].any()


def test_argument_errors(ctx):
    seqs = [np.ones(40, np.uint8)]
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    S0, D = np.zeros(4, np.int32), np.zeros((8, 16), np.int32)
    bad = D.copy()
    bad[3, 5] = 2001
    for s0, d, w in [(S0, bad, 8), (S0 - 2001, D, 8), (S0, D, 0), (S0, np.zeros((65, 16), np.int32), 65)]:
        with pytest.raises(pk.PengkError) as e:
            ctx.motif_scan_dinuc(scan, [s0], [d[:pk.MAX_MOTIF_LEN]], [w], True)
        assert e.value.code == pk.ERR_ARG
    unused = D.copy()
    unused[0, 0] = 99999  # (row 0 is not read)
    assert not ctx.motif_scan_dinuc(scan, [S0], [unused], [8], True).to_host().any()


# ---- a planted dependency --------------------------------------------------------------------------------------------------
def device_analysis(ctx, seqs, S, both, pvalue, flank, alpha, bg0, bg1, seed=1):
    """motif_dinuc_model.analyse on the device calls (motif 0, order-0 sampled negatives)"""
    w = len(S)
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    lo, tail = pk.score_tail_pvalues(S, bg0)
    thr = [pk.score_threshold(tail, lo, pvalue)]
    best, site = ctx.motif_best_sites(scan, [S], [w], both)
    k1 = ctx.site_profiles(scan, best, site, [w], thr, flank).to_host()[0]
    k2 = ctx.site_pair_profiles(scan, best, site, [w], thr, flank).to_host()[0]
    mod = pk.dinuc_model(k1, k2, w, flank, bg0, bg1, alpha)
    mod["width"] = W = w + 2 * mod["flank"]
    neg = ctx.sample_background(scan, seed, 0, 0, ms.thresholds([bg0], 0))
    n = len(seqs)
    for k, D in (("auc0", mod["D0"]), ("auc1", mod["D1"])):
        a, b = md.score_range(mod["S0"], D)
        hp, _ = ctx.score_histograms(ctx.motif_scan_dinuc(scan, [mod["S0"]], [D], [W], both), n, [a], [b])
        hn, _ = ctx.score_histograms(ctx.motif_scan_dinuc(scan, [mod["S0"]], [D], [W], both, words=neg, all_valid=True), n, [a], [b])
        mod[k] = pk.score_summary(hp.to_host(), hn.to_host())[0]
    mod["gain"] = mod["auc1"] - mod["auc0"]
    mod["mi_total"], mod["mi_max"], mod["mi_max_pair"] = md.mi_summary(mod)
    return mod


def test_planted_dependency_is_found_and_pays(ctx):
    """seed PLANT_SEED: the model satisfies the conditions with it (tests/test_motif_dinuc_cpu.py checks them on the CPU,
    and they were checked there before the device was asked: dependent mi_max 0.82 bits at the planted pair, gain +0.031;
    control mi_max 0.02, gain +0.0004).  The device must give the model's numbers exactly."""
    S = ms.log_odds(planted_start_pwm(), UNIFORM)
    g1 = np.full(16, 0.25, np.float32)
    res = []
    for dependent in (True, False):
        want = planted_analysis(dependent)
        got = device_analysis(ctx, planted_seqs(PLANT_SEED, dependent), S, True, 1e-3, 0, 20.0, UNIFORM, g1)
        for k in ("q0", "q1", "mi", "S0", "D1", "D0"):
            assert got[k].tobytes() == want[k].tobytes(), k
        for k in ("sites", "auc0", "auc1", "gain", "mi_total", "mi_max", "mi_max_pair"):
            assert got[k] == want[k], k
        res.append(got)
    assert_planted_conditions(*res)


# ---- the CLI -----------------------------------------------------------------------------------------------------------
def mafk_model_inputs(fa):
    seqs = ms.read_fasta_codes(fa)
    codes, offs = ms.flatten(seqs)
    Vc = np.asarray(po.bg_V(po.bg_counts(codes, offs, 2), 2), np.float32)
    V = [Vc[0:4], Vc[4:20], Vc[20:84]]
    negs = [n + 1 for n in ms.sample([len(s) for s in seqs], 1, 0, 2, ms.thresholds(V, 2))]
    return seqs, negs, V


def assert_files_equal_the_model(inputs, js, report, models, both, pvalue=1e-4, flank=0, alpha=20.0, batch=True):
    """byte for byte: every motif's report line and models block against the model run from the log-odds the run scanned
    with (found_log_odds of tests/test_gpu_motif_refine.py; where an entry of them is ambiguous, against the model of one
    of its possible values -- at most 64 per motif, more fails the test).  From the counts on the run and the model hold
    the same integers.  inputs: (the input's sequences, the negatives, the background model V of orders 0..2), as
    mafk_model_inputs gives them for a FASTA file and sampled negatives; batch: the model's vectorised path."""
    seqs, negs, V = inputs
    pats = json.loads(js)["patterns"]
    lines = report.splitlines(True)
    assert lines[0] == md.REPORT_HEAD and len(lines) == 1 + len(pats)
    head, _, rest = models.partition("MOTIF ")
    blocks = ["MOTIF " + b for b in rest.split("MOTIF ")] if rest else []
    assert head == md.models_head(alpha, 2) and len(blocks) == len(pats)
    out = []
    for m, p in enumerate(pats):
        S, amb = found_log_odds(p["pwm"], V[0], pvalue)
        assert np.prod([len(vals) for _, vals in amb]) <= 64, (m, amb)
        want, seen = [], {}
        for pick in itertools.product(*[vals for _, vals in amb]):
            S1 = S.copy()
            for (idx, _), val in zip(amb, pick):
                S1[idx] = val
            k = md.site_counts(seqs, S1, m, both, pvalue, flank, V[0], batch=batch)
            key = k[0].tobytes() + k[1].tobytes()
            if key not in seen:
                seen[key] = md.analyse(seqs, negs, S1, m, V[0], V[1], both, pvalue, flank, alpha, batch=batch, counts=k)
            r = seen[key]
            want.append((md.report_line(p["iupac_motif"], m + 1, r), md.models_block(p["iupac_motif"], r)))
        assert (lines[1 + m], blocks[m]) in want, (m, lines[1 + m], want[0][0])
        out.append(seen[list(seen)[0]] if len(seen) == 1 else None)
    return out


def report_rows(text):
    rows = [l.split("\t") for l in text.splitlines()]
    return [dict(zip(rows[0], r)) for r in rows[1:]]


def test_cli_dinuc_equals_the_model_and_leaves_everything_else_alone(tmp_path):
    fa = os.path.join(GOLD, "MafK.fasta")
    rep, mod = tmp_path / "dinuc.tsv", tmp_path / "dinuc.models"
    rc, so, se, meme, js = run_plain([fa, "-w", "10", "--dinuc", str(rep), "--dinuc-models", str(mod)], tmp_path, tag="dn")
    assert rc == 0, se.decode()[-2000:]
    for ext, got in [("stdout", so), ("meme", meme), ("json", js)]:
        with open(os.path.join(GOLD, "cli", "cli_mafk_w10." + ext), "rb") as fh:
            assert got == fh.read(), ext
    assert_files_equal_the_model(mafk_model_inputs(fa), js, rep.read_text(), mod.read_text(), True)
    rows = report_rows(rep.read_text())
    assert rows[0]["motif"] == "CTGASTCAGCAAW" and rows[0]["index"] == "1" and rows[0]["width"] == "13" and rows[0]["flank"] == "0"
    assert int(rows[0]["sites"]) > 100 and 0.5 < float(rows[0]["auc_order0"]) < 1 and 1 <= int(rows[0]["mi_max_pair"]) - 1 < 13
    assert abs(float(rows[0]["auc_gain"]) - (float(rows[0]["auc_order1"]) - float(rows[0]["auc_order0"]))) < 2e-6
    # the other settings reach the run
    rep2, mod2 = tmp_path / "dinuc2.tsv", tmp_path / "dinuc2.models"
    args = ["--dinuc-pvalue", "1e-5", "--dinuc-flank", "3", "--dinuc-alpha", "5"]
    rc, so2, se, meme2, js2 = run_plain([fa, "-w", "10", "--dinuc", str(rep2), "--dinuc-models", str(mod2)] + args, tmp_path, tag="dn2")
    assert rc == 0, se.decode()[-2000:]
    assert (so2, meme2, js2) == (so, meme, js)
    assert_files_equal_the_model(mafk_model_inputs(fa), js2, rep2.read_text(), mod2.read_text(), True, 1e-5, 3, 5.0)
    rows2 = report_rows(rep2.read_text())
    assert rows2[0]["width"] == "19" and rows2[0]["flank"] == "3" and int(rows2[0]["sites"]) < int(rows[0]["sites"])
    assert mod2.read_text().startswith("# first-order motif models: alpha= 5 bg_order= 1\n")
    # the report alone
    rep3 = tmp_path / "dinuc3.tsv"
    rc, _, se, _, _ = run_plain([fa, "-w", "10", "--dinuc", str(rep3)], tmp_path, tag="dn3")
    assert rc == 0 and rep3.read_bytes() == rep.read_bytes()


def test_cli_dinuc_plus_strand(tmp_path):
    fa = os.path.join(GOLD, "MafK.fasta")
    rep, mod = tmp_path / "plus.tsv", tmp_path / "plus.models"
    rc, _, se, _, js = run_plain([fa, "-w", "10", "--strand", "PLUS", "--dinuc", str(rep), "--dinuc-models", str(mod)], tmp_path)
    assert rc == 0, se.decode()[-2000:]
    assert_files_equal_the_model(mafk_model_inputs(fa), js, rep.read_text(), mod.read_text(), False)


def test_cli_shuffled_negatives_change_the_aucs_and_nothing_else(tmp_path):
    fa = os.path.join(GOLD, "MafK.fasta")
    out = []
    for tag, extra in [("sampled", []), ("shuffled", ["--score-negatives", "shuffled"]), ("seed", ["--score-seed", "5"])]:
        rep, mod = tmp_path / (tag + ".tsv"), tmp_path / (tag + ".models")
        rc, so, se, meme, js = run_plain([fa, "-w", "10", "--dinuc", str(rep), "--dinuc-models", str(mod)] + extra, tmp_path, tag=tag)
        assert rc == 0, se.decode()[-2000:]
        out.append((so, meme, js, mod.read_bytes(), report_rows(rep.read_text())))
    for other in out[1:]:
        assert other[:4] == out[0][:4]
        for a, b in zip(out[0][4], other[4]):
            aucs = ("auc_order0", "auc_order1", "auc_gain")
            assert {k: v for k, v in a.items() if k not in aucs} == {k: v for k, v in b.items() if k not in aucs}
            assert (a["auc_order0"], a["auc_order1"]) != (b["auc_order0"], b["auc_order1"])


def test_cli_dinuc_beside_sites_centrality_and_refine(tmp_path):
    fa = os.path.join(GOLD, "MafK.fasta")
    names = ["s0.tsv", "c0.tsv", "r0.meme", "s1.tsv", "c1.tsv", "r1.meme", "d.tsv", "d.models"]
    s0, c0, r0, s1, c1, r1, d, dm = (tmp_path / n for n in names)
    rc, so0, se, meme0, js0 = run_plain([fa, "-w", "10", "--sites", str(s0), "--centrality", str(c0), "--refine", str(r0)],
                                        tmp_path, tag="a")
    assert rc == 0, se.decode()[-2000:]
    rc, so1, se, meme1, js1 = run_plain([fa, "-w", "10", "--sites", str(s1), "--centrality", str(c1), "--refine", str(r1),
                                         "--dinuc", str(d), "--dinuc-models", str(dm)], tmp_path, tag="b")
    assert rc == 0, se.decode()[-2000:]
    assert (so1, meme1, js1) == (so0, meme0, js0)
    assert s1.read_bytes() == s0.read_bytes() and c1.read_bytes() == c0.read_bytes() and r1.read_bytes() == r0.read_bytes()
    alone, alone_m = tmp_path / "alone.tsv", tmp_path / "alone.models"
    rc, _, se, _, _ = run_plain([fa, "-w", "10", "--dinuc", str(alone), "--dinuc-models", str(alone_m)], tmp_path, tag="c")
    assert rc == 0, se.decode()[-2000:]
    assert d.read_bytes() == alone.read_bytes() and dm.read_bytes() == alone_m.read_bytes()
    assert dm.read_bytes().count(b"MOTIF ") == len(json.loads(js0)["patterns"])


@pytest.mark.parametrize("world", [2, 3])
def test_cli_ranks_write_what_one_process_writes(tmp_path, world):
    fa = os.path.join(GOLD, "MafK.fasta")
    one, one_m = tmp_path / "one.tsv", tmp_path / "one.models"
    rc, so, se, meme, js = run_plain([fa, "-w", "10", "--dinuc", str(one), "--dinuc-models", str(one_m), "--dinuc-flank", "2"], tmp_path)
    assert rc == 0, se.decode()[-2000:]
    many, many_m = tmp_path / "many.tsv", tmp_path / "many.models"
    res = run_ranks([fa, "-w", "10", "--dinuc", str(many), "--dinuc-models", str(many_m), "--dinuc-flank", "2"], world, tmp_path)
    for rank, (rrc, rso, rse, rmeme, rjs) in enumerate(res):
        assert rrc == 0, (rank, rse.decode()[-2000:])
        if rank == 0:
            assert rmeme == meme and rjs == js and rso == so
    assert many.read_bytes() == one.read_bytes() and many_m.read_bytes() == one_m.read_bytes()


@pytest.mark.parametrize("args", [["--dinuc-models", "m.txt"], ["--dinuc", "d.tsv", "--dinuc-pvalue", "0"],
                                  ["--dinuc", "d.tsv", "--dinuc-pvalue", "1.5"], ["--dinuc", "d.tsv", "--dinuc-flank", "-1"],
                                  ["--dinuc", "d.tsv", "--dinuc-flank", "1001"], ["--dinuc", "d.tsv", "--dinuc-flank", "2x"],
                                  ["--dinuc", "d.tsv", "--dinuc-alpha", "0"], ["--dinuc", "d.tsv", "--dinuc-alpha", "abc"],
                                  ["--dinuc"]], ids=lambda a: "_".join(a).replace("--", ""))
def test_cli_argument_errors_exit_4(tmp_path, args):
    """as --refine's: the help, an ERROR line, exit 4 (before the input is read: no device is needed for it)"""
    fa = os.path.join(GOLD, "MafK.fasta")
    args = [str(tmp_path / a) if a.endswith((".txt", ".tsv")) else a for a in args]
    rc, so, se, _, _ = run_plain_args_last(fa, args, tmp_path)
    assert rc == 4 and b"ERROR" in se and b"--dinuc FILE" in so
    assert not list(tmp_path.glob("*.tsv")) and not list(tmp_path.glob("*.txt"))


def run_plain_args_last(fa, args, tmp_path):
    """run_plain with the flags under test behind -o / -j, so that a flag without its value is the last argument"""
    import subprocess
    from test_gpu_multirank import CLI, clean_env
    meme, js = tmp_path / "e.meme", tmp_path / "e.json"
    r = subprocess.run([CLI, fa, "-w", "10", "-o", str(meme), "-j", str(js)] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=clean_env(), timeout=900)
    return r.returncode, r.stdout, r.stderr, None, None
