"""CPU checks of the control matching (tests/motif_match_model.py; include/pengk.h, "a control set matched to the input";
INTEGRATION.md 7n): the model's own invariants, pengk_match_quotas against it, the CLI's flag errors, and what the match
is for -- a GC-rich word that is in neither set looks enriched against an unmatched control and not against the matched
one.  No device compute here."""
import math
import os
import subprocess

import numpy as np
import pytest

import peng_motif_amd as pk
import motif_enrich_model as me
import motif_match_model as mm
import motif_score_model as ms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "peng-motif_amd", "host", "peng_motif")
GOLD = os.path.join(ROOT, "tests", "golden")


def test_library_and_wrapper_have_the_match():
    for name in ("pengk_seq_strata", "pengk_match_quotas", "pengk_select_strata"):
        assert hasattr(pk.lib(), name)
    assert hasattr(pk.Context, "seq_strata") and hasattr(pk.Context, "select_strata") and hasattr(pk, "match_quotas")


# ---- the model's own invariants ------------------------------------------------------------------------------------------
def test_length_bins_are_half_octaves():
    assert [mm.length_bin(L) for L in (1, 31, 47, 48, 63, 64, 95, 96, 127, 128, 6143, 6144, 70000)] == \
        [0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 14, 15, 15]
    for lb in range(16):
        lo, hi = mm.length_range(lb)
        assert mm.length_bin(lo) == lb and (lo == 1 or mm.length_bin(lo - 1) == lb - 1)
        assert hi is None or (mm.length_bin(hi) == lb and mm.length_bin(hi + 1) == lb + 1)


def test_strata_of_constructed_sequences():
    A, Cc, G, T, N = 1, 2, 3, 4, 0
    assert mm.stratum_of([], 10, True) == mm.NONE and mm.stratum_of([N, N, 9], 10, True) == mm.NONE
    assert mm.stratum_of([Cc] * 50, 10, True) == 1 * 10 + 9  # (gc = n: the last bin, not one beyond it)
    assert mm.stratum_of([Cc, A] * 25, 10, True) == 1 * 10 + 5  # (an exact multiple goes up)
    assert mm.stratum_of([Cc, A] * 25, 10, False) == 5
    assert mm.stratum_of([G, N, N, T], 2, True) == 1  # (the invalid bases count in the length, not in n)
    assert mm.stratum_of([G, N, N, T], 2, True, all_valid=True) == 0
    s, h = mm.strata([[Cc] * 50, [], [A] * 50], 10, True)
    assert s.tolist() == [19, mm.NONE, 10] and int(h.sum()) == 2 and h[19] == h[10] == 1


@pytest.mark.parametrize("G,use_length,all_valid", [(10, True, False), (1, True, False), (16, False, False), (7, True, True)])
def test_strata_at_once_equal_the_definition(G, use_length, all_valid):
    rng = np.random.default_rng(G)
    lens = [0, 1, 2, 31, 32, 33, 47, 48, 95, 96, 6143, 6144] + rng.integers(0, 400, 300).tolist()
    seqs = [rng.integers(0 if k % 3 == 0 else 1, 5, L).astype(np.uint8) for k, L in enumerate(lens)]
    s, h = mm.strata(seqs, G, use_length, all_valid)
    assert s.tolist() == [mm.stratum_of(c, G, use_length, all_valid) for c in seqs]
    assert int(h.sum()) == int((s != mm.NONE).sum())


def test_exactly_q_are_kept_and_evenly_spaced():
    for c in (1, 2, 3, 7, 64, 1000):
        for q in sorted({0, 1, c // 3, c // 2, c - 1, c}):
            if q < 0:
                continue
            kept = [r for r in range(c) if mm.kept_rank(r, q, c)]
            assert len(kept) == q, (c, q)
            # evenly spaced: the k-th kept rank is ceil((k + 1) c / q) - 1, so gaps differ by at most one
            assert kept == [-((-(k + 1) * c) // q) - 1 for k in range(q)]
            gaps = np.diff(kept)
            assert len(gaps) == 0 or gaps.max() - gaps.min() <= 1


def test_select_keeps_the_quota_of_every_stratum_in_file_order():
    rng = np.random.default_rng(3)
    s = rng.integers(0, 40, 5000).astype(np.uint16)
    s[rng.random(5000) < 0.02] = mm.NONE
    count = mm.histogram(s)
    quota = (count * rng.random(256)).astype(np.uint64)
    quota[5], quota[6] = count[5], 0
    sel = mm.select(s, count, quota)
    assert np.all(np.diff(sel) > 0) and not np.any(s[sel] == mm.NONE)
    assert np.array_equal(mm.histogram(s[sel]), quota)
    assert np.array_equal(sel[s[sel] == 5], np.flatnonzero(s == 5))


@pytest.mark.parametrize("cuts", [(0, 5000), (1, 2, 3), (1700, 3400), (5000, 5000), (13, 14, 4000, 4999)])
def test_the_union_over_any_sharding_is_the_one_shot_result(cuts):
    rng = np.random.default_rng(4)
    s = rng.integers(0, 256, 5000).astype(np.uint16)
    count = mm.histogram(s)
    quota = (count * rng.random(256)).astype(np.uint64)
    want = mm.select(s, count, quota)
    got, bounds = [], [0] + list(cuts) + [5000]
    for a, b in zip(bounds[:-1], bounds[1:]):
        got.append(a + mm.select(s[a:b], count, quota, rank0=mm.histogram(s[:a])))
    assert np.array_equal(np.concatenate(got), want)


# ---- pengk_match_quotas ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", [1, 2, 7])
def test_match_quotas_against_the_model(ratio):
    rng = np.random.default_rng(ratio)
    h_in = rng.integers(0, 1000, 256).astype(np.uint64)
    h_ctrl = rng.integers(0, 3000, 256).astype(np.uint64)
    h_in[:8], h_ctrl[4:12] = 0, 0
    q, short = pk.match_quotas(h_in, h_ctrl, ratio)
    wq, wshort = mm.quotas(h_in, h_ctrl, ratio)
    assert np.array_equal(q, wq) and short == wshort
    assert np.all(q <= h_ctrl) and np.all(q <= ratio * h_in)


def test_match_quotas_range_and_argument_errors():
    h = np.zeros(256, np.uint64)
    big = h.copy()
    big[200] = 2 ** 62
    q, short = pk.match_quotas(big, big, 2)  # 2^63 exactly: the last product that is allowed
    assert int(q[200]) == 2 ** 62 and short == 2 ** 62
    with pytest.raises(pk.PengkError) as e:
        pk.match_quotas(big, big, 3)
    assert e.value.code == pk.ERR_RANGE
    big[201] = 2 ** 62
    with pytest.raises(pk.PengkError) as e:  # every product fits, their sum does not
        pk.match_quotas(big, h, 2)
    assert e.value.code == pk.ERR_RANGE
    with pytest.raises(pk.PengkError) as e:
        pk.match_quotas(h, h, 0)
    assert e.value.code == pk.ERR_ARG


# ---- the CLI's flags ---------------------------------------------------------------------------------------------------------
def run_cli(args):
    return subprocess.run([CLI, os.path.join(GOLD, "MafK.fasta")] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)


def test_help_lists_the_control_flags():
    out = subprocess.run([CLI, "-h"], stdout=subprocess.PIPE).stdout.decode()
    for flag in ("--control-match ", "--control-match-gc-bins", "--control-ratio", "--control-match-report"):
        assert flag in out
    assert any("control:" in l for l in out.splitlines())


def test_control_needs_a_control_set(tmp_path):
    r = run_cli(["--score-motifs", "--score-negatives", "control", "-o", str(tmp_path / "o.meme")])
    assert r.returncode == 4, (r.returncode, r.stderr[-500:])
    assert b"--score-negatives control requires --background-sequences" in r.stderr.splitlines()[-2]
    assert not (tmp_path / "o.meme").exists()


@pytest.mark.parametrize("flag,bad", [("--control-match", "gc+length"), ("--control-match", "GC"), ("--control-match", ""),
                                      ("--control-match-gc-bins", "0"), ("--control-match-gc-bins", "17"),
                                      ("--control-match-gc-bins", "ten"), ("--control-match-gc-bins", "4.5"),
                                      ("--control-ratio", "0"), ("--control-ratio", "-1"), ("--control-ratio", "1.5"),
                                      ("--control-ratio", "")])
def test_bad_control_flags_are_refused(tmp_path, flag, bad):
    """as every other flag treats a bad argument: the help, the flag named in an error line, exit status 4, before anything
    is read or written"""
    r = run_cli(["--score-motifs", "--score-negatives", "control", "--background-sequences", os.path.join(GOLD, "MafK.fasta"), flag,
                 bad, "-o", str(tmp_path / "o.meme")])
    assert r.returncode == 4, (flag, bad, r.returncode, r.stderr[-500:])
    assert flag.encode() in r.stderr.splitlines()[-2] and not (tmp_path / "o.meme").exists()


@pytest.mark.parametrize("flag", ["--control-match", "--control-match-gc-bins", "--control-ratio", "--control-match-report"])
def test_control_flags_need_a_value(flag):
    r = run_cli([flag])
    assert r.returncode == 4 and ("No expression following " + flag).encode() in r.stderr


# ---- what the match is for ---------------------------------------------------------------------------------------------------
def scenario_figures(seed):
    """{none, matched}: (AUC, log10 adjusted p-value, enrichment, negatives) of the GC-rich word against the whole control
    and against the matched one, through the models of --score-motifs and --enrich"""
    pos, ctrl = mm.scenario(seed)
    c = np.concatenate(ctrl)
    bg0 = (np.bincount(c, minlength=5)[1:5] / len(c)).astype(np.float32)  # the background model is the control's
    pwm = mm.word_pwm(mm.GC_RICH_8MER)
    S = ms.log_odds(pwm, bg0)
    lo, hi = ms.score_range(S)
    _, h_in = mm.strata(pos)
    s_ctrl, h_ctrl = mm.strata(ctrl)
    quota, _ = mm.quotas(h_in, h_ctrl, 1)
    matched = [ctrl[i] for i in mm.select(s_ctrl, h_ctrl, quota)]
    P = me.Packed(pos)
    out = {}
    for name, neg in (("none", ctrl), ("matched", matched)):
        N = me.Packed(neg)
        auc = ms.auc(ms.histogram(me.best_scores(P, S, True), lo, hi), ms.histogram(me.best_scores(N, S, True), lo, hi))
        e = me.analyse(P, N, [pwm], bg0, 1e-3, True)[0]["summary"]
        out[name] = (auc, e["log10_adj_pvalue"], e["enrichment"], len(neg))
    return out


MARGIN = 0.1347 / 2


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_a_gc_rich_word_is_enriched_against_the_unmatched_control_only(seed):
    """The input is 2 000 x 100 bp at 60 % GC, the control 6 000 sequences at 30 % or 60 % GC and of 100 or 300 bp; the word
    GCCGCGGC is planted nowhere.  (The control's AT-rich share stands at 30 %, not 35 %: at 35 % the adjusted p-value
    against the whole control is 0.067 at seed 1, which calls nothing.)  Seen, seeds 1 / 2 / 3:
      AUC against the whole control 0.6678 / 0.6533 / 0.6601, against the matched one 0.4959 / 0.4814 / 0.5136;
      log10 adjusted p-value -1.76 / -4.52 / -31.11 against the whole control, 0 / 0 / -0.38 against the matched one.
    The gap |AUC - 0.5| unmatched minus matched is 0.1637 / 0.1347 / 0.1465; the smallest, 0.1347, halved is the margin."""
    f = scenario_figures(seed)
    print(seed, f)
    (auc_u, lp_u, en_u, n_u), (auc_m, lp_m, en_m, n_m) = f["none"], f["matched"]
    assert n_u == 6000 and 0 < n_m <= 2000
    assert auc_u > 0.5 and lp_u < math.log10(0.05) and en_u > 1.0  # enriched, by either measure
    assert lp_m > math.log10(0.05)  # not enriched
    assert abs(auc_u - 0.5) - abs(auc_m - 0.5) >= MARGIN


def test_the_report_of_the_scenario():
    pos, ctrl = mm.scenario(1, 200, 600)
    _, h_in = mm.strata(pos)
    _, h_ctrl = mm.strata(ctrl)
    quota, short = mm.quotas(h_in, h_ctrl, 1)
    lines = mm.report(h_in, h_ctrl, quota, 10, True).splitlines()
    assert lines[0] == mm.REPORT_HEADER.rstrip("\n")
    rows = [l.split("\t") for l in lines[1:]]
    assert {(r[0], r[1]) for r in rows} == {("96", "127"), ("256", "383")}
    assert sum(int(r[4]) for r in rows) == 200 and sum(int(r[5]) for r in rows) == 600
    assert sum(int(r[6]) for r in rows) == 200 - short
    assert all(int(r[6]) == min(int(r[4]), int(r[5])) for r in rows)
