"""Motif scoring on the device (include/pengk.h, "motif scoring"; the step scripts/shoot_peng.py adds after peng_motif)
against the numpy model of tests/motif_score_model.py: sampled negatives, best window scores and histograms bit for bit;
the CLI's --score-motifs output against the run without it, against the model and against its own multi-rank runs."""
import json
import os
import subprocess

import numpy as np
import pytest

import peng_motif_amd as pk
import motif_score_model as ms
from oracle import oracle as po
from test_gpu_multirank import clean_env, run_plain, run_ranks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "peng-motif_amd", "host", "peng_motif")
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def ctx():
    c = pk.Context(0)
    yield c
    c.close()


def unpack(words, offs, lens):
    out = []
    for o, L in zip(offs, lens):
        g = int(o) + np.arange(int(L))
        out.append(((words[g >> 5] >> (2 * (g & 31)).astype(np.uint64)) & np.uint64(3)).astype(np.uint8))
    return out


def random_V(rng):
    return [rng.dirichlet(np.ones(4) * 2, 4 ** k).astype(np.float32).reshape(-1) for k in range(3)]


def random_S(rng, w):
    S = rng.integers(-300, 301, (w, 4)).astype(np.int32)
    S[rng.random((w, 4)) < 0.05] = -2000
    S[rng.random((w, 4)) < 0.02] = 2000
    return S


@pytest.mark.parametrize("K", [0, 1, 2])
@pytest.mark.parametrize("seed,seq0", [(1, 0), (77, 12345), (2 ** 63 + 5, 3)])
def test_sampled_negatives_equal_the_model(ctx, K, seed, seq0):
    rng = np.random.default_rng(K * 7 + seq0)
    lens = [0, 1, 2, 31, 32, 33, 64, 65, 200] + rng.integers(0, 300, 40).tolist()
    seqs = [rng.integers(0, 5, n).astype(np.uint8) for n in lens]
    lay = pk.ScanLayout(*ms.flatten(seqs))
    scan = ctx.upload_scan(lay)
    th = ms.thresholds(random_V(rng), K)
    got = ctx.sample_background(scan, seed, seq0, K, th).to_host()
    want = ms.sample(lens, seed, seq0, K, th)
    for i, (g, w) in enumerate(zip(unpack(got, lay.offs, lay.lens), want)):
        assert np.array_equal(g, w), i


@pytest.mark.parametrize("fasta", ["MafK.fasta", "torture.fa"])
@pytest.mark.parametrize("both", [False, True], ids=["plus", "both"])
def test_best_scores_equal_the_model(ctx, fasta, both):
    seqs = ms.read_fasta_codes(os.path.join(GOLD, fasta))
    if fasta == "torture.fa":  # besides its N runs, lower case and short records: one without any valid base, tiny ones
        seqs = seqs + [np.zeros(30, np.uint8), np.array([1, 2, 0, 3, 4], np.uint8), np.array([2], np.uint8)]
    lay = pk.ScanLayout(*ms.flatten(seqs))
    scan = ctx.upload_scan(lay)
    rng = np.random.default_rng(len(seqs) + both)
    widths = [6, 10, 14, 21, 64] + ([3, 1] if fasta == "torture.fa" else [])
    S = [random_S(rng, w) for w in widths]
    best = ctx.motif_scan(scan, S, widths, both).to_host()
    for m, w in enumerate(widths):
        want = ms.best_scores(seqs, S[m], both)
        assert np.array_equal(best[m, :len(seqs)].astype(np.int64), want), (fasta, w)


def test_histograms_auc_and_occur_equal_the_model(ctx):
    seqs = ms.read_fasta_codes(os.path.join(GOLD, "MafK.fasta"))
    lay = pk.ScanLayout(*ms.flatten(seqs))
    scan = ctx.upload_scan(lay)
    rng = np.random.default_rng(9)
    widths = [8, 10, 12, 15]
    S = [random_S(rng, w) for w in widths]
    lo, hi = zip(*[ms.score_range(s) for s in S])
    th = ms.thresholds(random_V(rng), 2)
    neg = ctx.sample_background(scan, 3, 0, 2, th)
    hp, offs = ctx.score_histograms(ctx.motif_scan(scan, S, widths, True), len(seqs), lo, hi)
    hn, _ = ctx.score_histograms(ctx.motif_scan(scan, S, widths, True, words=neg, all_valid=True), len(seqs), lo, hi)
    hp, hn = hp.to_host(), hn.to_host()
    negs = [n + 1 for n in ms.sample([len(s) for s in seqs], 3, 0, 2, th)]
    for m in range(len(widths)):
        P = ms.histogram(ms.best_scores(seqs, S[m], True), lo[m], hi[m])
        N = ms.histogram(ms.best_scores(negs, S[m], True), lo[m], hi[m])
        gp, gn = hp[offs[m]:offs[m + 1]], hn[offs[m]:offs[m + 1]]
        assert np.array_equal(gp, P) and np.array_equal(gn, N), m
        assert pk.score_summary(gp, gn) == (ms.auc(P, N), ms.occur(P, N))


def test_cli_scores_rank_and_leave_everything_else_alone(tmp_path):
    fa = os.path.join(GOLD, "MafK.fasta")
    rc, _, se, meme0, js0 = run_plain([fa, "-w", "10"], tmp_path, tag="plain")
    assert rc == 0, se.decode()[-2000:]
    rc, _, se, meme1, js1 = run_plain([fa, "-w", "10", "--score-motifs"], tmp_path, tag="scored")
    assert rc == 0, se.decode()[-2000:]
    rc, _, se, meme2, js2 = run_plain([fa, "-w", "10", "--score-motifs"], tmp_path, tag="again")
    assert rc == 0 and meme2 == meme1 and js2 == js1
    a, b = json.loads(js0), json.loads(js1)
    assert a["bg"] == b["bg"] and len(a["patterns"]) == len(b["patterns"]) > 0
    # (log(Pval) and bg_prob are printed with the stream's state at their place: a motif that moves is printed
    # with another precision, so those two compare as numbers)
    key = lambda p: (p["iupac_motif"], p["sites"], p["pattern_length"])
    plain = {key(p): p for p in a["patterns"]}
    assert sorted(plain) == sorted(key(p) for p in b["patterns"])
    for p in b["patterns"]:
        q = dict(p)
        assert list(q)[6:8] == ["zoops_score", "occur"]  # right behind opt_bg_order
        del q["zoops_score"], q["occur"]
        r = plain[key(p)]
        assert list(q) == list(r)
        for f in q:
            if f in ("log(Pval)", "bg_prob"):
                assert abs(q[f] - r[f]) <= 1e-5 * abs(r[f]) + 1e-6, (f, q[f], r[f])
            else:
                assert q[f] == r[f], f
    z = [p["zoops_score"] for p in b["patterns"]]
    assert z == sorted(z, reverse=True)
    # MEME: the JSON's motifs in the JSON's order, the two fields behind log(Pval), nothing else changed
    lines = [l for l in meme1.decode().splitlines() if l.startswith("letter-probability matrix:")]
    assert len(lines) == len(b["patterns"])
    for l, p in zip(lines, b["patterns"]):
        f = l.split()
        assert f[-6] == "log(Pval)=" and f[-4] == "zoops_score=" and f[-2] == "occur="
        assert abs(float(f[-3]) - p["zoops_score"]) < 1e-6 and abs(float(f[-1]) - p["occur"]) < 1e-6
    assert meme0.decode().splitlines()[:6] == meme1.decode().splitlines()[:6]
    # the model, from the written PWMs and the input's background model (order 2, the CLI's default)
    seqs = ms.read_fasta_codes(fa)
    codes, offs = ms.flatten(seqs)
    Vc = np.asarray(po.bg_V(po.bg_counts(codes, offs, 2), 2), np.float32)
    V = [Vc[0:4], Vc[4:20], Vc[20:84]]
    negs = [n + 1 for n in ms.sample([len(s) for s in seqs], 1, 0, 2, ms.thresholds(V, 2))]
    for p in b["patterns"]:
        S = ms.log_odds(np.array(p["pwm"], np.float32), V[0])
        lo, hi = ms.score_range(S)
        P = ms.histogram(ms.best_scores(seqs, S, True), lo, hi)
        N = ms.histogram(ms.best_scores(negs, S, True), lo, hi)
        assert abs(ms.auc(P, N) - p["zoops_score"]) < 1e-3, p["iupac_motif"]
        assert abs(ms.occur(P, N) - p["occur"]) < 1e-3, p["iupac_motif"]


@pytest.mark.parametrize("world", [2, 3])
def test_cli_ranks_score_what_one_process_scores(tmp_path, world):
    args = [os.path.join(GOLD, "MafK.fasta"), "-w", "10", "--score-motifs", "--score-seed", "5"]
    rc, so, se, meme, js = run_plain(args, tmp_path)
    assert rc == 0, se.decode()[-2000:]
    res = run_ranks(args, world, tmp_path)
    for rank, (rrc, rso, rse, rmeme, rjs) in enumerate(res):
        assert rrc == 0, (rank, rse.decode()[-2000:])
        if rank == 0:
            assert rmeme == meme and rjs == js and rso == so


def planted_pwm():
    pwm = np.full((10, 4), 0.01, np.float32)
    for j, c in enumerate("GCTGAGTCAT"):
        pwm[j, "ACGT".index(c)] = 0.97
    return pwm


def test_planted_motif_is_found_and_a_random_one_is_not(ctx):
    n, L = 200000, 200
    scan = ctx.synth_scan(7, 0, n, L)
    rng = np.random.default_rng(4)
    bg = np.full(4, 0.25, np.float32)
    S = [ms.log_odds(planted_pwm(), bg), ms.log_odds(rng.dirichlet(np.ones(4), 10).astype(np.float32), bg)]
    lo, hi = zip(*[ms.score_range(s) for s in S])
    neg = ctx.sample_background(scan, 1, 0, 0, ms.thresholds([bg], 0))
    hp, offs = ctx.score_histograms(ctx.motif_scan(scan, S, [10, 10], True), n, lo, hi)
    hn, _ = ctx.score_histograms(ctx.motif_scan(scan, S, [10, 10], True, words=neg, all_valid=True), n, lo, hi)
    hp, hn = hp.to_host(), hn.to_host()
    z0, o0 = pk.score_summary(hp[offs[0]:offs[1]], hn[offs[0]:offs[1]])
    z1, _ = pk.score_summary(hp[offs[1]:offs[2]], hn[offs[1]:offs[2]])
    assert abs(o0 - 0.10) <= 0.03 and z0 > 0.53, (z0, o0)
    assert abs(z1 - 0.5) <= 0.01, z1


def test_configs2_size_sixteen_motifs(ctx):
    n, L = 10_000_000, 200
    scan = ctx.synth_scan(1, 0, n, L)
    rng = np.random.default_rng(16)
    widths = [10, 11, 12, 13, 14] * 3 + [12]
    S = [random_S(rng, w) for w in widths]
    lo, hi = zip(*[ms.score_range(s) for s in S])
    neg = ctx.sample_background(scan, 1, 0, 2, ms.thresholds(random_V(rng), 2))
    best = ctx.empty((len(widths), n), np.int32)
    hp, offs = ctx.score_histograms(ctx.motif_scan(scan, S, widths, True, best=best), n, lo, hi)
    hn, _ = ctx.score_histograms(ctx.motif_scan(scan, S, widths, True, words=neg, all_valid=True, best=best), n, lo, hi)
    hp, hn = hp.to_host(), hn.to_host()
    for m in range(len(widths)):
        assert int(hp[offs[m]:offs[m + 1]].sum()) == n and int(hn[offs[m]:offs[m + 1]].sum()) == n
        assert hp[offs[m]] == 0 and hn[offs[m]] == 0  # (every sequence has valid windows)


def test_help_lists_the_scoring_flags():
    r = subprocess.run([CLI, "-h"], stdout=subprocess.PIPE, env=clean_env())
    assert r.returncode == 0
    assert b"--score-motifs" in r.stdout and b"--score-seed" in r.stdout
