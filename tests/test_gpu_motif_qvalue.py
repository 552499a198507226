"""The sites' q-values on the device (--sites-qvalue; include/pengk.h, pengk_sites_histograms) against the numpy model of
tests/motif_qvalue_model.py: the per-motif histograms of the site scores, the scored window strands and the site counts,
exact for every width, threshold, motif group, under contention, over several calls, beyond the workgroup-private bins
and at scale (the comparison README asks of a new scan kernel, built on tests/scan_batch_model.py); then the CLI's TSV
against the model, against the file without the flag and against its own multi-rank runs."""
import json
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import peng_motif_amd as pk
import motif_qvalue_model as mq
import motif_score_model as ms
import motif_sites_model as mst
import scan_batch_model as sbm
from oracle import oracle as po
from test_gpu_motif_centrality import sub_scan
from test_gpu_multirank import CLI, clean_env, run_plain, run_ranks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SCAN_TABLES, PRIV_BINS, LONG_SEQ = 40, 2560, 1 << 16  # csrc/scan_walk.h, csrc/sites.hip
BG = np.full(4, 0.25, np.float32)


@pytest.fixture(scope="module")
def ctx():
    c = pk.Context(0)
    yield c
    c.close()


def random_S(rng, w):
    S = rng.integers(-300, 301, (w, 4)).astype(np.int32)
    S[rng.random((w, 4)) < 0.05] = -2000
    S[rng.random((w, 4)) < 0.02] = 2000
    return S


def random_seqs(rng, n=300):
    """lengths 0..300 (the first few fixed: empty, below every width but 1, around the word size), N runs in most"""
    lens = [0, 1, 3, 4, 5, 12, 13, 31, 32, 33, 63, 64, 65, 300] + rng.integers(0, 301, n - 14).tolist()
    seqs = []
    for L in lens:
        c = rng.integers(1, 5, L).astype(np.uint8)
        for _ in range(int(rng.integers(0, 3))):
            if L:
                a = int(rng.integers(0, L))
                c[a:a + int(rng.integers(1, 20))] = 0
        seqs.append(c)
    return seqs


@pytest.fixture(scope="module")
def small(ctx):
    seqs = random_seqs(np.random.default_rng(1234))
    return seqs, ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))


def threshold_at(S, P):
    lo, tail = mst.tail_pvalues(S, BG)
    return mst.threshold(lo, tail, P)


def model(seqs, S, thr, both):
    """(hists, tests, counts[m, i]) of the per-sequence model"""
    hists, tests, counts = [], [], np.zeros((len(S), len(seqs)), np.uint64)
    for m, (s, t) in enumerate(zip(S, thr)):
        h, N = mq.histogram(seqs, s, t, both)
        hists.append(h)
        tests.append(N)
        sq = np.array([x[0] for x in mst.sites(seqs, s, t, both)], np.int64)
        counts[m] = np.bincount(sq, minlength=len(seqs)).astype(np.uint64)
    return hists, tests, counts


def run(ctx, scan, S, both, thr, with_counts=True, **kw):
    widths = [len(s) for s in S]
    hi = [mq.score_hi(s) for s in S]
    counts = ctx.empty((len(S), max(scan[4], 1)), np.uint64) if with_counts else None
    hists, tests = ctx.sites_histograms(scan, S, widths, both, thr, hi, counts=counts, **kw)
    return hists, [int(x) for x in tests], counts.to_host() if with_counts else None


def assert_equal(got, want, n_motifs):
    (gh, gt, gc), (wh, wt, wc) = got, want
    assert gt == [int(x) for x in wt]
    for m in range(n_motifs):
        assert gh[m].dtype == np.uint64 and len(gh[m]) == len(wh[m]), m
        assert np.array_equal(gh[m], wh[m]), (m, np.nonzero(gh[m] != wh[m])[0][:10])
        if gc is not None:
            assert int(gh[m].sum()) == int(gc[m].sum())
    if gc is not None:
        assert gc.tobytes() == np.ascontiguousarray(wc, np.uint64).tobytes()


# ---- 1. equals the model -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("both", [True, False], ids=["both", "plus"])
def test_histograms_tests_and_counts_equal_the_model(ctx, small, both):
    seqs, scan = small
    rng = np.random.default_rng(5 + both)
    widths = [1, 4, 5, 13, 64]
    S = [random_S(rng, w) for w in widths] * 2 + [random_S(rng, 8)]
    thr = [threshold_at(s, 1e-2) for s in S[:5]] + [threshold_at(s, 1.0) for s in S[5:10]] + [mq.score_hi(S[10]) + 1]
    assert thr[5:10] == [int(s.min(axis=1).sum()) for s in S[5:10]]  # P = 1: t = lo, every scored strand is a site
    want = model(seqs, S, thr, both)
    assert len(want[0][10]) == 0 and want[2][10].sum() == 0  # no bins
    assert all(int(want[0][m].sum()) == want[1][m] > 1000 for m in range(5, 10))
    assert len(want[0][0]) == 0  # (w = 1: no base is as rare as 1e-2, t = hi + 1)
    assert all(0 < int(want[0][m].sum()) < want[1][m] for m in range(1, 5))
    assert want[1][0] == want[1][5] and (want[1][0] == 2 * sum(int(((c >= 1) & (c <= 4)).sum()) for c in seqs) // (1 if both else 2))
    got = run(ctx, scan, S, both, thr)
    assert_equal(got, want, len(S))
    # the counts are pengk_sites_count's, bit for bit
    assert got[2].tobytes() == ctx.sites_count(scan, S, [len(s) for s in S], both, thr).to_host().tobytes()
    # without d_counts: the same histograms
    again = run(ctx, scan, S, both, thr, with_counts=False)
    assert_equal(again, want, len(S))


# ---- 2. more than one motif group --------------------------------------------------------------------------------------
def test_three_motif_groups_with_guard_words_between_the_motifs(ctx, small):
    seqs, scan = small
    rng = np.random.default_rng(14)
    S = [random_S(rng, 14) for _ in range(12)]
    assert 12 * 8 > 2 * SCAN_TABLES and SCAN_TABLES // 8 == 5  # 8 tables each on both strands, 5 motifs a group: 3 groups
    thr = [threshold_at(s, 0.03) - 7 * m for m, s in enumerate(S)]  # distinct: one staged at another's record shows
    nb = [mq.n_bins(s, t) for s, t in zip(S, thr)]
    G = 3  # guard words before every motif's bins and after the last
    offs = np.cumsum([G] + [b + G for b in nb])[:-1]
    MARK = np.uint64(0xABCDABCDABCDABCD)
    buf = np.full(int(offs[-1]) + nb[-1] + G, MARK)
    for o, b in zip(offs, nb):
        buf[o:o + b] = 0
    d = ctx.to_device(buf)
    got = run(ctx, scan, S, True, thr, hist=d, offs=offs)
    want = model(seqs, S, thr, True)
    assert min(int(h.sum()) for h in want[0]) > 100
    assert_equal(got, want, len(S))
    after = d.to_host()
    guard = np.ones(len(buf), bool)
    for o, b in zip(offs, nb):
        guard[o:o + b] = False
    assert guard.sum() == 13 * G and np.all(after[guard] == MARK)


# ---- 3. contention -----------------------------------------------------------------------------------------------------
def planted_set(rng, S, n, L, moving):
    """n copies of one random sequence with the consensus of S at one position -- the same in every copy, or one that
    moves with the sequence index"""
    cons = (np.argmax(S, axis=1) + 1).astype(np.uint8)
    codes = np.tile(rng.integers(1, 5, L).astype(np.uint8), (n, 1))
    pos = (np.arange(n) * 7) % (L - len(cons) + 1) if moving else np.full(n, 20)
    codes[np.arange(n)[:, None], pos[:, None] + np.arange(len(cons))[None, :]] = cons[None, :]
    return codes


@pytest.mark.parametrize("P", [1e-4, 1.0], ids=["p1e-4", "p1"])
@pytest.mark.parametrize("moving", [False, True], ids=["fixed", "moving"])
def test_contended_bins_are_exact(ctx, moving, P):
    rng = np.random.default_rng(77)
    n, L = 20000, 64
    S = [ms.log_odds(np.where(np.eye(4)[rng.integers(0, 4, 10)] > 0, 0.97, 0.01).astype(np.float32), BG), random_S(rng, 11)]
    codes = planted_set(rng, S[0], n, L, moving)
    scan = ctx.upload_scan(pk.ScanLayout(codes.reshape(-1), np.arange(n + 1, dtype=np.int64) * L))
    thr = [threshold_at(s, P) for s in S]
    want_h, want_t, want_c = [], [], []
    for s, t in zip(S, thr):
        h, N = mq.histogram_batch(codes, s, t, True)
        want_h.append(h)
        want_t.append(N)
        want_c.append(sbm.site_counts(codes, s, t, True))
    assert want_h[0][-1] >= n  # every sequence adds to the top bin of motif 0 (a wave's 64 lanes at the same step when fixed)
    if P == 1.0:
        assert int(want_h[0].sum()) == want_t[0] == n * (L - 9) * 2
    assert_equal(run(ctx, scan, S, True, thr), (want_h, want_t, np.stack(want_c)), 2)


# ---- 4. adds, does not overwrite ---------------------------------------------------------------------------------------
def test_two_halves_and_a_prefilled_array_add_up(ctx, small):
    seqs, scan = small
    rng = np.random.default_rng(41)
    S = [random_S(rng, w) for w in [6, 13, 20]]
    thr = [threshold_at(s, 0.02) for s in S]
    whole = run(ctx, scan, S, True, thr)
    nb = [mq.n_bins(s, t) for s, t in zip(S, thr)]
    pre_h = rng.integers(0, 2 ** 40, sum(nb)).astype(np.uint64)
    pre_t = rng.integers(0, 2 ** 40, 3).astype(np.uint64)
    d_h, d_t = ctx.to_device(pre_h), ctx.to_device(pre_t)
    k, n = 131, len(seqs)
    parts = []
    for i0, i1 in [(0, k), (k, n)]:
        parts.append(run(ctx, sub_scan(scan, i0, i1), S, True, thr, hist=d_h, tests=d_t))
    hists, tests, _ = parts[-1]  # (the arrays' content after the second call)
    offs = np.concatenate([[0], np.cumsum(nb)])
    for m in range(3):
        assert np.array_equal(hists[m], whole[0][m] + pre_h[offs[m]:offs[m + 1]]), m
    assert tests == [a + int(b) for a, b in zip(whole[1], pre_t)]
    assert np.concatenate([parts[0][2], parts[1][2]], axis=1).tobytes() == whole[2].tobytes()
    assert_equal(whole, model(seqs, S, thr, True), 3)


# ---- 5. the range beyond any private bins ------------------------------------------------------------------------------
def test_a_quarter_million_bins(ctx):
    rng = np.random.default_rng(64)
    S = [np.where(rng.random((64, 4)) < 0.5, -2000, 2000).astype(np.int32)]
    S[0][np.arange(64), rng.integers(0, 4, 64)] = 2000  # (every column reaches 2000)
    S[0][np.arange(64), (np.argmax(S[0], axis=1) + 1) % 4] = -2000
    seqs = [rng.integers(1, 5, L).astype(np.uint8) for L in rng.integers(64, 400, 40)]
    seqs[3][5:69] = np.argmax(S[0], axis=1) + 1  # the top bin
    t = threshold_at(S[0], 1.0)
    assert mq.n_bins(S[0], t) == 64 * 4000 + 1 > 100 * PRIV_BINS
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    want = model(seqs, S, [t], True)
    assert want[0][0][-1] >= 1 and np.count_nonzero(want[0][0][:-PRIV_BINS]) > 10  # (scores 4000 apart)
    assert_equal(run(ctx, scan, S, True, [t]), want, 1)


# ---- 6. at scale, through the batch model ------------------------------------------------------------------------------
def test_a_million_short_sequences(ctx):
    n, L = 1_000_003, 20
    assert n > ctx.info("num_cu") * 8 * 256 and n % 256  # more than one trip of the grid-stride loop, a ragged last one
    rng = np.random.default_rng(606)
    codes = rng.integers(1, 5, (n, L), dtype=np.uint8)
    codes[rng.integers(0, 100, (n, L), dtype=np.uint8) == 0] = 0
    S = [random_S(rng, 4), random_S(rng, 10)]
    thr = [threshold_at(s, 0.02) for s in S]
    scan = ctx.upload_scan(pk.ScanLayout(codes.reshape(-1), np.arange(n + 1, dtype=np.int64) * L))
    got = run(ctx, scan, S, True, thr, with_counts=False)
    with ThreadPoolExecutor(2) as ex:  # (numpy releases the GIL in its inner loops)
        want = list(ex.map(lambda m: mq.histogram_batch(codes, S[m], thr[m], True), range(2)))
    assert min(int(h.sum()) for h, _ in want) > 10 ** 5
    assert_equal(got, ([h for h, _ in want], [N for _, N in want], None), 2)


def test_long_sequences_on_both_sides_of_the_private_bins_bound(ctx):
    rng = np.random.default_rng(4242)
    lens = [LONG_SEQ - 1, LONG_SEQ, LONG_SEQ + 1, 200000, 300]
    seqs = [rng.integers(1, 5, L).astype(np.uint8) for L in lens]
    seqs[2][65530:65546] = 0
    S = [random_S(rng, w) for w in [10, 33]]
    for i in [1, 3]:  # the top bins from a sequence that may use the private bins and from one that may not
        seqs[i][-10:] = np.argmax(S[0], axis=1) + 1
    thr = [threshold_at(s, 0.04) for s in S]
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    want = model(seqs, S, thr, True)
    assert want[0][0][-1] >= 2 and int(want[2][0][3]) > 5000
    assert_equal(run(ctx, scan, S, True, thr), want, 2)


def test_a_hundred_motifs(ctx, small):
    seqs, scan = small
    rng = np.random.default_rng(100)
    widths = rng.integers(1, 5, 100).tolist()  # one table each on the + strand: 40 a group, 64 private bins a motif
    S = [random_S(rng, w) for w in widths]
    thr = [threshold_at(s, 1.0 if m % 10 == 0 else 0.1) for m, s in enumerate(S)]
    assert len(S) > 2 * SCAN_TABLES and max(mq.n_bins(s, t) for s, t in zip(S, thr)) > PRIV_BINS // SCAN_TABLES
    k = 100  # (the first hundred sequences: the model walks them once per motif)
    assert_equal(run(ctx, sub_scan(scan, 0, k), S, False, thr), model(seqs[:k], S, thr, False), 100)


def test_arguments_are_checked_and_empty_inputs_do_nothing(ctx, small):
    seqs, scan = small
    S = [random_S(np.random.default_rng(1), 6)]
    hi = mq.score_hi(S[0])
    with pytest.raises(pk.PengkError):  # a score above h_hi would have no bin
        ctx.sites_histograms(scan, S, [6], True, [hi - 50], [hi - 1])
    h, t = ctx.sites_histograms(scan, [], [], True, [], [])
    assert h == [] and len(t) == 0
    empty = (scan[0], scan[1], scan[2], scan[3], 0)
    h, t = ctx.sites_histograms(empty, S, [6], True, [hi - 50], [hi])
    assert not h[0].any() and len(h[0]) == 51 and int(t[0]) == 0


# ---- 7. the CLI --------------------------------------------------------------------------------------------------------
def drop_q(text):
    return "".join("\t".join(l.split("\t")[:8] + l.split("\t")[9:]) for l in text.splitlines(True))


def read_scores(path):
    """the integer log-odds matrices the run scanned with (PENGK_SITES_SCORES: the JSON's PWMs are rounded, and written
    after the writers' pseudo count, so they do not give them back -- test_gpu_motif_sites.assert_cli_equals_model
    allows for that line by line; here the files are compared byte for byte)"""
    rows = [[int(x) for x in l.split()] for l in open(path)]
    out, k = [], 0
    while k < len(rows):
        w = rows[k][1]
        out.append(np.array(rows[k + 1:k + 1 + w], np.int32))
        k += 1 + w
    return out


def cli_model_inputs(fa, js, scores):
    seqs = ms.read_fasta_codes(fa)
    codes, offs = ms.flatten(seqs)
    bg = np.asarray(po.bg_V(po.bg_counts(codes, offs, 2), 2), np.float32)[0:4]
    names = mst.read_fasta_names(fa)
    pats = json.loads(js)["patterns"]
    Ss = read_scores(scores)
    assert [len(S) for S in Ss] == [len(p["pwm"]) for p in pats]
    return seqs, names, [p["iupac_motif"] for p in pats], Ss, bg


@pytest.mark.parametrize("fa,w,P", [("MafK_100seqs.fasta", "8", None), ("MafK.fasta", "10", None), ("MafK_100seqs.fasta", "8", "1e-2")],
                         ids=["mafk100_w8", "mafk_w10", "mafk100_w8_p1e-2"])
def test_cli_qvalue_file_equals_the_model_and_the_rest_is_unchanged(tmp_path, fa, w, P):
    fa = os.path.join(GOLD, fa)
    plain, qf, qmax = tmp_path / "plain.tsv", tmp_path / "q.tsv", tmp_path / "qmax.tsv"
    base = [fa, "-w", w] + (["--sites-pvalue", P] if P else [])
    P = float(P or 1e-4)
    scores = tmp_path / "scores.txt"
    rc, so0, se, meme0, js0 = run_plain(base + ["--sites", str(plain)], tmp_path, tag="plain", extra_env={"PENGK_SITES_SCORES": str(scores)})
    assert rc == 0, se.decode()[-2000:]
    rc, so1, se, meme1, js1 = run_plain(base + ["--sites", str(qf), "--sites-qvalue"], tmp_path, tag="q")
    assert rc == 0, se.decode()[-2000:]
    assert (so1, meme1, js1) == (so0, meme0, js0)
    text = qf.read_text()
    assert drop_q(text) == plain.read_text() and text.count("\n") > (20 if P > 1e-4 or w == "10" else 1)
    seqs, names, ids, Ss, bg = cli_model_inputs(fa, js0, scores)
    assert len(Ss) > 0
    assert mst.render(seqs, names, ids, Ss, bg, P, True) == plain.read_text()
    assert text == mq.render(seqs, names, ids, Ss, bg, P, True)
    # --sites-qvalue-max: exactly the model's subset, the q-values those of the whole set
    rc, so2, se, meme2, js2 = run_plain(base + ["--sites", str(qmax), "--sites-qvalue-max", "0.05"], tmp_path, tag="qmax")
    assert rc == 0, se.decode()[-2000:]
    assert (so2, meme2, js2) == (so0, meme0, js0)
    sub = qmax.read_text()
    assert sub == mq.render(seqs, names, ids, Ss, bg, P, True, Q=0.05)
    lines, kept = text.splitlines(True), sub.splitlines(True)
    assert kept == [lines[0]] + [l for l in lines[1:] if float(l.split("\t")[8]) <= 0.05]
    assert all(float(l.split("\t")[8]) <= 0.05 for l in kept[1:])


def test_cli_plus_strand_halves_the_tests(tmp_path):
    fa = os.path.join(GOLD, "MafK_100seqs.fasta")
    plain, qf = tmp_path / "plain.tsv", tmp_path / "q.tsv"
    base = [fa, "-w", "8", "--strand", "PLUS", "--sites-pvalue", "1e-2"]
    scores = tmp_path / "scores.txt"
    rc, _, se, _, js = run_plain(base + ["--sites", str(plain)], tmp_path, tag="plain", extra_env={"PENGK_SITES_SCORES": str(scores)})
    assert rc == 0, se.decode()[-2000:]
    rc, _, se, _, _ = run_plain(base + ["--sites", str(qf), "--sites-qvalue"], tmp_path, tag="q")
    assert rc == 0, se.decode()[-2000:]
    seqs, names, ids, Ss, bg = cli_model_inputs(fa, js, scores)
    text = qf.read_text()
    assert text == mq.render(seqs, names, ids, Ss, bg, 1e-2, False) and text.count("\n") > 20
    assert all(l.split("\t")[5] == "+" for l in text.splitlines()[1:])
    for S in Ss:
        t = threshold_at_bg(S, bg, 1e-2)
        assert 2 * mq.histogram(seqs, S, t, False)[1] == mq.histogram(seqs, S, t, True)[1] > 0


def threshold_at_bg(S, bg, P):
    lo, tail = mst.tail_pvalues(S, bg)
    return mst.threshold(lo, tail, P)


@pytest.mark.parametrize("bad", ["0", "2", "x"])
def test_cli_refuses_a_bad_qvalue_max(tmp_path, bad):
    r = subprocess.run([CLI, os.path.join(GOLD, "MafK_100seqs.fasta"), "--sites", str(tmp_path / "s.tsv"), "--sites-qvalue-max", bad],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=clean_env(), timeout=60)
    assert r.returncode == 4 and b"--sites-qvalue-max" in r.stderr


@pytest.mark.parametrize("world", [2, 3])
def test_cli_ranks_write_what_one_process_writes(tmp_path, world):
    fa = os.path.join(GOLD, "MafK.fasta")
    for tag, extra in [("q", ["--sites-qvalue"]), ("qmax", ["--sites-qvalue-max", "0.05"])]:
        one, many = tmp_path / (tag + "_one.tsv"), tmp_path / (tag + "_many.tsv")
        args = [fa, "-w", "10", "--sites-pvalue", "1e-3"] + extra
        rc, so, se, meme, js = run_plain(args + ["--sites", str(one)], tmp_path, tag=tag)
        assert rc == 0, se.decode()[-2000:]
        res = run_ranks(args + ["--sites", str(many)], world, tmp_path, tag=tag + "r")
        for rank, (rrc, rso, rse, rmeme, rjs) in enumerate(res):
            assert rrc == 0, (rank, rse.decode()[-2000:])
            if rank == 0:
                assert rmeme == meme and rjs == js and rso == so
        assert many.read_bytes() == one.read_bytes() and one.read_bytes().count(b"\n") > 20
