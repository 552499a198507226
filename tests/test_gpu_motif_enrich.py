"""The database enrichment on the device (--enrich; include/pengk.h, pengk_motif_enrich) against the numpy model of
tests/motif_enrich_model.py: the histograms of the sequences' best scores and the scored counts, exact for every width,
threshold and strand setting, over several motif groups and launches, under contention, over several calls, and against
pengk_motif_scan's own d_best at a size the model does not walk; then the CLI's TSV against the model, against its own
multi-rank runs, and the other outputs against the run without the flag."""
import os

import numpy as np
import pytest

import peng_motif_amd as pk
import motif_compare_model as mc
import motif_enrich_model as me
import motif_score_model as ms
import motif_sites_model as mst
from oracle import oracle as po
from test_gpu_motif_centrality import sub_scan
from test_gpu_motif_qvalue import random_S, random_seqs
from test_gpu_multirank import run_plain, run_ranks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SCAN_TABLES, PRIV_BINS = 40, 2560  # csrc/scan_walk.h, csrc/sites.hip
BG = np.full(4, 0.25, np.float32)


@pytest.fixture(scope="module")
def ctx():
    c = pk.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def small(ctx):
    seqs = random_seqs(np.random.default_rng(1234))
    return seqs, me.Packed(seqs), ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))


def threshold_at(S, P):
    lo, tail = mst.tail_pvalues(S, BG)
    return mst.threshold(lo, tail, P)


def model(packed, S, thr, both):
    """(hists, scored) of the model"""
    out = [me.histogram(me.best_scores(packed, s, both), t, me.score_hi(s)) for s, t in zip(S, thr)]
    return [h for h, _ in out], [n for _, n in out]


def run(ctx, scan, S, both, thr, **kw):
    hists, scored = ctx.motif_enrich(scan, S, [len(s) for s in S], both, thr, [me.score_hi(s) for s in S], **kw)
    return hists, [int(x) for x in scored]


def assert_equal(got, want):
    (gh, gs), (wh, ws) = got, want
    assert gs == [int(x) for x in ws]
    assert len(gh) == len(wh)
    for m in range(len(wh)):
        assert gh[m].dtype == np.uint64 and len(gh[m]) == len(wh[m]), m
        assert np.array_equal(gh[m], wh[m]), (m, np.nonzero(gh[m] != wh[m])[0][:10])


# ---- 1. equals the model -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("both", [True, False], ids=["both", "plus"])
def test_histograms_and_scored_counts_equal_the_model(ctx, small, both):
    seqs, packed, scan = small
    rng = np.random.default_rng(5 + both)
    widths = [1, 4, 5, 13, 64]
    S = [random_S(rng, w) for w in widths] * 3
    thr = ([threshold_at(s, 1e-2) for s in S[:5]] + [int(s.min(axis=1).sum()) for s in S[5:10]] +
           [me.score_hi(s) + 1 for s in S[10:]])
    want = model(packed, S, thr, both)
    # at lo every scored sequence lands in a bin; at hi + 1 there is no bin; the scored counts depend on the width alone
    assert all(int(want[0][m].sum()) == want[1][m] > 0 for m in range(5, 10))
    assert all(len(want[0][m]) == 0 for m in range(10, 15))
    assert all(0 < int(want[0][m].sum()) <= want[1][m] for m in range(1, 5))
    assert any(int(want[0][m].sum()) < want[1][m] for m in range(1, 5))
    assert want[1][:5] == want[1][5:10] == want[1][10:] and want[1][0] > want[1][3] > want[1][4] > 0
    assert_equal(run(ctx, scan, S, both, thr), want)


def test_without_validity_words(ctx):
    rng = np.random.default_rng(9)
    seqs = [rng.integers(1, 5, L).astype(np.uint8) for L in [0, 1, 9, 10, 11, 31, 32, 33, 64, 65] + rng.integers(0, 200, 150).tolist()]
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    S = [random_S(rng, w) for w in (1, 10, 33)]
    thr = [threshold_at(s, 0.05) for s in S]
    want = model(me.Packed(seqs), S, thr, True)
    assert want[1] == [sum(len(s) >= w for s in seqs) for w in (1, 10, 33)]
    assert_equal(run(ctx, scan, S, True, thr, all_valid=True), want)
    assert_equal(run(ctx, scan, S, True, thr), want)


# ---- 2. several groups, several launches ---------------------------------------------------------------------------------
def test_a_hundred_motifs_over_the_launch_seam(ctx, small):
    seqs, packed, scan = small
    rng = np.random.default_rng(100)
    widths = rng.integers(1, 14, 100).tolist()
    S = [random_S(rng, w) for w in widths]
    thr = [threshold_at(s, 1.0 if m % 10 == 0 else 0.05) for m, s in enumerate(S)]
    tables = sum(2 * ((w + 3) // 4) for w in widths)
    assert tables > 3 * SCAN_TABLES  # more than three groups, whatever the packing
    want = model(packed, S, thr, True)
    default = ctx.info("enrich_groups_per_launch")
    assert default >= 1
    results = []
    try:
        for per_launch in (1, 2, default):
            ctx.set_option("enrich_groups_per_launch", per_launch)
            assert ctx.info("enrich_groups_per_launch") == per_launch
            results.append(run(ctx, scan, S, True, thr))
    finally:
        ctx.set_option("enrich_groups_per_launch", default)
    for got in results:
        assert_equal(got, want)
    with pytest.raises(pk.PengkError):
        ctx.set_option("enrich_groups_per_launch", 0)
    assert ctx.info("enrich_groups_per_launch") == default


# ---- 3. contention -------------------------------------------------------------------------------------------------------
def test_twenty_thousand_sequences_in_one_bin(ctx):
    """20 000 copies of one 40-base sequence under a 10-mer that matches it, the top score inside the private bins; then --
    a motif of width 64 has no window on 40 bases -- 20 000 copies of one 64-base sequence under a width-64 motif at its
    lowest threshold, whose 256 001 bins exceed the private ones: one global bin takes all 20 000"""
    rng = np.random.default_rng(77)
    n, L = 20000, 40
    seq = rng.integers(1, 5, L).astype(np.uint8)
    codes = np.tile(seq, (n, 1))
    scan = ctx.upload_scan(pk.ScanLayout(codes.reshape(-1), np.arange(n + 1, dtype=np.int64) * L))
    # a motif that matches the sequence at position 20: the top score, inside the private bins
    cons = seq[20:30] - 1
    S10 = ms.log_odds(np.where(np.eye(4)[cons] > 0, 0.97, 0.01).astype(np.float32), BG)
    # and a width-64 motif of +-2000 at its lowest threshold: 256 001 bins, the sequence's best far below the private ones
    S64 = np.where(rng.random((64, 4)) < 0.5, -2000, 2000).astype(np.int32)
    S64[np.arange(64), rng.integers(0, 4, 64)] = 2000  # (every column reaches 2000 ...
    S64[np.arange(64), (np.argmax(S64, axis=1) + 1) % 4] = -2000  # ... and -2000)
    seq64 = np.tile(rng.integers(1, 5, 64).astype(np.uint8), (n, 1))
    scan64 = ctx.upload_scan(pk.ScanLayout(seq64.reshape(-1), np.arange(n + 1, dtype=np.int64) * 64))
    for sc, S, one, private in ((scan, S10, [seq], True), (scan64, S64, [seq64[0]], False)):
        hi, lo = me.score_hi(S), int(S.min(axis=1).sum())
        thr = threshold_at(S, 1e-3) if private else lo
        b = int(me.best_scores(me.Packed(one), S, True)[0])
        per = PRIV_BINS  # (one motif in the group: all private bins are its own)
        assert (b > hi - per) == private and b >= thr
        if private:
            assert b == hi
        else:
            assert hi - thr + 1 == 64 * 4000 + 1
        hists, scored = run(ctx, sc, [S], True, [thr])
        assert scored == [n]
        assert int(hists[0][b - thr]) == n and int(hists[0].sum()) == n


# ---- 4. adds, does not overwrite -----------------------------------------------------------------------------------------
def test_two_halves_and_a_prefilled_array_add_up(ctx, small):
    seqs, packed, scan = small
    rng = np.random.default_rng(41)
    S = [random_S(rng, w) for w in [6, 13, 20]]
    thr = [threshold_at(s, 0.05) for s in S]
    whole = run(ctx, scan, S, True, thr)
    assert_equal(whole, model(packed, S, thr, True))
    nb = [len(h) for h in whole[0]]
    pre_h = rng.integers(0, 2 ** 40, sum(nb)).astype(np.uint64)
    pre_s = rng.integers(0, 2 ** 40, 3).astype(np.uint64)
    d_h, d_s = ctx.to_device(pre_h), ctx.to_device(pre_s)
    k, n = 131, len(seqs)
    for i0, i1 in [(0, k), (k, n)]:
        hists, scored = run(ctx, sub_scan(scan, i0, i1), S, True, thr, hist=d_h, scored=d_s)
    offs = np.concatenate([[0], np.cumsum(nb)])
    for m in range(3):
        assert np.array_equal(hists[m], whole[0][m] + pre_h[offs[m]:offs[m + 1]]), m
    assert scored == [a + int(b) for a, b in zip(whole[1], pre_s)]


# ---- 5. independent of the model: pengk_motif_scan's own best scores -----------------------------------------------------
def test_equals_the_histograms_of_the_scan_on_synthetic_sequences(ctx):
    n, L = 20000, 120
    scan = ctx.synth_scan(11, 0, n, L)
    rng = np.random.default_rng(60)
    widths = rng.integers(4, 21, 60).tolist()
    S = [random_S(rng, w) for w in widths]
    thr = [threshold_at(s, 1e-2) if m % 3 else int(s.min(axis=1).sum()) for m, s in enumerate(S)]
    best = ctx.motif_scan(scan, S, widths, True).to_host()[:, :n].astype(np.int64)
    hists, scored = run(ctx, scan, S, True, thr)
    total = 0
    for m in range(60):
        had = best[m] != pk.SCORE_SENTINEL
        hi = me.score_hi(S[m])
        want = np.bincount(best[m][had & (best[m] >= thr[m])] - thr[m], minlength=hi - thr[m] + 1).astype(np.uint64)
        assert np.array_equal(hists[m], want), m
        assert scored[m] == int(had.sum()) == n
        total += int(want.sum())
    assert total > 20 * n  # (the motifs at their lowest threshold bin every sequence)


# ---- 6. arguments ----------------------------------------------------------------------------------------------------------
def test_arguments_are_checked_and_empty_inputs_do_nothing(ctx, small):
    seqs, packed, scan = small
    S = [random_S(np.random.default_rng(1), 6)]
    wide = [np.concatenate([S[0]] * 11)[:64]]  # (64 rows, declared 65 wide)
    hi = me.score_hi(S[0])
    pre_h, pre_s = np.arange(51, dtype=np.uint64) + 7, np.array([99], np.uint64)

    def fresh():
        return dict(hist=ctx.to_device(pre_h), scored=ctx.to_device(pre_s))
    for kw, mats, args in [(dict(n_seq=2 ** 32), S, ([6], [hi - 50], [hi])),   # a private 32-bit bin could wrap
                           (dict(), S, ([6], [hi - 50], [hi - 1])),             # a score above h_hi would have no bin
                           (dict(), wide, ([65], [hi - 50], [hi]))]:            # width
        buf = fresh()
        with pytest.raises(pk.PengkError) as e:
            ctx.motif_enrich(scan, mats, args[0], True, args[1], args[2], **kw, **buf)
        assert e.value.code == pk.ERR_ARG and "pengk_motif_enrich" in str(e.value)
        assert np.array_equal(buf["hist"].to_host(), pre_h) and np.array_equal(buf["scored"].to_host(), pre_s)
    assert int(ctx.motif_enrich(scan, S, [6], True, [hi - 50], [hi])[1][0]) > 0  # (the same call, within the bounds)
    h, s = ctx.motif_enrich(scan, [], [], True, [], [])
    assert h == [] and len(s) == 0
    buf = fresh()
    h, s = ctx.motif_enrich(scan, S, [6], True, [hi - 50], [hi], n_seq=0, **buf)
    assert np.array_equal(h[0], pre_h) and int(s[0]) == 99


# ---- 7. the CLI ------------------------------------------------------------------------------------------------------------
FA = os.path.join(GOLD, "MafK.fasta")


@pytest.fixture(scope="module")
def database(tmp_path_factory):
    """the decoy-plus-word database of tests/test_motif_compare_cpu.py (motif_compare_model.planted_database)"""
    names, rows = mc.planted_database()
    path = tmp_path_factory.mktemp("enrich_db") / "planted.meme"
    mc.write_meme(path, names, rows)
    return str(path), names, rows


@pytest.fixture(scope="module")
def mafk_inputs():
    """MafK.fasta and the sampled negatives of --score-motifs (seed 1, order 2) as the model holds them, and bg0"""
    seqs = ms.read_fasta_codes(FA)
    codes, offs = ms.flatten(seqs)
    Vc = np.asarray(po.bg_V(po.bg_counts(codes, offs, 2), 2), np.float32)
    V = [Vc[0:4], Vc[4:20], Vc[20:84]]
    negs = [n + 1 for n in ms.sample([len(s) for s in seqs], 1, 0, 2, ms.thresholds(V, 2))]
    return me.Packed(seqs), me.Packed(negs), V[0]


@pytest.fixture(scope="module")
def mafk_model(database, mafk_inputs):
    """the model's results for the whole database at the defaults"""
    pos, neg, bg0 = mafk_inputs
    return me.analyse(pos, neg, database[2], bg0, 1e-3, True)


def assert_same_tsv(got, want):
    """strings and integers exactly; the floating-point columns to the tolerance of the CPU module plus a unit of the last
    printed digit (three decimals, or three significant digits)"""
    g, w = got.split("\n"), want.split("\n")
    assert g[0] == w[0] and len(g) == len(w), (len(g), len(w))
    assert g[-1] == w[-1] == ""
    for a, b in zip(g[1:-1], w[1:-1]):
        fa, fb = a.split("\t"), b.split("\t")
        assert len(fa) == len(fb) == 15, (a, b)
        assert fa[:10] == fb[:10], (a, b)  # (threshold_pvalue is the exact DP's, printed from the same double)
        for x, y in zip(fa[10:14], fb[10:14]):
            assert x == y or abs(float(x) - float(y)) <= 1e-9 * abs(float(y)) + 1e-9 + 1.001e-3, (a, b)
        # (10^lq: a difference of 1e-9 |lq| + 1e-9 in the logarithm is 1e-6 of the value at most, for |lq| < 400)
        assert fa[14] == fb[14] or abs(float(fa[14]) - float(fb[14])) <= (1e-6 + 1.001e-2) * float(fb[14]) + 1e-300, (a, b)


def test_cli_writes_the_models_table_and_changes_no_other_output(tmp_path, database, mafk_model):
    db, names, rows = database
    rc, so0, se, meme0, js0 = run_plain([FA, "-w", "10"], tmp_path, tag="a")
    assert rc == 0, se.decode()[-2000:]
    out = tmp_path / "e.tsv"
    rc, so1, se, meme1, js1 = run_plain([FA, "-w", "10", "--enrich", str(out), "--enrich-db", db], tmp_path, tag="b")
    assert rc == 0, se.decode()[-2000:]
    assert (so1, meme1, js1) == (so0, meme0, js0)
    got = out.read_text()
    assert_same_tsv(got, me.render(names, [""] * len(names), mafk_model))
    lines = [l.split("\t") for l in got.split("\n")[1:] if l]
    for l in lines[:3]:
        print("\t".join(l))
    assert lines[0][:4] == ["1", "MARE", ".", "13"] and float(lines[0][12]) < -20  # (rank 1: ahead of every decoy)
    # --enrich-evalue filters lines
    strict = tmp_path / "strict.tsv"
    rc, _, se, _, _ = run_plain([FA, "-w", "10", "--enrich", str(strict), "--enrich-db", db, "--enrich-evalue", "1e-5"], tmp_path,
                                tag="c")
    assert rc == 0, se.decode()[-2000:]
    want = me.render(names, [""] * len(names), mafk_model, E=1e-5)
    assert_same_tsv(strict.read_text(), want)
    assert 2 <= len(want.split("\n")) - 2 < len(lines)


def test_cli_pvalue_and_plus_strand_reach_the_device(tmp_path, mafk_inputs):
    """a small database with alternative names, --enrich-pvalue 1e-2, --strand PLUS: the model's file at those settings"""
    pos, neg, bg0 = mafk_inputs
    names, rows = mc.planted_database(n_decoys=4)
    alts = ["alt%d" % m if m % 2 else "" for m in range(len(names))]
    db = tmp_path / "small.meme"
    mc.write_meme(db, ["%s %s" % (n, a) if a else n for n, a in zip(names, alts)], rows)
    files = {}
    for tag, extra, both in [("plus", ["--strand", "PLUS"], False), ("both", [], True)]:
        out = tmp_path / (tag + ".tsv")
        rc, _, se, _, _ = run_plain([FA, "-w", "10", "--enrich", str(out), "--enrich-db", str(db), "--enrich-pvalue", "1e-2",
                                     "--enrich-evalue", "1e300"] + extra, tmp_path, tag=tag)
        assert rc == 0, se.decode()[-2000:]
        files[tag] = out.read_text()
        res = me.analyse(pos, neg, rows, bg0, 1e-2, both)
        assert_same_tsv(files[tag], me.render(names, alts, res, E=1e300))
        assert files[tag].count("\n") == 1 + len(names)  # (every motif at this E-value)
    assert files["plus"] != files["both"] and "\talt1\t" in files["plus"]


@pytest.mark.parametrize("world", [2, 3])
def test_cli_ranks_write_what_one_process_writes(tmp_path, database, world):
    db, _, _ = database
    one, many = tmp_path / "one.tsv", tmp_path / "many.tsv"
    rc, so, se, meme, js = run_plain([FA, "-w", "10", "--enrich", str(one), "--enrich-db", db], tmp_path)
    assert rc == 0, se.decode()[-2000:]
    res = run_ranks([FA, "-w", "10", "--enrich", str(many), "--enrich-db", db], world, tmp_path)
    for rank, (rrc, rso, rse, rmeme, rjs) in enumerate(res):
        assert rrc == 0, (rank, rse.decode()[-2000:])
    assert (res[0][1], res[0][3], res[0][4]) == (so, meme, js)
    assert many.read_bytes() == one.read_bytes() and one.read_text().count("\n") > 2


def test_cli_scores_against_the_negatives_of_score_motifs(tmp_path, database):
    """--score-motifs with and without --enrich: the same MEME and JSON (zoops_score and occur included), and the same
    enrichment file with and without --score-motifs -- one set of negatives, built once"""
    db, _, _ = database
    rc, so0, se, meme0, js0 = run_plain([FA, "-w", "10", "--score-motifs"], tmp_path, tag="s")
    assert rc == 0, se.decode()[-2000:]
    assert b"zoops_score" in js0
    both, alone = tmp_path / "both.tsv", tmp_path / "alone.tsv"
    rc, so1, se, meme1, js1 = run_plain([FA, "-w", "10", "--score-motifs", "--enrich", str(both), "--enrich-db", db], tmp_path, tag="se")
    assert rc == 0, se.decode()[-2000:]
    assert (so1, meme1, js1) == (so0, meme0, js0)
    rc, _, se, _, _ = run_plain([FA, "-w", "10", "--enrich", str(alone), "--enrich-db", db], tmp_path, tag="e")
    assert rc == 0, se.decode()[-2000:]
    assert both.read_bytes() == alone.read_bytes()
    # another seed: other negatives, another file
    seeded = tmp_path / "seed.tsv"
    rc, _, se, _, _ = run_plain([FA, "-w", "10", "--score-seed", "5", "--enrich", str(seeded), "--enrich-db", db], tmp_path, tag="e5")
    assert rc == 0, se.decode()[-2000:]
    assert seeded.read_bytes() != alone.read_bytes()
