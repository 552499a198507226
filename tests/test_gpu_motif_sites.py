"""Motif sites on the device (--sites; include/pengk.h, "motif sites") against the numpy model of
tests/motif_sites_model.py: the exact set of window strands at or above each motif's threshold, in the file's order, for
any record budget; recall of a planted motif; the CLI's TSV against the model and against its own multi-rank runs."""
import json
import os

import numpy as np
import pytest

import peng_motif_amd as pk
import motif_score_model as ms
import motif_sites_model as mst
from oracle import oracle as po
from test_gpu_multirank import run_plain, run_ranks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


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


def random_seqs(rng):
    lens = [0, 1, 31, 32, 33, 64, 65, 200] + rng.integers(0, 400, 60).tolist()
    seqs = []
    for n in lens:
        c = rng.integers(1, 5, n).astype(np.uint8)
        for _ in range(int(rng.integers(0, 3))):  # N runs
            if n:
                a = int(rng.integers(0, n))
                c[a:a + int(rng.integers(1, 20))] = 0
        seqs.append(c)
    return seqs


def thresholds(Ss, bg, P):
    out = []
    for S in Ss:
        lo, tail = mst.tail_pvalues(S, bg)
        out.append(mst.threshold(lo, tail, P))
    return out


WIDTHS = [1, 2, 3, 4, 5, 8, 10, 13, 16, 21, 31, 33, 48, 64, 7, 12]


@pytest.mark.parametrize("both", [True, False], ids=["both", "plus"])
def test_sites_equal_the_model(ctx, both):
    rng = np.random.default_rng(11 + both)
    seqs = random_seqs(rng)
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    bg = rng.dirichlet(np.ones(4) * 4).astype(np.float32)
    S = [random_S(rng, w) for w in WIDTHS]
    thr = thresholds(S, bg, 0.05)
    thr[3] = 10 ** 6  # (a motif without any site)
    got, tot = ctx.motif_sites(scan, S, WIDTHS, both, thr)
    want = mst.all_sites(seqs, S, thr, both)
    assert len(want) > 1000
    assert got.tobytes() == want.tobytes()
    assert [int(x) for x in tot] == [int((want["motif"] == m).sum()) for m in range(len(WIDTHS))]


def test_record_budget_slices_give_the_same_records():
    c = pk.Context(0)
    try:
        rng = np.random.default_rng(21)
        seqs = random_seqs(rng)
        scan = c.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
        bg = np.full(4, 0.25, np.float32)
        S = [random_S(rng, w) for w in WIDTHS]
        thr = thresholds(S, bg, 0.02)
        whole, _ = c.motif_sites(scan, S, WIDTHS, True, thr)
        again, _ = c.motif_sites(scan, S, WIDTHS, True, thr)
        assert whole.tobytes() == again.tobytes()
        for budget in [1, 3, 50]:
            pk._check(pk.lib().pengk_set_option(c.h, b"sites_record_budget", budget))
            counts = c.sites_count(scan, S, WIDTHS, True, thr)
            bounds, recs, _ = c.sites_slices(counts, scan[4], len(WIDTHS))
            assert len(recs) > 10 and int(bounds[0]) == 0 and int(bounds[-1]) == scan[4]
            assert all(r <= budget or b1 - b0 == 1 for r, b0, b1 in zip(recs, bounds[:-1], bounds[1:]))
            got, _ = c.motif_sites(scan, S, WIDTHS, True, thr)
            assert got.tobytes() == whole.tobytes(), budget
    finally:
        c.close()


def planted_pwm():
    pwm = np.full((10, 4), 0.01, np.float32)
    for j, ch in enumerate("GCTGAGTCAT"):
        pwm[j, "ACGT".index(ch)] = 0.97
    return pwm


def test_planted_sites_are_all_found_and_a_random_motif_hits_at_its_rate(ctx):
    n, L, seed = 200000, 200, 7
    scan = ctx.synth_scan(seed, 0, n, L)
    bg = np.full(4, 0.25, np.float32)
    rng = np.random.default_rng(4)
    S = [ms.log_odds(planted_pwm(), bg), ms.log_odds(rng.dirichlet(np.ones(4), 10).astype(np.float32), bg)]
    P = 1e-4
    lo1, tail1 = mst.tail_pvalues(S[1], bg)
    thr = thresholds(S, bg, P)
    got, tot = ctx.motif_sites(scan, S, [10, 10], True, thr)
    assert [int(x) for x in tot] == [int((got["motif"] == m).sum()) for m in range(2)]
    # the planted occurrences of pengk_synth_scan_sequences (count.hip's synthetic input)
    idx = np.arange(n, dtype=np.uint64) + np.uint64(1)
    planted = (ms.mix64(np.uint64(seed) ^ np.uint64(0xA5A5A5A5) ^ idx) % np.uint64(10)) == 0
    q = ms.mix64(np.uint64(seed) ^ np.uint64(0x5A5A5A5A) ^ idx) % np.uint64(L - 9)
    g0 = got[(got["motif"] == 0) & (got["strand"] == 0)]
    found = set(zip(g0["seq"].tolist(), g0["pos"].tolist()))
    want = set(zip(np.nonzero(planted)[0].tolist(), q[planted].tolist()))
    assert len(want) > 15000 and want <= found
    # a random PWM: every window strand is a site with probability P(score >= t)
    e = n * (L - 9) * 2 * tail1[thr[1] - lo1]
    k = int((got["motif"] == 1).sum())
    assert abs(k - e) <= 6 * np.sqrt(e) + 0.01 * e, (k, e)


def test_configs2_size_sixteen_motifs(ctx):
    n, L = 10_000_000, 200
    scan = ctx.synth_scan(1, 0, n, L)
    rng = np.random.default_rng(16)
    widths = [10, 11, 12, 13, 14] * 3 + [12]
    bg = np.full(4, 0.25, np.float32)
    S = [random_S(rng, w) for w in widths]
    thr = thresholds(S, bg, 1e-4)
    counts = ctx.sites_count(scan, S, widths, True, thr)
    bounds, recs, tot = ctx.sites_slices(counts, n, len(widths))
    assert int(recs.sum()) == int(tot.sum()) > 16 * 10 ** 5
    cap = int(recs.max())
    buf = ctx.empty(cap * pk.SITE.itemsize, np.uint8)
    per_motif = np.zeros(len(widths), np.int64)
    for k in range(len(recs)):
        ctx.sites_emit(scan, S, widths, True, thr, counts, int(bounds[k]), int(bounds[k + 1]), buf, cap)
        r = buf.to_host()[:int(recs[k]) * pk.SITE.itemsize].view(pk.SITE)
        per_motif += np.bincount(r["motif_strand"] >> 1, minlength=len(widths))
        assert np.all(r["seq"] < bounds[k + 1] - bounds[k]) and np.all(r["pos"] <= L - 10)
    assert per_motif.tolist() == [int(x) for x in tot]


def assert_cli_equals_model(fa, js, text, P, both):
    """the CLI's TSV against the model built from the JSON's PWMs and the input's order-0 background (the CLI's default:
    the input is the background set), motif by motif.  The JSON holds each PWM after the writers' pseudo count and row
    renormalisation, rounded to 8 decimals, so a log-odds entry of it can round one unit away from the PWM the run
    scanned with: a line may then differ in its score (by at most one unit per column, its p-value with it), and a window
    that close to the threshold may be in one set only.  Everything else is equal, line for line."""
    seqs = ms.read_fasta_codes(fa)
    codes, offs = ms.flatten(seqs)
    bg = np.asarray(po.bg_V(po.bg_counts(codes, offs, 2), 2), np.float32)[0:4]
    names = mst.read_fasta_names(fa)
    pats = json.loads(js)["patterns"]
    lines = text.splitlines(True)
    assert lines[0] == mst.HEADER
    by_motif = {}
    for l in lines[1:]:
        by_motif.setdefault(int(l.split("\t", 1)[0]), []).append(l)
    assert set(by_motif) <= set(range(1, len(pats) + 1))
    same = total = 0
    for m, p in enumerate(pats):
        S = ms.log_odds(np.array(p["pwm"], np.float32), bg)
        w = len(S)
        lo, tail = mst.tail_pvalues(S, bg)
        t = mst.threshold(lo, tail, P)
        want = mst.render(seqs, names, [p["iupac_motif"]], [S], bg, P, both, header=False, first_index=m + 1).splitlines()
        got = [l.rstrip("\n") for l in by_motif.get(m + 1, [])]
        # (records may share a name: a line's key is its name, start, strand and bases, and which of its kind it is)
        def keyed(ls):
            seen, out = {}, []
            for l in ls:
                f = l.split("\t")
                k0 = (f[2], int(f[3]), f[5], f[8])
                seen[k0] = seen.get(k0, 0) + 1
                out.append((k0 + (seen[k0],), f))
            return out
        Gl, Wl = keyed(got), keyed(want)
        G, W = dict(Gl), dict(Wl)
        for k in set(G) | set(W):
            g, v = G.get(k), W.get(k)
            if g is not None and v is not None:
                assert g[:6] == v[:6] and g[8] == v[8], (g, v)
                assert abs(round(float(g[6]) * 100) - round(float(v[6]) * 100)) <= w, (g, v)
            else:
                x = v if v is not None else g
                assert abs(round(float(x[6]) * 100) - t) <= w, (m, x, t)
        # the order: the model's order of the keys both share
        assert [k for k, _ in Gl if k in W] == [k for k, _ in Wl if k in G]
        same += len(set(got) & set(want))
        total += max(len(got), len(want))
    assert total > 100 and same >= 0.75 * total, (same, total)  # (one entry off by a unit shifts every line that uses it)


def test_cli_sites_equal_the_model_and_leave_everything_else_alone(tmp_path):
    fa = os.path.join(GOLD, "MafK.fasta")
    rc, so0, se, meme0, js0 = run_plain([fa, "-w", "10"], tmp_path, tag="plain")
    assert rc == 0, se.decode()[-2000:]
    tsv = tmp_path / "sites.tsv"
    rc, so1, se, meme1, js1 = run_plain([fa, "-w", "10", "--sites", str(tsv)], tmp_path, tag="sites")
    assert rc == 0, se.decode()[-2000:]
    assert (so1, meme1, js1) == (so0, meme0, js0)
    text = tsv.read_text()
    assert len(json.loads(js0)["patterns"]) > 0 and text.count("\n") > 100
    assert_cli_equals_model(fa, js1, text, 1e-4, True)
    # beside --score-motifs: its outputs unchanged, the sites in its order
    rc, so2, se, meme2, js2 = run_plain([fa, "-w", "10", "--score-motifs"], tmp_path, tag="scored")
    assert rc == 0, se.decode()[-2000:]
    tsv3 = tmp_path / "sites3.tsv"
    rc, so3, se, meme3, js3 = run_plain([fa, "-w", "10", "--score-motifs", "--sites", str(tsv3), "--sites-pvalue", "1e-3"],
                                        tmp_path, tag="scored_sites")
    assert rc == 0, se.decode()[-2000:]
    assert (so3, meme3, js3) == (so2, meme2, js2)
    assert_cli_equals_model(fa, js3, tsv3.read_text(), 1e-3, True)


def test_cli_plus_strand_has_no_minus_lines(tmp_path):
    fa = os.path.join(GOLD, "MafK.fasta")
    tsv = tmp_path / "plus.tsv"
    rc, _, se, _, js = run_plain([fa, "-w", "8", "--strand", "PLUS", "--sites", str(tsv), "--sites-pvalue", "1e-3"], tmp_path)
    assert rc == 0, se.decode()[-2000:]
    lines = tsv.read_text().splitlines()
    assert len(lines) > 1 and all(l.split("\t")[5] == "+" for l in lines[1:])
    assert_cli_equals_model(fa, js, tsv.read_text(), 1e-3, False)


@pytest.mark.parametrize("world", [2, 3])
def test_cli_ranks_write_what_one_process_writes(tmp_path, world):
    fa = os.path.join(GOLD, "MafK.fasta")
    one = tmp_path / "one.tsv"
    rc, so, se, meme, js = run_plain([fa, "-w", "10", "--sites", str(one), "--sites-pvalue", "1e-3"], tmp_path)
    assert rc == 0, se.decode()[-2000:]
    many = tmp_path / "many.tsv"
    res = run_ranks([fa, "-w", "10", "--sites", str(many), "--sites-pvalue", "1e-3"], world, tmp_path)
    for rank, (rrc, rso, rse, rmeme, rjs) in enumerate(res):
        assert rrc == 0, (rank, rse.decode()[-2000:])
        if rank == 0:
            assert rmeme == meme and rjs == js and rso == so
    assert many.read_bytes() == one.read_bytes()
