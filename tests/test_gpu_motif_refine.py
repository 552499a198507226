"""Motif refinement on the device (--refine; include/pengk.h, "motif refinement") against the numpy model of
tests/motif_refine_model.py: the site profiles bit for bit (sites at both sequence ends, both strands, clamped flanks,
split records, a motif nearly every sequence holds), a planted motif regrown from its inner columns, and the CLI's file
against the model, beside the other outputs and over several ranks."""
import itertools
import json
import os

import numpy as np
import pytest

import peng_motif_amd as pk
import motif_centrality_model as mc
import motif_refine_model as mr
import motif_score_model as ms
import motif_sites_model as mst
from oracle import oracle as po
from test_gpu_multirank import run_plain, run_ranks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
WIDTHS = [4, 5, 7, 10, 13, 16, 21, 30]
FLANKS = [0, 1, 8, 40]  # (40: clamped for every width, to 17 at w = 30)


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
    """as tests/test_gpu_motif_centrality.py: lengths 0..400 (shorter than a motif, not multiples of 32), runs of N"""
    lens = [0, 1, 3, 4, 31, 32, 33, 64, 65, 200] + rng.integers(0, 300, 90).tolist()
    seqs = []
    for n in lens:
        c = rng.integers(1, 5, n).astype(np.uint8)
        for _ in range(int(rng.integers(0, 3))):  # N runs
            if n:
                a = int(rng.integers(0, n))
                c[a:a + int(rng.integers(1, 20))] = 0
        seqs.append(c)
    return seqs


def sub_scan(scan, i0, i1):
    """records [i0, i1) of a device scan layout (the words stay shared)"""
    return scan[0], scan[1], scan[2].ptr + 8 * i0, scan[3].ptr + 4 * i0, i1 - i0


def low_thresholds(gb):
    """thresholds that most sequences pass, so that sites at both sequence ends occur"""
    return [int(np.percentile(b[b > ms.SENTINEL], 30)) if np.any(b > ms.SENTINEL) else 0 for b in gb]


def model_counts(seqs, gb, gs, widths, thr, flank):
    return np.stack([mr.site_profile(seqs, gb[m], gs[m], widths[m], thr[m], flank) for m in range(len(widths))])


@pytest.mark.parametrize("both", [True, False], ids=["both", "plus"])
def test_counts_equal_the_model(ctx, both):
    rng = np.random.default_rng(131 + both)
    seqs = random_seqs(rng)
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    S = [random_S(rng, w) for w in WIDTHS]
    best, site = ctx.motif_best_sites(scan, S, WIDTHS, both)
    gb, gs = best.to_host(), site.to_host()
    # the best sites themselves are the model's (tests/test_gpu_motif_centrality.py checks every case of them)
    for m in range(len(S)):
        wb, ws = mc.best_sites(seqs, S[m], both, m)
        assert gb[m].tobytes() == wb.tobytes() and gs[m].tobytes() == ws.tobytes()
    thr = low_thresholds(gb)
    for flank in FLANKS:
        got = ctx.site_profiles(scan, best, site, WIDTHS, thr, flank).to_host()
        want = model_counts(seqs, gb, gs, WIDTHS, thr, flank)
        assert got.tobytes() == want.tobytes(), flank
        F = [pk.clamp_flank(w, flank) for w in WIDTHS]
        assert F == [mr.clamp_flank(w, flank) for w in WIDTHS] and all(w + 2 * f <= pk.MAX_MOTIF_LEN for w, f in zip(WIDTHS, F))
        for m, w in enumerate(WIDTHS):
            n = got[m, F[m]].sum()
            assert n > 20 and np.all(got[m, :w + 2 * F[m]].sum(axis=1) == n) and not got[m, w + 2 * F[m]:].any()
            assert not got[m, F[m]:F[m] + w, 4].any()  # (a site's own columns are bases)
        if flank >= 8:  # sites at both sequence ends: the first and the last flank column fall off some sequence
            assert got[:, 0, 4].sum() > 0 and sum(got[m, w + 2 * F[m] - 1, 4] for m, w in enumerate(WIDTHS)) > 0
        if both:
            assert np.count_nonzero(gs[:, :] & np.uint64(1)) > 50
    # a second call adds to the first
    c = ctx.site_profiles(scan, best, site, WIDTHS, thr, 8)
    ctx.site_profiles(scan, best, site, WIDTHS, thr, 8, counts=c)
    assert c.to_host().tobytes() == (2 * model_counts(seqs, gb, gs, WIDTHS, thr, 8)).tobytes()


def test_every_base_valid_without_validity_words(ctx):
    """d_valid = NULL (the sampled sequences' layout): a letter other than A/C/G/T is stored as A and counts as A"""
    rng = np.random.default_rng(141)
    seqs = random_seqs(rng)
    words, _, offs, lens, n = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    scan = (words, 0, offs, lens, n)
    as_a = [np.where(c == 0, 1, c).astype(np.uint8) for c in seqs]
    S = [random_S(rng, w) for w in WIDTHS]
    best, site = ctx.motif_best_sites(scan, S, WIDTHS, True)
    gb, gs = best.to_host(), site.to_host()
    thr = low_thresholds(gb)
    got = ctx.site_profiles(scan, best, site, WIDTHS, thr, 8).to_host()
    assert got.tobytes() == model_counts(as_a, gb, gs, WIDTHS, thr, 8).tobytes()
    assert got[..., 4].any()


def test_two_halves_add_up_to_one_call(ctx):
    rng = np.random.default_rng(151)
    seqs = random_seqs(rng)
    n = len(seqs)
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    S = [random_S(rng, w) for w in WIDTHS]
    best, site = ctx.motif_best_sites(scan, S, WIDTHS, True)
    thr = low_thresholds(best.to_host())
    whole = ctx.site_profiles(scan, best, site, WIDTHS, thr, 8).to_host()
    assert whole.any()
    for k in [1, 37, n // 2, n - 1]:
        c = None
        for i0, i1 in [(0, k), (k, n)]:
            part = sub_scan(scan, i0, i1)
            b, s = ctx.motif_best_sites(part, S, WIDTHS, True, seq0=i0)
            c = ctx.site_profiles(part, b, s, WIDTHS, thr, 8, counts=c)
        assert c.to_host().tobytes() == whole.tobytes(), k


def consensus_pwm(word, hit=0.97):
    pwm = np.full((len(word), 4), (1.0 - hit) / 3.0, np.float32)
    for j, ch in enumerate(word):
        pwm[j, "ACGT".index(ch)] = hit
    return pwm


def test_a_motif_nearly_every_sequence_holds(ctx):
    """> 90 % of the sequences select the same consensus: whole waves add to one (column, base) bin, the contended path"""
    rng = np.random.default_rng(161)
    n, L, word = 20000, 100, "TGCTGAGTCAGC"
    mot = np.array(["ACGT".index(c) + 1 for c in word], np.uint8)
    seqs = [rng.integers(1, 5, L).astype(np.uint8) for _ in range(n)]
    for i in np.nonzero(rng.random(n) < 0.96)[0]:
        p = int(rng.integers(0, L - len(word) + 1))
        if rng.random() < 0.5:
            seqs[i][p:p + len(word)] = mot
        else:
            seqs[i][p:p + len(word)] = 5 - mot[::-1]
    bg = np.full(4, 0.25, np.float32)
    S = [ms.log_odds(consensus_pwm(word), bg), random_S(rng, 9)]
    widths = [len(word), 9]
    thr = []
    for s in S:
        lo, tail = pk.score_tail_pvalues(s, bg)
        thr.append(pk.score_threshold(tail, lo, 1e-4))
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    best, site = ctx.motif_best_sites(scan, S, widths, True)
    gb, gs = best.to_host(), site.to_host()
    got = ctx.site_profiles(scan, best, site, widths, thr, 8).to_host()
    assert got.tobytes() == model_counts(seqs, gb, gs, widths, thr, 8).tobytes()
    assert got[0, 8].sum() > 0.9 * n
    for j, ch in enumerate(word):
        assert got[0, 8 + j, "ACGT".index(ch)] > 0.9 * n


# ---- a planted motif, regrown from its inner columns ---------------------------------------------------------------
PLANT_CONSENSUS = "TGCTGACTCAGCAATT"
PLANT_HIT = [0.7, 0.8, 0.9, 0.9, 0.95, 0.95, 0.95, 0.95, 0.95, 0.95, 0.95, 0.95, 0.9, 0.8, 0.7, 0.45]
B = 0.25


def planted_ic():
    """bits of every planted column against the uniform background"""
    out = []
    for h in PLANT_HIT:
        q = np.array([h] + [(1.0 - h) / 3.0] * 3)
        out.append(float((q * np.log2(q / 0.25)).sum()))
    return out


def planted_seqs(seed=7, n=2000, L=200, rate=0.5):
    """seed 7, every second sequence planted: the model below satisfies the test's assertions with them (checked on the
    CPU before the device was asked), with room: the weakest column asked for has 0.64 planted bits, diluted by the
    sites that are not planted ones it still stands far above B"""
    rng = np.random.default_rng(seed)
    seqs = [rng.integers(1, 5, L).astype(np.uint8) for _ in range(n)]
    for i in np.nonzero(rng.random(n) < rate)[0]:
        mot = np.empty(16, np.uint8)
        for j, (ch, h) in enumerate(zip(PLANT_CONSENSUS, PLANT_HIT)):
            b = "ACGT".index(ch)
            mot[j] = b + 1 if rng.random() < h else 1 + (b + 1 + int(rng.integers(0, 3))) % 4
        p = int(rng.integers(0, L - 15))
        seqs[i][p:p + 16] = mot if rng.random() < 0.5 else 5 - mot[::-1]
    return seqs


def device_refine(ctx, scan, pwms, bg, both, pvalue=1e-4, flank=8, iterations=3, min_ic=B):
    """the rounds of motif_refine_model.refine on the device calls"""
    mot = [{"pwm": np.asarray(p, np.float32), "w0": len(p), "sites": 0, "rounds": 0, "left": 0, "right": 0, "active": True,
            "prev": None} for p in pwms]
    for _ in range(iterations):
        if not any(r["active"] for r in mot):
            break
        S = [ms.log_odds(r["pwm"], bg) for r in mot]
        widths = [len(s) for s in S]
        thr = []
        for s, r in zip(S, mot):
            lo, tail = pk.score_tail_pvalues(s, bg)
            thr.append(pk.score_threshold(tail, lo, pvalue) if r["active"] else 2 ** 31 - 1)
        best, site = ctx.motif_best_sites(scan, S, widths, both)
        counts = ctx.site_profiles(scan, best, site, widths, thr, flank).to_host()
        for m, r in enumerate(mot):
            if not r["active"]:
                continue
            w = widths[m]
            got = pk.profile_refine(counts[m], w, flank, bg, min_ic)
            if got["sites"] == 0 or got["first"] == got["last"]:
                r["active"] = False
                continue
            F = pk.clamp_flank(w, flank)
            a, b = -r["left"] - F + got["first"], -r["left"] - F + got["last"]
            kept = counts[m, got["first"]:got["last"]].tobytes()
            if r["prev"] == (a, b, kept):
                r["active"] = False
            r["prev"] = (a, b, kept)
            r["pwm"], r["left"], r["right"] = got["pwm"], -a, b - r["w0"]
            r["rounds"] += 1
            r["sites"] = got["sites"]
    return mot


def assert_regrown(r):
    """started from the planted columns 4..11: wider on both sides, and every planted column of >= 2B bits kept with
    its consensus base"""
    assert r["left"] >= 1 and r["right"] >= 1 and len(r["pwm"]) == 8 + r["left"] + r["right"]
    strong = [j for j, ic in enumerate(planted_ic()) if ic >= 2 * B]
    assert strong == list(range(15))  # (all but the last, a 0.14-bit column)
    for j in strong:
        row = j - 4 + r["left"]  # planted column j in the refined matrix
        assert 0 <= row < len(r["pwm"]), (j, r["left"], r["right"])
        assert "ACGT"[int(np.argmax(r["pwm"][row]))] == PLANT_CONSENSUS[j], j
    assert r["sites"] > 500


def test_planted_motif_regrows_from_its_inner_columns(ctx):
    seqs = planted_seqs()
    bg = np.full(4, 0.25, np.float32)
    start = consensus_pwm(PLANT_CONSENSUS[4:12], 0.9)
    model = mr.refine(seqs, [start], bg, True, min_ic=B)
    assert_regrown(model[0])  # the model first, on the CPU
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    got = device_refine(ctx, scan, [start], bg, True)
    assert_regrown(got[0])
    for k in ("sites", "rounds", "left", "right"):
        assert got[0][k] == model[0][k], k
    assert got[0]["pwm"].tobytes() == model[0]["pwm"].tobytes()


# ---- the CLI -----------------------------------------------------------------------------------------------------------
def found_log_odds(pwm, bg, pvalue):
    """(S, ambiguous): the log-odds the run scanned with, from a PWM of the JSON.  The JSON holds the found PWM after the
    writers added eps = 1e-8 / (1 - 4e-8) to every cell and renormalised, twice (MEME, then JSON), rounded to 8 decimals:
    p' = (p + 2 eps) / (1 + 8 eps) up to a few float32 roundings and 5e-9.  Undone in double, the found entry is known to
    dp = 5e-9 + 3 * 2^-24 p', its log-odds to tol = 100 / ln 2 * dp / p units.  An entry so low that no window holding it
    reaches the threshold T (hi - its column's maximum + S + tol + 1 < T) changes neither T (the tail at and above T sums
    windows without it, in the same order) nor any site at or above T, whatever its value: the near-zero cells, which
    are the uncertain ones, are all of this kind.  Any other entry within tol of a rounding boundary is returned as
    ambiguous: (index, its possible values, the likeliest first)."""
    eps = 1e-8 / (1.0 - 4e-8)
    pj = np.asarray(pwm, np.float64)
    p = np.maximum(pj * (1.0 + 8.0 * eps) - 2.0 * eps, 1e-300)
    g = np.asarray(bg, np.float32).astype(np.float64)
    v = np.clip(100.0 * np.log2(p / g), -2000.0, 2000.0)
    S = (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int32)
    tol = 100.0 / np.log(2.0) * (5e-9 + 3.0 * 2.0 ** -24 * pj) / p + 1e-9
    lo, tail = mst.tail_pvalues(S, bg)
    T = mst.threshold(lo, tail, pvalue)
    hi = int(S.max(axis=1).sum())
    matters = hi - S.max(axis=1, keepdims=True) + S + np.minimum(tol, 4000.0) + 1 >= T
    near = np.abs(np.abs(v) - np.floor(np.abs(v)) - 0.5) < tol
    amb = []
    for j, a in zip(*np.nonzero(near & matters)):
        rd = lambda x: int(np.sign(x) * np.floor(abs(x) + 0.5))
        vals = sorted({rd(x) for x in np.linspace(v[j, a] - tol[j, a], v[j, a] + tol[j, a], 9)} - {int(S[j, a])})
        amb.append(((int(j), int(a)), [int(S[j, a])] + [x for x in vals if abs(x) <= 2000]))
    return S, amb


def motif_blocks(text):
    head, _, rest = text.partition("MOTIF ")
    return head, ["MOTIF " + b for b in rest.split("MOTIF ")] if rest else []


def assert_refined_file_equals_model(fa, js, text, both, pvalue=1e-4, flank=8, iterations=3, min_ic=B):
    """byte for byte: the header, and every motif's block against the model run from the log-odds the run scanned with
    (found_log_odds; where an entry of them is ambiguous, against the model of one of its possible values -- at most
    64 models per motif, more fails the test).  From the first counts on the run and the model hold the same integers."""
    seqs = ms.read_fasta_codes(fa)
    codes, offs = ms.flatten(seqs)
    bg = np.asarray(po.bg_V(po.bg_counts(codes, offs, 2), 2), np.float32)[0:4]
    pats = json.loads(js)["patterns"]
    head, blocks = motif_blocks(text)
    assert head == motif_blocks(mr.render([], [], bg))[0]
    assert len(blocks) == len(pats)
    out = []
    for m, p in enumerate(pats):
        S, amb = found_log_odds(p["pwm"], bg, pvalue)
        assert np.prod([len(vals) for _, vals in amb]) <= 64, (m, amb)
        want = []
        for pick in itertools.product(*[vals for _, vals in amb]):
            S1 = S.copy()
            for (idx, _), val in zip(amb, pick):
                S1[idx] = val
            # (the motif's index seeds the tie-break: the model runs it as motif m)
            r = mr.refine(seqs, [None] * m + [np.array(p["pwm"], np.float32)], bg, both, pvalue, flank, iterations, min_ic,
                          S0=[None] * m + [S1], only=m)[m]
            want.append(motif_blocks(mr.render([p["iupac_motif"]], [r], bg))[1][0])
            if r["rounds"] == 0:  # the found PWM itself, which the JSON holds only to 8 decimals and after the writers' eps
                gl, wl = blocks[m].splitlines(), want[-1].splitlines()
                assert gl[:2] == wl[:2] and len(gl) == len(wl)
                a = np.array([l.split() for l in gl[2:] if l], np.float64)
                b = np.array([l.split() for l in wl[2:] if l], np.float64)
                assert np.abs(a - b).max() <= 5e-8
                want[-1] = blocks[m]
        assert blocks[m] in want, (m, blocks[m], want[0])
        out.append(blocks[m])
    return out


def matrix_line(block):
    f = block.splitlines()[1].split()
    return {f[i].rstrip("="): int(f[i + 1]) for i in range(2, len(f), 2)}


def test_cli_refine_equals_the_model_and_leaves_everything_else_alone(tmp_path):
    fa = os.path.join(GOLD, "MafK.fasta")
    ref = tmp_path / "refined.meme"
    rc, so, se, meme, js = run_plain([fa, "-w", "10", "--refine", str(ref)], tmp_path, tag="ref")
    assert rc == 0, se.decode()[-2000:]
    for ext, got in [("stdout", so), ("meme", meme), ("json", js)]:
        with open(os.path.join(GOLD, "cli", "cli_mafk_w10." + ext), "rb") as fh:
            assert got == fh.read(), ext
    blocks = assert_refined_file_equals_model(fa, js, ref.read_text(), True)
    # the first motif, CTGASTCAGCAAW, gains the G of TGCTGAsTCAGCA on its left
    assert blocks[0].startswith("MOTIF CTGASTCAGCAAW\n")
    first = matrix_line(blocks[0])
    assert first["left"] >= 1 and first["w"] == 13 + first["left"] + first["right"] and first["iterations"] >= 1
    rows = np.array([l.split() for l in blocks[0].splitlines()[2:] if l], np.float64)
    assert len(rows) == first["w"]
    assert "ACGT"[int(np.argmax(rows[first["left"] - 1]))] == "G"
    # other settings reach the run
    ref2 = tmp_path / "refined2.meme"
    args = ["--refine-pvalue", "1e-5", "--refine-flank", "3", "--refine-iterations", "1", "--refine-min-ic", "0.5"]
    rc, so2, se, meme2, js2 = run_plain([fa, "-w", "10", "--refine", str(ref2)] + args, tmp_path, tag="ref2")
    assert rc == 0, se.decode()[-2000:]
    assert (so2, meme2, js2) == (so, meme, js)
    for b in assert_refined_file_equals_model(fa, js2, ref2.read_text(), True, 1e-5, 3, 1, 0.5):
        assert matrix_line(b)["iterations"] <= 1 and matrix_line(b)["left"] <= 3 and matrix_line(b)["right"] <= 3


def test_cli_refine_beside_sites_and_centrality(tmp_path):
    fa = os.path.join(GOLD, "MafK.fasta")
    s0, c0, s1, c1, ref = (tmp_path / n for n in ["s0.tsv", "c0.tsv", "s1.tsv", "c1.tsv", "r.meme"])
    rc, so0, se, meme0, js0 = run_plain([fa, "-w", "10", "--sites", str(s0), "--centrality", str(c0)], tmp_path, tag="a")
    assert rc == 0, se.decode()[-2000:]
    rc, so1, se, meme1, js1 = run_plain([fa, "-w", "10", "--sites", str(s1), "--centrality", str(c1), "--refine", str(ref)],
                                        tmp_path, tag="b")
    assert rc == 0, se.decode()[-2000:]
    assert (so1, meme1, js1) == (so0, meme0, js0)
    assert s1.read_bytes() == s0.read_bytes() and c1.read_bytes() == c0.read_bytes()
    alone = tmp_path / "alone.meme"
    rc, _, se, _, _ = run_plain([fa, "-w", "10", "--refine", str(alone)], tmp_path, tag="c")
    assert rc == 0, se.decode()[-2000:]
    assert ref.read_bytes() == alone.read_bytes() and ref.read_bytes().count(b"MOTIF ") == len(json.loads(js0)["patterns"])


def test_cli_refine_plus_strand(tmp_path):
    fa = os.path.join(GOLD, "MafK.fasta")
    ref = tmp_path / "plus.meme"
    rc, _, se, _, js = run_plain([fa, "-w", "10", "--strand", "PLUS", "--refine", str(ref)], tmp_path)
    assert rc == 0, se.decode()[-2000:]
    assert_refined_file_equals_model(fa, js, ref.read_text(), False)


@pytest.mark.parametrize("world", [2, 3])
def test_cli_ranks_write_what_one_process_writes(tmp_path, world):
    fa = os.path.join(GOLD, "MafK.fasta")
    one = tmp_path / "one.meme"
    rc, so, se, meme, js = run_plain([fa, "-w", "10", "--refine", str(one)], tmp_path)
    assert rc == 0, se.decode()[-2000:]
    many = tmp_path / "many.meme"
    res = run_ranks([fa, "-w", "10", "--refine", str(many)], world, tmp_path)
    for rank, (rrc, rso, rse, rmeme, rjs) in enumerate(res):
        assert rrc == 0, (rank, rse.decode()[-2000:])
        if rank == 0:
            assert rmeme == meme and rjs == js and rso == so
    assert many.read_bytes() == one.read_bytes()
