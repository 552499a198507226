"""The dinucleotide-preserving shuffle on the device (include/pengk.h, pengk_shuffle_sequences) against
the model of tests/motif_shuffle_model.py, whole output words and validity words bit for bit; its invariants and its
shard invariance from the device output alone at a size of more than one pass of the grid (the scale comparison of this
kernel: tests/test_gpu_scan_scale.py holds those of the older scan kernels); the CLI's --score-negatives shuffled
against the model, against itself and against its own multi-rank runs."""
import json
import os

import numpy as np
import pytest

import peng_motif_amd as pk
import motif_score_model as ms
import motif_shuffle_model as sm
from oracle import oracle as po
from test_gpu_multirank import run_plain, run_ranks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SEEDS = [(1, 0), (77, 12345), (2 ** 63 + 5, 3)]


@pytest.fixture(scope="module")
def ctx():
    c = pk.Context(0)
    yield c
    c.close()


def upload(ctx, seqs):
    words, valid, offs, lens = sm.pack(seqs)
    return (ctx.to_device(words), ctx.to_device(valid), ctx.to_device(offs), ctx.to_device(lens), len(seqs)), (words, valid, offs, lens)


def zeros_like(ctx, a):
    return ctx.to_device(np.zeros_like(a))


def device_equals_model(ctx, seqs, seed, seq0):
    scan, (words, valid, offs, lens) = upload(ctx, seqs)
    got_w, got_v = ctx.shuffle_sequences(scan, seed, seq0, words=zeros_like(ctx, words), valid=zeros_like(ctx, valid))
    want_w, want_v = sm.shuffle_layout(words, valid, offs, lens, len(seqs), seed, seq0)
    gw, gv = got_w.to_host(), got_v.to_host()
    assert np.array_equal(gw, want_w), np.flatnonzero(gw != want_w)[:8]
    assert np.array_equal(gv, want_v), np.flatnonzero(gv != want_v)[:8]


def constructed():
    rng = np.random.default_rng(11)
    return [
        [2] * 50,                                        # a homopolymer
        [0] * 199 + [1],                                 # A^(L-1) C: the longest tree walks
        [0, 1] * 20, [0, 1] * 20 + [0],                  # ACAC.. of even and odd length
        [4] * 37,                                        # no valid base at all
        [0, 1] * 10 + [3] + [1, 0] * 10,                 # a letter that occurs once, in the middle
        [0, 1, 0, 0, 1, 1] * 5 + [2],                    # ... and one that occurs only at the end
        rng.choice([1, 3], 70).tolist(), rng.choice([0, 4], 45).tolist(), rng.choice([2, 3], 33).tolist(),  # two letters
        rng.integers(0, 3, 60).tolist() + [3],           # the last letter occurs nowhere else
        rng.integers(0, 3, 64).tolist() + [4],           # ... and is not a base
        [3], [4], [1, 4], [4, 4, 0],
    ]


@pytest.mark.parametrize("seed,seq0", SEEDS)
def test_device_equals_the_model(ctx, seed, seq0):
    rng = np.random.default_rng(seq0 + 1)
    lens = [0, 1, 2, 3, 31, 32, 33, 64, 65, 200] + rng.integers(0, 300, 40).tolist()
    seqs = [rng.integers(0, 5, n).tolist() for n in lens]
    device_equals_model(ctx, seqs, seed, seq0)


@pytest.mark.parametrize("seed,seq0", SEEDS)
def test_device_equals_the_model_on_constructed_sequences(ctx, seed, seq0):
    device_equals_model(ctx, constructed(), seed, seq0)


@pytest.mark.parametrize("seed,seq0", SEEDS)
@pytest.mark.parametrize("out_valid", [False, True], ids=["no_out_valid", "out_valid"])
def test_without_validity_words_every_base_is_valid(ctx, seed, seq0, out_valid):
    rng = np.random.default_rng(seq0 + 2)
    lens = [0, 1, 2, 3, 31, 32, 33, 64, 65, 200] + rng.integers(0, 300, 40).tolist()
    seqs = [rng.integers(0, 4, n).tolist() for n in lens] + [[2] * 50, [0] * 199 + [1], [0, 1] * 20, [1, 3] * 16 + [1]]
    scan, (words, valid, offs, lens) = upload(ctx, seqs)
    # (the input's validity words are not read: poison them)
    scan = (scan[0], ctx.to_device(np.zeros_like(valid)), scan[2], scan[3], scan[4])
    got_w, got_v = ctx.shuffle_sequences(scan, seed, seq0, all_valid=True, words=zeros_like(ctx, words),
                                         valid=zeros_like(ctx, valid) if out_valid else None)
    want_w, want_v = sm.shuffle_layout(words, None, offs, lens, len(seqs), seed, seq0)
    assert np.array_equal(got_w.to_host(), want_w)
    if out_valid:
        assert np.array_equal(got_v.to_host(), want_v) and np.array_equal(want_v, valid)  # ones inside, zero padding
    else:
        assert got_v is None


def test_argument_errors(ctx):
    scan, (words, valid, offs, lens) = upload(ctx, [[0, 1, 2, 3] * 10, [1, 1, 4]])
    ow, ov = zeros_like(ctx, words), zeros_like(ctx, valid)
    L, P = pk.lib(), pk._ptr
    call = lambda *a: L.pengk_shuffle_sequences(ctx.h, *a)
    assert call(1, 0, 2, P(scan[0]), P(scan[1]), P(scan[2]), P(scan[3]), P(scan[0]), P(ov)) == pk.ERR_ARG  # in place
    assert call(1, 0, 2, P(scan[0]), P(scan[1]), P(scan[2]), P(scan[3]), P(ow), P(scan[1])) == pk.ERR_ARG
    assert call(1, 0, 2, P(scan[0]), P(scan[1]), P(scan[2]), P(scan[3]), P(ow), None) == pk.ERR_ARG  # the negatives need their bits
    assert call(1, 0, 2, None, P(scan[1]), P(scan[2]), P(scan[3]), P(ow), P(ov)) == pk.ERR_ARG
    assert call(1, 2 ** 32 - 1, 2, P(scan[0]), P(scan[1]), P(scan[2]), P(scan[3]), P(ow), P(ov)) == pk.ERR_ARG
    assert call(1, 2 ** 32 - 2, 2, P(scan[0]), P(scan[1]), P(scan[2]), P(scan[3]), P(ow), P(ov)) == pk.PENGK_OK
    assert call(1, 0, 0, None, None, None, None, None, None) == pk.PENGK_OK  # nothing to do
    ctx.synchronize()


def letters_2d(words, n, L):
    """(n, L) letters of n all-valid sequences of equal length L in the scan layout"""
    w = words[:n * ((L + 31) // 32)].reshape(n, -1)
    p = np.arange(L)
    return ((w[:, p >> 5] >> (2 * (p & 31)).astype(np.uint64)) & np.uint64(3)).astype(np.uint8)


def doublets_2d(a):
    n = a.shape[0]
    d = (np.arange(n)[:, None] * 25 + 5 * a[:, :-1].astype(np.int64) + a[:, 1:]).reshape(-1)
    return np.bincount(d, minlength=25 * n).reshape(n, 25)


@pytest.mark.parametrize("n", [200_000, 400_000])
def test_invariants_and_shards_beyond_one_pass_of_the_grid(ctx, n):
    """n sequences of 40 bp, from the device output alone.  The kernel's grid is capped at 6 workgroups of 256 threads
    per CU (1536 workgroups, 393 216 threads on 256 CUs): at 400 000 the threads of the first workgroups take a second
    sequence."""
    L, seed = 40, 9
    scan = ctx.synth_scan(3, 0, n, L)
    win = scan[0].to_host()
    got_w, got_v = ctx.shuffle_sequences(scan, seed, 0)
    gw, gv = got_w.to_host(), got_v.to_host()
    assert np.array_equal(gv, scan[1].to_host())  # (every base valid, nothing beyond the ends)
    a, o = letters_2d(win, n, L), letters_2d(gw, n, L)
    assert not (gw.reshape(n, -1)[:, 1] >> np.uint64(2 * (L - 32))).any()
    assert np.array_equal(o[:, 0], a[:, 0]) and np.array_equal(o[:, -1], a[:, -1])
    assert np.array_equal(doublets_2d(o), doublets_2d(a))
    assert (o != a).any(axis=1).mean() > 0.99
    # the shuffle of [a, b) called with seq0 = a: a cut inside a workgroup's 256 sequences, and one at its boundary
    wps = (L + 31) // 32
    for lo, hi in ((12345, 12345 + 3001), (256 * 300, 256 * 300 + 5000), (n - 777, n)):
        sub = ctx.synth_scan(3, lo, hi - lo, L)
        sw, sv = ctx.shuffle_sequences(sub, seed, lo)
        assert np.array_equal(sw.to_host(), gw[lo * wps:hi * wps]), (lo, hi)
        assert np.array_equal(sv.to_host(), gv[lo * wps:hi * wps]), (lo, hi)
    rng = np.random.default_rng(n)
    for i in np.concatenate([[0, n - 1], rng.integers(0, n, 498)]).tolist():
        assert sm.shuffle(a[i].tolist(), seed, i) == o[i].tolist(), i


def test_one_long_skewed_sequence(ctx):
    """200 000 bases, 90 % A with a few runs of other letters: one doublet counter far above 65 535"""
    rng = np.random.default_rng(8)
    s = rng.choice(5, 200_000, p=[0.9, 0.04, 0.03, 0.03, 0.0])
    for at, k in ((1000, 17), (77_777, 300), (199_000, 1)):
        s[at:at + k] = 4
    assert sm.doublets(s)[0, 0] > 150_000
    seqs = [rng.integers(0, 5, 30).tolist(), s.tolist(), rng.integers(0, 5, 65).tolist(), [1, 2]]
    device_equals_model(ctx, seqs, 21, 1000)


# ---- the CLI: --score-motifs --score-negatives sampled|shuffled ----------------------------------------------------------
FA = os.path.join(GOLD, "MafK.fasta")


@pytest.fixture(scope="module")
def cli_runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("shuffle_cli")
    runs = {}
    for tag, extra in (("plain", []), ("scored", ["--score-motifs"]), ("sampled", ["--score-motifs", "--score-negatives", "sampled"]),
                       ("shuffled", ["--score-motifs", "--score-negatives", "shuffled"]),
                       ("again", ["--score-negatives", "shuffled", "--score-motifs"]), ("alone", ["--score-negatives", "shuffled"])):
        runs[tag] = run_plain([FA, "-w", "10"] + extra, tmp, tag=tag)
        assert runs[tag][0] == 0, (tag, runs[tag][2].decode()[-2000:])
    return runs


def test_cli_sampled_is_the_path_without_the_flag(cli_runs):
    pick = lambda r: (r[1], r[3], r[4])  # stdout, MEME, JSON
    assert pick(cli_runs["sampled"]) == pick(cli_runs["scored"])
    # without --score-motifs the flag does nothing, as --sites-qvalue without --sites
    assert pick(cli_runs["alone"]) == pick(cli_runs["plain"]) and b"shuffles" not in cli_runs["alone"][2]


def test_cli_shuffled_runs_repeat_and_say_so(cli_runs):
    a, b = cli_runs["shuffled"], cli_runs["again"]
    assert a[3] == b[3] and a[4] == b[4] and a[1] == b[1]
    assert a[2].count(b"dinucleotide-preserving shuffles") == 1 and b"shuffles" not in cli_runs["scored"][2]
    assert a[4] != cli_runs["scored"][4]


def test_cli_shuffled_scores_equal_the_model_and_nothing_else_moves(cli_runs):
    a, b = json.loads(cli_runs["plain"][4]), json.loads(cli_runs["shuffled"][4])
    assert a["bg"] == b["bg"] and len(a["patterns"]) == len(b["patterns"]) > 0
    # (the rules of test_gpu_motif_score.py: log(Pval) and bg_prob are printed with the stream's state at their place,
    # so a motif that moves compares as numbers there)
    key = lambda p: (p["iupac_motif"], p["sites"], p["pattern_length"])
    plain = {key(p): p for p in a["patterns"]}
    assert sorted(plain) == sorted(key(p) for p in b["patterns"])
    for p in b["patterns"]:
        q = dict(p)
        assert list(q)[6:8] == ["zoops_score", "occur"]
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
    lines = [l for l in cli_runs["shuffled"][3].decode().splitlines() if l.startswith("letter-probability matrix:")]
    assert len(lines) == len(b["patterns"])
    for l, p in zip(lines, b["patterns"]):
        f = l.split()
        assert f[-6] == "log(Pval)=" and f[-4] == "zoops_score=" and f[-2] == "occur="
        assert abs(float(f[-3]) - p["zoops_score"]) < 1e-6 and abs(float(f[-1]) - p["occur"]) < 1e-6
    # the model: the written PWMs against the input's order-0 frequencies, the negatives the model's shuffles at the
    # default --score-seed 1 and g = the sequence's index
    seqs = ms.read_fasta_codes(FA)
    codes, offs = ms.flatten(seqs)
    V0 = np.asarray(po.bg_V(po.bg_counts(codes, offs, 2), 2), np.float32)[0:4]
    negs = []
    for i, c in enumerate(seqs):
        o = np.array(sm.shuffle(np.where(c >= 1, c.astype(np.int64) - 1, 4).tolist(), 1, i), np.uint8)
        negs.append(np.where(o < 4, o + 1, 0).astype(np.uint8))
    for p in b["patterns"]:
        S = ms.log_odds(np.array(p["pwm"], np.float32), V0)
        lo, hi = ms.score_range(S)
        P = ms.histogram(ms.best_scores(seqs, S, True), lo, hi)
        N = ms.histogram(ms.best_scores(negs, S, True), lo, hi)
        assert abs(ms.auc(P, N) - p["zoops_score"]) < 1e-3, p["iupac_motif"]
        assert abs(ms.occur(P, N) - p["occur"]) < 1e-3, p["iupac_motif"]


@pytest.mark.parametrize("world", [1, 2, 3])
def test_cli_ranks_shuffle_what_one_process_shuffles(cli_runs, tmp_path, world):
    args = [FA, "-w", "10", "--score-motifs", "--score-negatives", "shuffled"]
    _, so, se, meme, js = cli_runs["shuffled"]
    for rank, (rrc, rso, rse, rmeme, rjs) in enumerate(run_ranks(args, world, tmp_path)):
        assert rrc == 0, (rank, rse.decode()[-2000:])
        if rank == 0:
            assert rmeme == meme and rjs == js and rso == so
        else:
            assert rso == b"" and rmeme is None and rjs is None


def test_cli_refuses_another_value(tmp_path):
    """as the other flags treat a bad argument: exit status 4 with the flag named, nothing written"""
    rc, _, se, meme, js = run_plain([FA, "-w", "10", "--score-motifs", "--score-negatives", "nonsense"], tmp_path, tag="bad")
    assert rc == 4 and b"--score-negatives" in se and meme is None and js is None
