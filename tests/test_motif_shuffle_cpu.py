"""CPU checks of the dinucleotide-preserving shuffle's model (tests/motif_shuffle_model.py; include/pengk.h,
pengk_shuffle_sequences): its invariants, its uniformity over all sequences with the same doublets and ends, what it is
for (a control that keeps every sequence's own composition), the layout helpers, the kernel's per-sequence body run on
the host, and the CLI's handling of --score-negatives.  No device compute here."""
import collections
import os
import subprocess

import numpy as np
import pytest

import peng_motif_amd as pk
import motif_score_model as ms
import motif_shuffle_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "peng-motif_amd", "host", "peng_motif")
GOLD = os.path.join(ROOT, "tests", "golden")


def test_library_and_wrapper_have_the_shuffle():
    assert hasattr(pk.lib(), "pengk_shuffle_sequences") and hasattr(pk.Context, "shuffle_sequences")


def test_invariants_on_random_sequences():
    rng = np.random.default_rng(0)
    most_draws = 0
    for it in range(3000):
        L, A = int(rng.integers(0, 80)), int(rng.integers(1, 6))
        s = rng.integers(0, A, L).tolist()
        st = {}
        o = sm.shuffle(s, int(rng.integers(0, 2 ** 63)), it, st)
        assert len(o) == L
        if L == 0:
            continue
        assert o[0] == s[0] and o[-1] == s[-1]
        assert np.array_equal(sm.doublets(o), sm.doublets(s)), (it, s)
        assert st["rem"] == [0] * 5 and st["cnt"] == [[0] * 5] * 5
        most_draws = max(most_draws, st["tree_draws"])
        if L <= 2:
            assert o == s
    assert most_draws > 0


def same_doublets_and_ends(s):
    """every sequence with the doublet counts, the first and (hence) the last letter of s, by exhaustive search"""
    L, c, res = len(s), collections.Counter(zip(s[:-1], s[1:])), []

    def rec(cur):
        if len(cur) == L:
            res.append(tuple(cur))
            return
        for v in range(5):
            if c[(cur[-1], v)] > 0:
                c[(cur[-1], v)] -= 1
                cur.append(v)
                rec(cur)
                cur.pop()
                c[(cur[-1], v)] += 1
    rec([s[0]])
    return sorted(set(res))


@pytest.mark.parametrize("s,distinct,chi_max", [([0, 1, 2, 0, 1, 3, 0, 2, 1, 0, 4, 0, 1], 168, 230.0),
                                                ([0, 0, 1, 0, 1, 1, 0, 2, 2, 0, 1, 0], 60, 98.0),
                                                ([1, 2, 3, 1, 2, 3, 1, 3, 2, 1], 21, 46.0)])
def test_uniform_over_every_sequence_with_the_same_doublets(s, distinct, chi_max):
    """seed 12345, g = 0 .. 200 * distinct - 1: every doublet-preserving sequence occurs and no other; chi-square at most
    about the 99.9 % point of its distribution (167, 59, 20 degrees of freedom).  The inputs are fixed, so the values are
    too: 177.4, 55.0 and 31.8."""
    every = same_doublets_and_ends(s)
    assert len(every) == distinct and all(e[-1] == s[-1] for e in every)
    N = 200 * distinct
    h = collections.Counter(tuple(sm.shuffle(s, 12345, g)) for g in range(N))
    assert sorted(h) == every
    e = N / distinct
    chi = sum((h[a] - e) ** 2 / e for a in every)
    print("chi-square", round(chi, 1), "of", distinct, "results over", N)
    assert chi <= chi_max, chi


def test_shuffled_negatives_do_not_score_composition():
    """1500 x 100 bp alternating 30 % and 70 % GC, a GC-rich 8-mer PWM that is NOT planted, both strands: against each
    sequence's own shuffle the AUC is 0.5 (|auc - 0.5| = 0.010 here), against samples of the global order-2 model it
    measures the composition (|auc - 0.5| = 0.104 here)."""
    rng = np.random.default_rng(1)
    n, L = 1500, 100
    seqs = []
    for i in range(n):
        gc = 0.3 if i % 2 == 0 else 0.7
        seqs.append((rng.choice(4, L, p=[(1 - gc) / 2, gc / 2, gc / 2, (1 - gc) / 2]) + 1).astype(np.uint8))
    allb = np.concatenate([s - 1 for s in seqs])
    V0 = np.bincount(allb, minlength=4) / len(allb)
    c1, c2 = np.ones((4, 4)), np.ones((16, 4))
    for s in seqs:
        b = s.astype(int) - 1
        np.add.at(c1, (b[:-1], b[1:]), 1)
        np.add.at(c2, (b[:-2] * 4 + b[1:-1], b[2:]), 1)
    V = [V0.astype(np.float32), (c1 / c1.sum(1, keepdims=True)).astype(np.float32).reshape(-1),
         (c2 / c2.sum(1, keepdims=True)).astype(np.float32).reshape(-1)]
    neg_sampled = [x + 1 for x in ms.sample([L] * n, 7, 0, 2, ms.thresholds(V, 2))]
    neg_shuffled = [np.array(sm.shuffle((s - 1).tolist(), 7, i), np.uint8) + 1 for i, s in enumerate(seqs)]
    pwm = np.full((8, 4), 0.05)
    for j, a in enumerate([2, 1, 1, 2, 2, 1, 2, 1]):  # G C C G G C G C
        pwm[j, a] = 0.85
    S = ms.log_odds(pwm, V0)
    lo, hi = ms.score_range(S)
    P = ms.histogram(ms.best_scores(seqs, S, True), lo, hi)
    auc = {name: ms.auc(P, ms.histogram(ms.best_scores(neg, S, True), lo, hi))
           for name, neg in (("sampled", neg_sampled), ("shuffled", neg_shuffled))}
    print("auc", auc)
    assert abs(auc["shuffled"] - 0.5) < 0.03, auc
    assert abs(auc["sampled"] - 0.5) > 0.05, auc


@pytest.mark.parametrize("L", [0, 1, 31, 32, 33, 64, 65])
def test_pack_and_unpack_round_trip(L):
    rng = np.random.default_rng(L)
    seqs = [rng.integers(0, 5, L).astype(np.uint8), rng.integers(0, 5, 7).astype(np.uint8), rng.integers(0, 5, L).astype(np.uint8)]
    words, valid, offs, lens = sm.pack(seqs)
    assert lens.tolist() == [L, 7, L] and all(o % 32 == 0 for o in offs)
    assert len(words) == max(2 * ((L + 31) // 32) + 1, 1)
    back = sm.unpack(words, valid, offs, lens)
    assert all(np.array_equal(a, b) for a, b in zip(back, seqs))
    # padding bits, and the code of a letter 4, are zero: whole words compare equal
    for o, n in zip(offs, lens):
        for j in range((int(n) + 31) // 32):
            k = min(32, int(n) - 32 * j)
            w, v = int(words[int(o) // 32 + j]), int(valid[int(o) // 32 + j])
            assert w >> (2 * k) == 0 and v >> k == 0
            for b in range(k):
                if not (v >> b) & 1:
                    assert (w >> (2 * b)) & 3 == 0
    # the library's host builder makes the same layout of the same letters (its byte codes: 0 = other, 1..4 = A,C,G,T)
    lay = pk.ScanLayout(*ms.flatten([np.where(s < 4, s + 1, 0).astype(np.uint8) for s in seqs]))
    nw = len(words) if L else 1
    assert np.array_equal(lay.words[:nw], words[:nw]) and np.array_equal(lay.valid[:nw], valid[:nw])
    assert np.array_equal(lay.offs, offs) and np.array_equal(lay.lens, lens)


def test_kernel_body_on_the_host_equals_the_model(tmp_path):
    """csrc/shuffle_core.h is the kernel's per-sequence body; a host compiler takes it too.  Letters and whole output
    words against the model, with and without validity words."""
    exe = str(tmp_path / "shuffle_core_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "peng-motif_amd", "csrc"),
                    os.path.join(ROOT, "tests", "tools", "shuffle_core_driver.cpp"), "-o", exe], check=True)
    rng = np.random.default_rng(5)
    cases = []
    for it in range(400):
        L, A = int(rng.integers(0, 150)), int(rng.integers(1, 6))
        cases.append((int(rng.integers(0, 2 ** 64, dtype=np.uint64)), int(rng.integers(0, 2 ** 32)),
                      int(A <= 4 and it % 3 == 0), rng.integers(0, A, L).tolist()))
    cases.append((5, 2 ** 32 - 1, 0, [0] * 199 + [1]))
    cases.append((2 ** 63 + 5, 3, 0, ([0] * 9 + [1]) * 300 + [4] * 40 + [0] * 2000 + [2]))
    text = "".join("%d %d %d %s\n" % (sd, g, av, "".join(map(str, s)) or "-") for sd, g, av, s in cases)
    out = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    assert len(out) == len(cases)
    for (sd, g, av, s), line in zip(cases, out):
        want = sm.shuffle(s, sd, g)
        w, v, _, _ = sm.pack([want])
        exp = ("".join(map(str, want)) or "-") + "".join(" %016x:%08x" % (int(w[j]), int(v[j])) for j in range((len(s) + 31) // 32))
        assert line == exp, (sd, g, av, s)


def test_help_lists_score_negatives_next_to_score_seed():
    r = subprocess.run([CLI, "-h"], stdout=subprocess.PIPE)
    assert r.returncode == 0
    lines = r.stdout.decode().splitlines()
    at = [i for i, l in enumerate(lines) if "--score-seed" in l]
    assert len(at) == 1 and "--score-negatives" in lines[at[0] + 1] and "sampled" in lines[at[0] + 1]
    assert any("shuffled" in l for l in lines[at[0] + 1:at[0] + 4])


@pytest.mark.parametrize("bad", ["nonsense", "Shuffled", "", "shuffle"])
def test_bad_score_negatives_is_refused(tmp_path, bad):
    """as the other flags treat a bad argument (--strand, --optimization_score): the help, the flag named in an error
    line, exit status 4, before anything is read or written"""
    r = subprocess.run([CLI, os.path.join(GOLD, "MafK.fasta"), "--score-motifs", "--score-negatives", bad, "-o", str(tmp_path / "o.meme")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 4, (bad, r.returncode, r.stderr[-500:])
    assert b"--score-negatives" in r.stderr.splitlines()[-2] and not (tmp_path / "o.meme").exists()
    r = subprocess.run([CLI, os.path.join(GOLD, "MafK.fasta"), "--score-negatives"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=60)
    assert r.returncode == 4 and b"No expression following --score-negatives" in r.stderr
