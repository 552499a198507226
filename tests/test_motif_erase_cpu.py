"""--erase without a device: the numpy model of tests/motif_erase_model.py certified -- its constructed mask cases hold
the classes they are named for, the host packer (pengk_pack, pure CPU) writes the model's words and items on the pack
cases, so that the same cases mean the same thing on the GPU (tests/test_gpu_motif_erase.py) -- and the two scenarios
that say why erasing is worth a flag: a planted weak motif that the seeds of a strong one keep out of the optimised
places, and the MafK rows of the README."""
import os

import numpy as np
import pytest

import peng_motif_amd as pk
import motif_erase_model as me
import motif_score_model as ms
import motif_sites_model as mst
from oracle import oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
BG = np.full(4, 0.25, np.float32)
A, B = "TGACTCAGCA", "GGCTGGAGTG"


@pytest.fixture(scope="module")
def cases():
    return {c["name"]: c for c in me.mask_cases()}


def all_sites(c):
    return [mst.sites(c["seqs"], S, t, c["both"]) for S, t in zip(c["Ss"], c["ts"])]


def covered(c):
    return [np.flatnonzero(v).tolist() for v in me.cover(c["seqs"], c["Ss"], c["ts"], c["both"])[0]]


# ---- the mask cases hold their classes -----------------------------------------------------------------------------------
def test_case_first_and_last_window(cases):
    c = cases["first_and_last_window"]
    L = len(c["seqs"][0])
    assert [(p, s) for _, p, s, _ in all_sites(c)[0]] == [(0, 0), (L - 4, 0)]
    assert covered(c)[0] == [0, 1, 2, 3, L - 4, L - 3, L - 2, L - 1]


def test_case_overlapping_sites(cases):
    c = cases["overlapping_sites"]
    assert [p for _, p, _, _ in all_sites(c)[0]] == [5, 6, 7]  # three sites, four bases each ...
    assert covered(c)[0] == list(range(5, 11))                 # ... one cover of six
    assert me.mask(c["seqs"], c["Ss"], c["ts"], c["both"])[1:] == (np.array([3], np.uint64), 6)


def test_case_minus_strand_only(cases):
    c = cases["minus_strand_only"]
    assert [(p, s) for _, p, s, _ in all_sites(c)[0]] == [(7, 1)]
    assert not mst.sites(c["seqs"], c["Ss"][0], c["ts"][0], False)


def test_case_cover_ends_at_bit_31_and_32(cases):
    c = cases["cover_ends_at_bit_31_and_32"]
    cov = covered(c)
    assert cov[0] == [28, 29, 30, 31] and cov[1] == [29, 30, 31, 32]
    words = me.valid_words(me.mask(c["seqs"], c["Ss"], c["ts"], c["both"])[0]).reshape(2, -1)
    assert words[0, 0] == 0x0FFFFFFF and words[0, 1] & 1 == 1
    assert words[1, 0] == 0x1FFFFFFF and words[1, 1] & 3 == 2


def test_case_window_across_invalid_base(cases):
    c = cases["window_across_invalid_base"]
    s = all_sites(c)[0]
    assert [(i, p) for i, p, _, _ in s] == [(0, 15)]  # neither ACNGG nor ACGN is a site
    masked, _, erased = me.mask(c["seqs"], c["Ss"], c["ts"], c["both"])
    assert erased == 4 and masked[0][2] == 0 and np.array_equal(masked[1], c["seqs"][1])


def test_case_thresholds_at_the_ends_of_the_range(cases):
    c = cases["threshold_above_every_score"]
    assert c["ts"][0] == me.score_range(c["Ss"][0])[1] + 1
    masked, n, erased = me.mask(c["seqs"], c["Ss"], c["ts"], c["both"])
    assert erased == 0 and n[0] == 0 and all(np.array_equal(a, b) for a, b in zip(masked, c["seqs"]))
    c = cases["threshold_below_every_score"]
    assert c["ts"][0] <= me.score_range(c["Ss"][0])[0]
    masked, n, erased = me.mask(c["seqs"], c["Ss"], c["ts"], c["both"])
    w, windows = 5, 0
    for orig, m in zip(c["seqs"], masked):
        ok = (orig >= 1) & (orig <= 4)
        in_window = np.zeros(len(orig), bool)
        for p in range(len(orig) - w + 1):
            if ok[p:p + w].all():
                in_window[p:p + w] = True
                windows += 1
        assert np.array_equal(m == 0, in_window | ~ok)
    assert n[0] == 2 * windows and erased > 0
    assert any(((o >= 1) & (m != 0)).any() for o, m in zip(c["seqs"], masked))  # (valid bases that no all-valid window holds stay)


def test_case_three_groups_cover_one_base(cases):
    c = cases["three_groups_cover_one_base"]
    assert me.groups([len(S) for S in c["Ss"]], c["both"]) == [0, 1, 2]
    per = [me.cover(c["seqs"], [S], [t], c["both"])[0] for S, t in zip(c["Ss"], c["ts"])]
    assert all((per[0][i] & per[1][i] & per[2][i]).any() for i in range(len(c["seqs"])))
    _, n, erased = me.mask(c["seqs"], c["Ss"], c["ts"], c["both"])
    assert erased == sum(int((per[0][i] | per[1][i] | per[2][i]).sum()) for i in range(len(c["seqs"])))  # each base once
    assert erased < sum(int(p[i].sum()) for p in per for i in range(len(c["seqs"])))


def test_groups_of_41_motifs_of_width_4():
    assert me.groups([4] * 41, True) == [0] * 20 + [1] * 20 + [2]
    assert me.groups([4] * 41, False) == [0] * 40 + [1]


# ---- the host packer against the model: the yardstick of the device packer -----------------------------------------------
@pytest.mark.parametrize("W", [4, 10, 14])
def test_host_packer_writes_the_models_layout(W):
    classes = set()
    for name, seqs, M in me.pack_cases(W):
        p = pk.Packed(*ms.flatten(seqs), W, M)
        m = me.pack(seqs, W, M)
        assert np.array_equal(p.words, m["words"]), name
        assert np.array_equal(p.items, m["items"]), name
        got = (p.n_bases, p.n_windows, p.max_bin_bound, p.all_whole, p.max_len, p.item_windows)
        assert got == (m["n_bases"], m["n_windows"], m["max_bin_bound"], m["all_whole"], m["max_len"], M or me.DEFAULT_ITEM_WINDOWS), name
        classes.add(name.split("/")[0])
    assert classes == {"alignment", "runs_and_N", "item_lengths", "long", "nothing_stored", "nothing_between", "no_sequence"}


def test_render_report():
    rounds = [dict(seeds=16, windows=186000, bases_erased=0, motifs=[("TGACTCAG", 8, 1234, 1010), ("NNACTCAN", 8, -5, 3)]),
              dict(seeds=0, windows=170000, bases_erased=9990, motifs=[])]
    assert me.render_report(rounds) == (me.REPORT_HEADER + "1\tTGACTCAG\t8\t12.34\t1010\t16\t186000\t0\n"
                                        "1\tNNACTCAN\t8\t-0.05\t3\t16\t186000\t0\n2\t-\t0\t-\t0\t0\t170000\t9990\n")


# ---- why: what the seeds of a strong motif hide -----------------------------------------------------------------------------
def discover(seqs, W):
    """the reference's seeds of a sequence set, ranked: both strands, order 2, default thresholds -> (k-mer strings, ltot)"""
    codes, offs = ms.flatten(seqs)
    counts, ltot = po.count(codes, offs, W, True)
    V = po.bg_V(po.bg_counts(codes, offs, 2), 2)
    _, _, z = po.stats(W, counts, po.bgprob(W, 2, V, True), ltot)
    return [po.kmer_str(int(x), W) for x in po.select(W, z, counts)], ltot


def pwm_mask(seqs, word, P=1e-4):
    S = ms.log_odds(me.consensus_pwm(word), BG)
    lo, tail = mst.tail_pvalues(S, BG)
    return me.mask(seqs, [S], [mst.threshold(lo, tail, P)], True)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_planted_weak_motif_surfaces_after_the_mask(seed):
    seqs = me.planted(seed)
    first, _ = discover(seqs, 8)
    print("seed %d round 1: %d seeds, the first B seed at rank %s" % (
        seed, len(first), next((k + 1 for k, s in enumerate(first) if me.shares_kmer(s, B)), None)))
    assert len(first) >= 5 and all(me.shares_kmer(s, A) for s in first[:5])
    masked, n, erased = pwm_mask(seqs, A)
    second, _ = discover(masked, 8)
    print("seed %d round 2: %d sites, %d bases erased, seeds %s" % (seed, int(n[0]), erased, second))
    assert second and all(me.shares_kmer(s, B) for s in second)


def test_mafk_rows():
    """the README's table: MafK.fasta at W = 10, as it is and with the sites of the MARE masked"""
    mare = "TGCTGASTCAGCA"
    seqs = ms.read_fasta_codes(os.path.join(GOLD, "MafK.fasta"))
    first, _ = discover(seqs, 10)
    masked, n, erased = pwm_mask(seqs, mare)
    second, _ = discover(masked, 10)
    hit = sum(1 for m, s in zip(masked, seqs) if not np.array_equal(m, s))
    share1 = sum(me.shares_kmer(s, mare.replace("S", "C")) or me.shares_kmer(s, mare.replace("S", "G")) for s in first[:50])
    share2 = sum(me.shares_kmer(s, mare.replace("S", "C")) or me.shares_kmer(s, mare.replace("S", "G")) for s in second[:50])
    new = [s for s in second[:50] if s not in first[:50]]
    print("| the input as it is | %d | %d |" % (len(first), share1))
    print("| after masking the MARE sites (%d sites in %d sequences; %d of %d bases) | %d | %d |" % (
        int(n[0]), hit, erased, sum(len(s) for s in seqs), len(second), share2))
    print("seeds among the second run's first 50 that the first run never optimised: %d (%s ...)" % (len(new), ", ".join(new[:4])))
    assert share2 < share1
    assert len(new) >= 20
