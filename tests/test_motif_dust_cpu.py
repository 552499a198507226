"""--mask-low-complexity without a device: the two restatements of tests/motif_dust_model.py -- the definition read
literally and the recurrence that the kernel follows -- held equal on random sequences and on every constructed case that
tests/test_gpu_motif_dust.py runs on the device; every constructed case held to its class; and what the mask is for,
through the oracle's count and sweep: the tracts' words among the seeds without it, none with it, the planted word's
seeds kept."""
import os

import numpy as np
import pytest

import motif_dust_model as md
import motif_score_model as ms
from oracle import oracle as po


def both_ways(codes, T):
    s, v = md.letters(codes)
    a, b = md.mask_bruteforce(s, v, T), md.mask(s, v, T)
    assert np.array_equal(a, b), ("".join("NACGT"[x] for x in codes), T, np.flatnonzero(a != b)[:8])
    return b


def test_the_flank_has_no_repeated_triplet():
    F = md.de_bruijn_flank()
    tr = [F[i:i + 3] for i in range(len(F) - 2)]
    assert len(F) == 62 and len(set(tr)) == len(tr) == 60 and not any(x * 3 in F for x in "ACGT")
    s, v = md.letters(md.codes_of(F))
    assert md.mask(s, v, 20).all() and not md.perfect_intervals(s, v, 20)


def test_definition_and_recurrence_agree_on_random_sequences():
    seqs = md.random_sequences(1, 260)
    masked = 0
    for k, c in enumerate(seqs):
        T = (20, 20, 10, 5, 30, 1, 60)[k % 7]
        out = both_ways(c, T)
        masked += int(((c >= 1) & ~out).sum())
    assert masked > 2000
    assert {len(c) for c in seqs} >= {0, 1, 2, 3}  # (the shortest lengths are among them)


@pytest.mark.parametrize("case", md.cases(), ids=lambda c: c["name"])
def test_constructed_cases(case):
    seqs, T = case["seqs"], case["T"]
    # (the definition is slow: of the 32 alignments of a long repeat every fifth is held to it, all to the recurrence)
    outs = [both_ways(c, T) if len(seqs) <= 16 or k % 5 == 0 else md.mask(*md.letters(c), T) for k, c in enumerate(seqs)]
    # all sequences in one pass of the recurrence (what the device tests compare with) is the same thing
    masked, bits, touched = md.mask_codes(seqs, T)
    for c, o, m in zip(seqs, outs, masked):
        assert np.array_equal(np.where(o, c, 0), m)
    assert bits == sum(int(((c >= 1) & ~o).sum()) for c, o in zip(seqs, outs))
    assert touched == sum(bool(((c >= 1) & ~o).any()) for c, o in zip(seqs, outs))
    got = md.masked_runs(seqs, masked)
    cls = case["cls"]
    if cls == "nothing":
        assert bits == 0
    elif cls == "run":
        assert got == [case["run"]]  # from the run's first base to its last, and nothing else
    elif cls == "runs_exact":
        assert got == case["runs"]
    elif cls == "runs":
        assert len(got) == len(case["runs"])  # one piece per sequence: a run longer than the window is covered end to end
        for (k, a, b), (k2, a2, b2) in zip(got, case["runs"]):
            assert k == k2 and a <= a2 and b >= b2 and a2 - a <= 8 and b - b2 <= 8, (got, case["runs"])
    elif cls == "ties":
        for k, i, l, i2, l2 in case["ties"]:
            s, v = md.letters(seqs[k])
            N = md.interval_nums(*md.triplets(s, v))
            assert (i, l) in md.perfect_intervals(s, v, T)
            assert i <= i2 and i2 + l2 <= i + l and (i2, l2) != (i, l) and N[i2, l2] * (l - 1) == N[i, l] * (l2 - 1)
    elif cls == "overlap":
        s, v = md.letters(seqs[0])
        P = md.perfect_intervals(s, v, T)
        assert any(i < i2 < i + l + 2 < i2 + l2 + 2 for i, l in P for i2, l2 in P), P
        assert len(md.masked_runs(seqs[:1], masked[:1])) == 1  # their union, in one piece
    else:
        assert cls == "model"
    if cls != "nothing" and not case["name"].startswith("lengths"):
        assert bits > 0


def test_an_invalid_base_splits_a_run_and_each_half_is_judged_alone():
    run = "A" * 30
    for q in (12, 13, 14):
        c = md.codes_of(run[:q] + "N" + run[q + 1:])
        s, v = md.letters(c)
        out = md.mask(s, v, 20)
        assert not out.any()  # both halves (>= 7 bases) go; the invalid base was never valid
        alone = [md.mask(*md.letters(md.codes_of("A" * q)), 20), md.mask(*md.letters(md.codes_of("A" * (29 - q))), 20)]
        assert not alone[0].any() and not alone[1].any()
    c = md.codes_of("A" * 7 + "N" + "A" * 6 + "C")
    masked, bits, _ = md.mask_codes([c], 20)
    assert md.masked_runs([c], masked) == [(0, 0, 7)] and bits == 7  # the half of 6 sits at equality and stays


def test_seams_and_many_sequences_are_what_they_say():
    c = md.seam_sequence()
    assert len(c) == 70000
    masked, bits, _ = md.mask_codes([c], 20)
    gone = np.asarray(masked[0]) != c
    at = np.arange(64, 70000 - 70, 64)
    assert (gone[at] | gone[at - 1]).mean() > 0.9  # a masked run lies across nearly every multiple of 64
    seqs, idx, pool = md.many_sequences()
    assert len(seqs) == 100000 and {len(s) for s in seqs} == set(range(1, 301))


# ---- why: what low-complexity tracts do to the seeds ---------------------------------------------------------------------------
def discover(seqs, W, bg_seqs=None):
    """the reference's seeds of a sequence set, ranked: both strands, order 2 (the model of bg_seqs, the unmasked set),
    default thresholds"""
    codes, offs = ms.flatten(seqs)
    counts, ltot = po.count(codes, offs, W, True)
    V = po.bg_V(po.bg_counts(*ms.flatten(bg_seqs if bg_seqs is not None else seqs), 2), 2)
    _, _, z = po.stats(W, counts, po.bgprob(W, 2, V, True), ltot)
    return [po.kmer_str(int(x), W) for x in po.select(W, z, counts)]


def revcomp_str(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def canonical(s):
    """a k-mer as the both-strand count holds it: the smaller of the word and its reverse complement"""
    return min(s, revcomp_str(s))


def of_the_word(seed, word="TGACTCAGCA"):
    """the seed is a piece of the planted word itself, on either strand"""
    return seed in word or seed in revcomp_str(word)


@pytest.mark.parametrize("W", [8, 10])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_tract_words_leave_the_seeds_and_the_planted_word_stays(seed, W):
    seqs = md.tracts(seed)
    masked, bits, touched = md.mask_codes(seqs, 20)
    before, after = discover(seqs, W), discover(masked, W, bg_seqs=seqs)
    low = [s for s in before if md.period(s) <= 2]
    print("seed %d W %d: %d bases masked in %d sequences; seeds %d -> %d, of period <= 2: %d -> %d"
          % (seed, W, bits, touched, len(before), len(after), len(low), sum(md.period(s) <= 2 for s in after)))
    assert len(low) >= 1
    assert not any(md.period(s) <= 2 for s in after), after
    # under both strands a word and its reverse complement are one k-mer, which the count holds as one object; which strand
    # a run names it on follows from the order of exact z ties (include/pengk.h, pengk_seed_candidates), which the mask may
    # change.  So the seeds are compared as that object, strand-folded on both sides
    kept = {canonical(s) for s in before if of_the_word(s)}
    assert kept and kept <= {canonical(s) for s in after}, (kept, after)


def test_mafk_figures(golden_dir):
    """the figures of the README's table: tests/golden/MafK.fasta at W = 10"""
    codes, offs = po.read_fasta(os.path.join(golden_dir, "MafK.fasta"))
    seqs = [codes[a:b] for a, b in zip(offs[:-1], offs[1:])]
    masked, bits, touched = md.mask_codes(seqs, 20)
    before, after = discover(seqs, 10), discover(masked, 10, bg_seqs=seqs)
    print("MafK.fasta: %d of %d bases masked in %d of %d sequences; seeds %d -> %d, of period <= 2: %d -> %d"
          % (bits, len(codes), touched, len(seqs), len(before), len(after), sum(md.period(s) <= 2 for s in before),
             sum(md.period(s) <= 2 for s in after)))
    assert 0 < bits < len(codes) // 10 and 0 < touched < len(seqs)
    assert not any(md.period(s) <= 2 for s in after)
