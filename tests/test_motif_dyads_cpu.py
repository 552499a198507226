"""--dyads on the CPU (include/pengk.h, "spaced dyads"): the numpy model of tests/motif_dyads_model.py against the definition
read literally, pengk_dyad_summary against the model on the model's tables -- keys, counts and families exactly, p bit for
bit, the tail the library's own --, and the planted scenarios of the README's table on seeds 1, 2, 3.  What the contiguous
search makes of the same inputs at W = 8 is printed through the oracle, not asserted."""
import numpy as np
import pytest

import peng_motif_amd as pk
import motif_dyads_model as dy
import motif_score_model as ms
from oracle import oracle as po


def test_symbols():
    assert hasattr(pk.lib(), "pengk_dyad_count") and hasattr(pk.lib(), "pengk_dyad_summary")
    assert "pengk_dyad_count" in pk.EXPORTS and "pengk_dyad_summary" in pk.EXPORTS
    assert pk.DYAD_MAX_GAP == dy.MAX_GAP == 26


# ---- the model ------------------------------------------------------------------------------------------------------------
def test_reverse_complement_tables():
    assert dy.RC3[dy.key_of("AAA", "ACG") & 63] == dy.key_of("AAA", "CGT") & 63
    assert dy.RC6[dy.key_of("CGG", "CCG")] == dy.key_of("CGG", "CCG")      # CGG n CCG is its own reverse complement
    assert dy.RC6[dy.key_of("ACC", "GTA")] == dy.key_of("TAC", "GGT")
    assert sum(int(dy.RC6[k]) == k for k in range(4096)) == 64
    assert len({dy.canonical(k) for k in range(4096)}) == 2080
    assert dy.dyad_string(dy.key_of("CGG", "CCG"), 11) == "CGGnnnnnnnnnnnCCG"


@pytest.mark.parametrize("both", [False, True])
def test_model_is_the_definition(both):
    rng = np.random.default_rng(3)
    seqs = dy.random_sequences(4, list(range(12)) + [31, 32, 33, 40, 64, 65, 90])
    for c in seqs[12:]:
        c[rng.integers(0, len(c), 2)] = 0
    seqs.append(dy.codes_of("CGG" + "A" * 11 + "CCG"))
    for G in (0, 1, 20, 26):
        counts, mono = dy.tables(seqs, G, both)
        wc, wm = np.zeros_like(counts), np.zeros_like(mono)
        for c in seqs:
            a, b = dy.tables_literal(c, G, both)
            wc += a
            wm += b
        assert np.array_equal(counts, wc) and np.array_equal(mono, wm)
        if both:
            assert not counts[:, [k for k in range(4096) if dy.canonical(k) != k]].any()
    w = [3, 0, 2] + [1] * (len(seqs) - 3)
    a = dy.tables(seqs, 20, both, weights=w)
    b = dy.tables(seqs[:1] * 3 + seqs[2:3] * 2 + seqs[3:], 20, both)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_a_dyad_that_is_its_own_reverse_complement_counts_once():
    c = dy.codes_of("CGG" + "ACGTACGTACG" + "CCG")
    counts, mono = dy.tables([c], 11, True)
    assert counts[11, dy.key_of("CGG", "CCG")] == 1 and counts[11].sum() == 1
    assert mono.sum() == 15


# ---- the summary ------------------------------------------------------------------------------------------------------------
def check_summary(counts, mono, both, min_count=5, E=0.01):
    want = dy.summary(counts, mono, both, pk.binomial_log10_sf, min_count, E)
    got = pk.dyad_summary(counts, mono, both, min_count, E)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for k in ("gap", "key", "count", "positions", "family", "is_head"):
            assert g[k] == w[k], (k, g, w)
        for k in ("p", "expected", "log10_pvalue", "log10_evalue", "other_gaps_mean"):
            assert np.float64(g[k]).tobytes() == np.float64(w[k]).tobytes(), (k, g, w)
        assert g["log10_pvalue"] == pk.binomial_log10_sf(g["positions"], g["count"], g["p"])
    return got


@pytest.fixture(scope="module")
def scenario():
    return {(name, frac, seed): dy.planted(seed, a, g, b, frac)
            for name, a, g, b in (("CGG n11 CCG", "CGG", 11, "CCG"), ("ACC n9 GTA", "ACC", 9, "GTA"))
            for frac in (0.3, 0.05) for seed in (1, 2, 3)}


@pytest.mark.parametrize("both", [False, True])
def test_summary_is_the_model(scenario, both):
    seqs = scenario[("ACC n9 GTA", 0.3, 1)]
    for G in (0, 9, 20):
        counts, mono = dy.tables(seqs, G, both)
        rep = check_summary(counts, mono, both, E=10.0)   # (a long report: many families, ties in the order)
        assert len(rep) > 20 or G == 0
        check_summary(counts, mono, both, min_count=1, E=100.0)
    counts, mono = dy.tables(seqs, 20, both)
    full = pk.dyad_summary(counts, mono, both, 5, 10.0)
    assert pk.dyad_summary(counts, mono, both, 5, 10.0, capacity=3) == full   # (a second call with room for all)
    assert check_summary(np.zeros((21, 4096), np.uint64), np.zeros(64, np.uint64), both) == []   # M = 0: nothing
    for bad in (dict(max_evalue=0.0), dict(max_evalue=-1.0)):
        with pytest.raises(pk.PengkError) as e:
            pk.dyad_summary(counts, mono, both, **bad)
        assert e.value.code == pk.ERR_ARG
    with pytest.raises(pk.PengkError) as e:
        pk.dyad_summary(np.zeros((28, 4096), np.uint64), mono, both)
    assert e.value.code == pk.ERR_ARG


def test_families_fold_the_shifted_neighbours():
    X = dy.columns(dy.key_of("CGG", "CCG"), 11)
    assert dy.related(X, dy.columns(dy.key_of("GGA", "CGT"), 11))       # one to the right: GG . . . C in common, 4 columns
    assert dy.related(X, dy.columns(dy.key_of("CGG", "ACC"), 10))   # CGG n10 ACC: the spacer's last base named
    assert not dy.related(X, dy.columns(dy.key_of("CGG", "CCG"), 12))   # another spacing: three columns agree at most
    assert not dy.related(X, dy.columns(dy.key_of("CGG", "CCT"), 11))   # a letter differs
    assert not dy.related(X, dy.columns(dy.key_of("AAA", "TTT"), 11))


# ---- the README's scenarios --------------------------------------------------------------------------------------------------
def w8_seeds(seqs):
    """the reference's seeds at W = 8: both strands, order 2, default thresholds"""
    codes, offs = ms.flatten(seqs)
    counts, ltot = po.count(codes, offs, 8, True)
    V = po.bg_V(po.bg_counts(codes, offs, 2), 2)
    _, _, z = po.stats(8, counts, po.bgprob(8, 2, V, True), ltot)
    return [po.kmer_str(int(x), 8) for x in po.select(8, z, counts)]


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("frac", [0.3, 0.05])
@pytest.mark.parametrize("name,a,g,b", [("CGG n11 CCG", "CGG", 11, "CCG"), ("ACC n9 GTA", "ACC", 9, "GTA")])
def test_planted_dyad_is_found(scenario, name, a, g, b, frac, seed):
    seqs = scenario[(name, frac, seed)]
    counts, mono = dy.tables(seqs, 20, True)
    rep = check_summary(counts, mono, True)
    top = rep[0]
    print("%s in %g %%, seed %d: top %s count %d expected %.1f log10_E %.1f, %d dyads at E <= 0.01 in %d families; W = 8 seeds: %d"
          % (name, 100 * frac, seed, dy.dyad_string(top["key"], top["gap"]), top["count"], top["expected"], top["log10_evalue"],
             len(rep), sum(d["is_head"] for d in rep), len(w8_seeds(seqs))))
    assert (top["key"], top["gap"]) == (dy.canonical(dy.key_of(a, b)), g)
    assert sum(d["is_head"] for d in rep) == 1 and all(d["family"] == 1 for d in rep)
    if frac == 0.05:
        assert top["log10_evalue"] <= -10


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_nothing_planted_nothing_found(seed):
    seqs = dy.planted(seed, frac=0.0)
    counts, mono = dy.tables(seqs, 20, True)
    assert check_summary(counts, mono, True) == []
    rep = check_summary(counts, mono, True, E=100.0)   # (about a hundred lines: 100 of 43 680 tests by chance)
    print("nothing planted, seed %d: best log10_E %.2f; W = 8 seeds: %d" % (seed, rep[0]["log10_evalue"], len(w8_seeds(seqs))))
    assert not any(d["log10_evalue"] <= -2 for d in rep)
