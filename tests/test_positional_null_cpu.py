"""--positional-null composition on the CPU (include/pengk.h, "the composition null of the positional report"): the numpy
model of tests/positional_null_model.py against the definition read position by position, pengk_position_summary_null
against the model on the model's tables -- integers exactly, doubles bit for bit --, h_pairs = NULL against
pengk_position_summary field for field, the constructed edges (equal composition, a bin without pairs, a letter that begins
no pair, a key with G = 0), the gradient scenario of the README on seeds 1, 2, 3 under both nulls, the TATA scenario under
the new one, and the CLI's help and flag errors.  No device compute."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import peng_motif_amd as pk
import motif_positional_model as mp
import positional_null_model as pn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "peng-motif_amd", "host", "peng_motif")
GOLD = os.path.join(ROOT, "tests", "golden")
INTS = ("key", "bin", "count", "total", "bin_positions", "bins_significant", "family", "is_head")
DOUBLES = ("expected", "log10_pvalue", "log10_evalue")


def test_symbols():
    for name in ("pengk_position_pairs", "pengk_position_summary_null"):
        assert hasattr(pk.lib(), name) and name in pk.EXPORTS
    assert hasattr(pk.Context, "position_pairs")


# ---- the pair table of the model -----------------------------------------------------------------------------------------
def model_sequences():
    rng = np.random.default_rng(3)
    lengths = list(range(9)) + [31, 32, 33, 63, 64, 65]
    seqs = mp.random_sequences(4, lengths, skew=True)    # two letters mostly
    for c in seqs[9:]:
        c[rng.integers(0, len(c), 2)] = 0                # invalid bases
    seqs += mp.random_sequences(5, lengths)
    seqs += [mp.codes_of("AC" * 20), mp.codes_of("A" * 33), mp.codes_of("AT" * 16 + "N" + "TA" * 16)]
    return seqs


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("K", [4, 5, 6, 7])
def test_model_is_the_definition(K, both):
    seqs = model_sequences()
    assert set(range(K + 2)) | {31, 32, 33, 63, 64, 65} <= {len(c) for c in seqs}
    for anchor in (mp.START, mp.END, mp.CENTER):
        for S, B in ((3, 9), (1, 64), (10, 20)):
            got = pn.pair_tables(seqs, K, anchor, S, B, both)
            want = np.zeros_like(got)
            standing = np.zeros(B, np.int64)
            for c in seqs:
                p, n = pn.pair_tables_literal(c, K, anchor, S, B, both)
                want += p
                standing += n
            assert np.array_equal(got, want), (anchor, S, B)
            # a row sums to 1 x / 2 x the standing words of its bin
            assert np.array_equal(got.sum(axis=1).astype(np.int64), (2 if both else 1) * standing)
            assert standing.sum() > 0
    w = [3, 0, 2] + [1] * (len(seqs) - 3)
    a = pn.pair_tables(seqs, K, 2, 3, 9, both, weights=w)
    b = pn.pair_tables(seqs[:1] * 3 + seqs[2:3] * 2 + seqs[3:], K, 2, 3, 9, both)
    assert np.array_equal(a, b)


def test_pairs_of_a_few_words_by_hand():
    # ACGTA, K = 4, one bin: the words ACGT and CGTA stand; first pairs AC and CG; on the other strand ACGT reads ACGT (AC)
    # and CGTA reads TACG (TA)
    one = pn.pair_tables([mp.codes_of("ACGTA")], 4, mp.START, 10, 1, False)
    assert one.sum() == 2 and one[0, 4 * 0 + 1] == 1 and one[0, 4 * 1 + 2] == 1
    two = pn.pair_tables([mp.codes_of("ACGTA")], 4, mp.START, 10, 1, True)
    assert two.sum() == 4 and two[0, 4 * 0 + 1] == 2 and two[0, 4 * 1 + 2] == 1 and two[0, 4 * 3 + 0] == 1
    # every standing word, not only the clump heads: 30 bases of A hold 25 words of 6
    assert pn.pair_tables([mp.codes_of("A" * 30)], 6, mp.START, 100, 1, False)[0, 0] == 25
    assert mp.tables([mp.codes_of("A" * 30)], 6, mp.START, 100, 1, False).sum() == 1


# ---- the summary ---------------------------------------------------------------------------------------------------------
def check_summary(counts, pairs, K, both, min_count=5, E=0.01):
    want = pn.summary(counts, pairs, K, both, pk.binomial_log10_sf, min_count, E)
    got = pk.position_summary(counts, K, both, min_count, E, pairs=pairs)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for k in INTS:
            assert g[k] == w[k], (k, g, w)
        for k in DOUBLES:
            assert np.float64(g[k]).tobytes() == np.float64(w[k]).tobytes(), (k, g, w)
    return got


@pytest.fixture(scope="module")
def tata():
    return {(frac, seed): mp.planted(seed, frac) for frac in (0.1, 0.0) for seed in (1, 2, 3)}


SHAPES = ((6, 0, 10, 20), (4, 2, 7, 15), (5, 1, 10, 20), (7, 0, 20, 10))   # those of test_summary_is_the_model


@pytest.mark.parametrize("both", [False, True])
def test_summary_is_the_model(tata, both):
    seqs = tata[(0.1, 1)]
    for K, anchor, S, B in SHAPES:
        counts = mp.tables(seqs, K, anchor, S, B, both)
        pairs = pn.pair_tables(seqs, K, anchor, S, B, both)
        rep = check_summary(counts, pairs, K, both, E=100.0)     # (a long report: many families, several bins a key)
        assert len(rep) > 20
        check_summary(counts, pairs, K, both, min_count=1, E=1000.0)
        check_summary(counts, pairs, K, both)
    counts, pairs = mp.tables(seqs, 6, 0, 10, 20, both), pn.pair_tables(seqs, 6, 0, 10, 20, both)
    full = pk.position_summary(counts, 6, both, 5, 100.0, pairs=pairs)
    assert len(full) > 3 and pk.position_summary(counts, 6, both, 5, 100.0, capacity=3, pairs=pairs) == full
    assert pk.position_summary(counts, 6, both, 5, 100.0, capacity=0, pairs=pairs) == full
    assert check_summary(np.zeros((20, 4096), np.uint64), pairs, 6, both) == []   # Nt = 0: nothing
    for bad in (dict(max_evalue=0.0), dict(max_evalue=-1.0)):
        with pytest.raises(pk.PengkError) as e:
            pk.position_summary(counts, 6, both, pairs=pairs, **bad)
        assert e.value.code == pk.ERR_ARG


def raw_summary(fn, counts, K, both, min_count, E, pairs=False):
    """the lines of one call as tuples of every field, the doubles as their bytes (the struct's padding is not a field)"""
    c = np.ascontiguousarray(counts, np.uint64)
    n = C.c_uint64()
    out = (pk.PositionWordStruct * 4096)()
    args = (int(K), c.shape[0], int(both), int(min_count), float(E), C.addressof(out), 4096, C.byref(n))
    rc = fn(c.ctypes.data, None, *args) if pairs else fn(c.ctypes.data, *args)
    assert rc == 0 and n.value <= 4096
    fields = [k for k, _ in pk.PositionWordStruct._fields_]
    assert set(fields) == set(INTS + DOUBLES)
    return [tuple(np.float64(getattr(out[i], k)).tobytes() if k in DOUBLES else getattr(out[i], k) for k in fields)
            for i in range(n.value)], n.value


@pytest.mark.parametrize("both", [False, True])
def test_without_a_pair_table_it_is_the_flat_summary(tata, both):
    seqs = tata[(0.1, 1)]
    for K, anchor, S, B in SHAPES:
        counts = mp.tables(seqs, K, anchor, S, B, both)
        for mc, E in ((5, 100.0), (1, 1000.0), (5, 0.01)):
            old, n_old = raw_summary(pk.lib().pengk_position_summary, counts, K, both, mc, E)
            new, n_new = raw_summary(pk.lib().pengk_position_summary_null, counts, K, both, mc, E, pairs=True)
            assert n_old == n_new and old == new      # every field of every line
            got = pk.position_summary(counts, K, both, mc, E)
            want = mp.summary(counts, K, both, pk.binomial_log10_sf, mc, E)
            assert len(got) == len(want) == n_old
            for g, w in zip(got, want):
                assert all(g[k] == w[k] for k in INTS)
                assert all(np.float64(g[k]).tobytes() == np.float64(w[k]).tobytes() for k in DOUBLES)


@pytest.mark.parametrize("both", [False, True])
def test_equal_composition_is_the_flat_null(tata, both):
    """every bin with the same pair counts up to a factor of its own (1, 2, 3, 5 .. 19): each expected is the flat one within
    1e-12 relative.  The pseudocounts are what keeps a multiple from being the same chain -- (k c + 1) / (k n + 4) against
    (c + 1) / (n + 4), a relative 1 / c --, so the counts are of the order 2^50: 1 / c < 1e-15 in each of the K - 1 = 5
    factors and in f, far inside the 1e-12 that is asked, beside the roundings of 20 bins' sums."""
    seqs = tata[(0.1, 1)]
    counts = mp.tables(seqs, 6, 0, 10, 20, both)
    base = np.random.default_rng(7).integers(1000, 5000, 16).astype(np.uint64) << np.uint64(40)
    factors = [1, 2, 3, 5, 7, 11, 13, 17, 19, 4, 6, 8, 9, 10, 12, 14, 15, 16, 18, 1]
    pairs = np.stack([base * np.uint64(f) for f in factors])
    assert int(pairs.max()) * 16 < 2 ** 64
    flat = {(d["key"], d["bin"]): d for d in pk.position_summary(counts, 6, both, 1, 1e9)}
    comp = check_summary(counts, pairs, 6, both, 1, 1e9)
    assert len(comp) > 1000
    seen = 0
    for d in comp:
        f = flat.get((d["key"], d["bin"]))
        if f is not None:      # (the best bin may differ where two bins tie to the last bits)
            seen += 1
            assert abs(d["expected"] - f["expected"]) <= 1e-12 * f["expected"], (d, f)
    assert seen > 1000
    # every share, not only the best bins': q_key[b] against N[b] / Nt
    N = counts.sum(axis=1).astype(np.float64)
    for key in np.flatnonzero(counts.sum(axis=0))[::37].tolist():
        q = pn.shares(counts, pairs, 6, both, key)
        assert np.allclose(q, N / N.sum(), rtol=1e-12, atol=0.0)


def test_constructed_edges():
    K, B = 4, 4
    counts = np.zeros((B, 256), np.uint64)
    counts[:, :] = 3
    key = mp.key_of("ACGT")
    counts[1, key] = 60
    pairs = np.zeros((B, 16), np.uint64)
    pairs[0] = 50
    pairs[1] = 50
    pairs[2] = 50
    # a bin without pairs: weight 0, so its count is over any expectation and the other bins share the whole
    rep = check_summary(counts, pairs, K, False, 1, 1e9)
    q = pn.shares(counts, pairs, K, False, key)
    assert q[3] == 0.0 and abs(sum(q) - 1.0) < 1e-15 and q[0] == q[2] < q[1]     # (bin 1 holds more words)
    by = {d["key"]: d for d in rep}
    assert by[key]["bin"] == 3 and by[key]["expected"] == 0.0 and by[key]["log10_pvalue"] == -np.inf   # 3 words where none can be
    assert by[key]["bins_significant"] == 2                                                             # ... and bin 1
    # a letter that begins no pair: its row of T is 1/4 each, its f is 0
    pairs[:, 12:16] = 0
    ch = pn.chains(pairs)
    assert ch[0][1][3] == [0.25] * 4 and ch[0][0][3] == 0.0 and ch[3] is None
    check_summary(counts, pairs, K, False, 1, 1e9)
    tkey = mp.key_of("TACG")            # begins with T: f = 0 in every bin, G = 0 -- the key is skipped ...
    assert pn.shares(counts, pairs, K, False, tkey) is None
    counts[2, tkey] = 80
    rep = check_summary(counts, pairs, K, False, 1, 1e9)
    assert tkey not in {d["key"] for d in rep} and mp.key_of("ACGT") in {d["key"] for d in rep}
    assert tkey in {d["key"] for d in pk.position_summary(counts, K, False, 1, 1e9)}
    # ... but not on both strands, where its reverse complement CGTA begins with C
    both_counts = counts.copy()
    both_counts[:, [k for k in range(256) if mp.canonical(k, 4) != k]] = 0
    ckey = mp.canonical(tkey, 4)
    both_counts[2, ckey] = 80
    assert pn.shares(both_counts, pairs, K, True, ckey) is not None
    check_summary(both_counts, pairs, K, True, 1, 1e9)
    # no pair anywhere: every key is skipped
    assert check_summary(counts, np.zeros((B, 16), np.uint64), K, False, 1, 1e9) == []


# ---- the gradient scenario -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gradient():
    out = {}
    for seed in (1, 2, 3):
        for frac in (0.0, 0.05):
            seqs = pn.gradient(seed, frac)
            out[(frac, seed)] = (mp.tables(seqs, 6, mp.CENTER, 10, 10, True), pn.pair_tables(seqs, 6, mp.CENTER, 10, 10, True))
    return out


def extreme(key):
    return pn.gc_letters(key, 6) >= 5 or pn.gc_letters(key, 6) <= 1


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_gradient_nothing_planted(gradient, seed):
    """2 000 x 200 bp, G+C 65 % at the centre falling to 35 % at the ends, nothing planted; anchor centre, K 6, S 10, B 10,
    both strands.  Measured through the library on seeds 1, 2, 3: the flat null reports 218 / 245 / 217 words (best log10 E
    -20.39 / -21.45 / -16.90), 216 / 243 / 213 of them with >= 5 or <= 1 of 6 letters G+C; the composition null reports none
    (best log10 E 0.24 / 0.21 / 0.53)."""
    counts, pairs = gradient[(0.0, seed)]
    flat = pk.position_summary(counts, 6, True)
    comp = check_summary(counts, pairs, 6, True)
    best = check_summary(counts, pairs, 6, True, E=100.0)[0]
    n_extreme = sum(extreme(d["key"]) for d in flat)
    print("gradient, nothing planted, seed %d: flat %d words (best log10_E %.2f), %d of them extreme in G+C; composition %d words (best %.2f, %s bin %d)"
          % (seed, len(flat), flat[0]["log10_evalue"], n_extreme, len(comp), best["log10_evalue"], mp.word_string(best["key"], 6), best["bin"]))
    assert len(flat) > 100 and n_extreme >= 0.9 * len(flat)
    assert comp == []


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_gradient_with_the_motif_in_5_percent(gradient, seed):
    """TGACTCA on the plus strand of 5 % at the centre +- 3.  Measured through the library on seeds 1, 2, 3: the composition
    null reports 6 / 5 / 4 words, the first GACTCA / GACTCA / GAGTCA in bin 0 at log10 E -29.58 / -36.23 / -35.14 (the bound
    below: one unit above the weakest); the flat null 240 / 211 / 227 words, 233 / 203 / 223 of them extreme in G+C."""
    counts, pairs = gradient[(0.05, seed)]
    flat = pk.position_summary(counts, 6, True)
    comp = check_summary(counts, pairs, 6, True)
    print("gradient, motif in 5 %%, seed %d: flat %d words, %d extreme in G+C; composition %d words: %s; the first in bin %d at log10_E %.2f"
          % (seed, len(flat), sum(extreme(d["key"]) for d in flat), len(comp), " ".join(mp.word_string(d["key"], 6) for d in comp),
             comp[0]["bin"], comp[0]["log10_evalue"]))
    assert mp.word_string(comp[0]["key"], 6) in ("GACTCA", "GAGTCA") and comp[0]["bin"] == 0
    assert comp[0]["log10_evalue"] <= -28.58
    assert comp[0]["is_head"] == 1
    for d in comp:
        assert pn.shares_a_4mer(mp.word_string(d["key"], 6)), d


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_ramp_from_one_end(seed):
    """G+C rising from 35 % to 65 % along the sequence, anchor start, B = 20, plus strand: the flat null reports 42 / 37 / 37
    words with nothing planted, the composition null none (best log10 E 0.08 / 0.49 / 0.68)"""
    seqs = pn.ramp(seed)
    counts, pairs = mp.tables(seqs, 6, mp.START, 10, 20, False), pn.pair_tables(seqs, 6, mp.START, 10, 20, False)
    flat = pk.position_summary(counts, 6, False)
    best = check_summary(counts, pairs, 6, False, E=100.0)[0]
    print("ramp, seed %d: flat %d words, composition best log10_E %.2f" % (seed, len(flat), best["log10_evalue"]))
    assert len(flat) > 20 and check_summary(counts, pairs, 6, False) == []


# ---- the known cost: the TATA scenario --------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_tata_scenario_pays_part_of_itself_to_the_null(tata, seed):
    """the README's TATA scenario (mp.planted, anchor start, B = 20, both strands) under the composition null: the motif's own
    letters feed its bin's pairs.  Measured through the library on seeds 1, 2, 3: the first line TATAAA bin 6 / TATATA bin 6 /
    TATATA bin 5 still, at log10 E -4.63 / -6.45 / -4.81 (flat: -9.34 / -12.66 / -11.25), 2 / 2 / 3 words instead of 3 / 5 / 6;
    nothing planted: none under either null.  The bound: one unit above the weakest seed."""
    seqs = tata[(0.1, seed)]
    counts, pairs = mp.tables(seqs, 6, mp.START, 10, 20, True), pn.pair_tables(seqs, 6, mp.START, 10, 20, True)
    flat = pk.position_summary(counts, 6, True)
    comp = check_summary(counts, pairs, 6, True)
    top = comp[0]
    print("tata, seed %d: composition %s bin %d log10_E %.2f, %d words; flat log10_E %.2f, %d words"
          % (seed, mp.word_string(top["key"], 6), top["bin"], top["log10_evalue"], len(comp), flat[0]["log10_evalue"], len(flat)))
    assert (mp.word_string(top["key"], 6), top["bin"]) == {1: ("TATAAA", 6), 2: ("TATATA", 6), 3: ("TATATA", 5)}[seed]
    assert (top["key"], top["bin"]) == (flat[0]["key"], flat[0]["bin"])
    assert top["log10_evalue"] <= -3.63 and top["log10_evalue"] > flat[0]["log10_evalue"]
    assert 1 <= len(comp) <= len(flat)
    seqs = tata[(0.0, seed)]
    counts, pairs = mp.tables(seqs, 6, mp.START, 10, 20, True), pn.pair_tables(seqs, 6, mp.START, 10, 20, True)
    assert check_summary(counts, pairs, 6, True) == [] and pk.position_summary(counts, 6, True) == []


# ---- the CLI's flags ---------------------------------------------------------------------------------------------------------
def clean_env():
    return {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PENGK_COMM_TRANSPORT")}


def test_help_lists_the_flag():
    r = subprocess.run([CLI, "-h"], stdout=subprocess.PIPE, env=clean_env(), timeout=60)
    assert r.returncode == 0
    assert b"--positional-null NAME" in r.stdout and b"flat_expected" in r.stdout and b"composition" in r.stdout


@pytest.mark.parametrize("extra,message", [
    (["--positional", "F", "--positional-null", "gc"], b"--positional-null must be flat or composition"),
    (["--positional", "F", "--positional-null", "Composition"], b"--positional-null must be flat or composition"),
    (["--positional", "F", "--positional-null", ""], b"--positional-null must be flat or composition"),
    (["--positional-null", "composition"], b"--positional-null requires --positional"),
    (["--positional-null", "flat"], b"--positional-null requires --positional"),
    (["--positional", "F", "--positional-null"], b"--positional-null"),
], ids=["gc", "capital", "empty", "composition_without_the_flag", "flat_without_the_flag", "no_value"])
def test_bad_arguments_exit_with_4(tmp_path, extra, message):
    args = [str(tmp_path / "p.tsv") if a == "F" else a for a in extra]
    r = subprocess.run([CLI, os.path.join(GOLD, "MafK.fasta"), "-o", str(tmp_path / "o.meme")] + args, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, env=clean_env(), timeout=60)
    assert r.returncode == 4 and message in r.stderr and b"ERROR" in r.stderr, (r.returncode, r.stderr.decode()[-500:])
    assert not (tmp_path / "p.tsv").exists() and not (tmp_path / "o.meme").exists()
