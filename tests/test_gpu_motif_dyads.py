"""--dyads on the device (include/pengk.h, "spaced dyads"): pengk_dyad_count against the numpy model of
tests/motif_dyads_model.py, both tables bit for bit -- at the lengths where a span, a word or a tile ends, with one
invalid base at every position in turn, without input validity, on one strand and on both, on one hot bin, across the
tiles and workgroups of 100 000 sequences, in two calls, on a subset of the offset arrays, and the argument errors."""
import numpy as np
import pytest

import peng_motif_amd as pk
import motif_dyads_model as dy
import motif_score_model as ms

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = pk.Context(0)
    yield c
    c.close()


def check_tables(ctx, seqs, G, both, all_valid=False, want=None):
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    counts, mono = ctx.dyad_count(scan, G, both, all_valid=all_valid)
    wc, wm = want if want is not None else dy.tables(seqs, G, both)
    gc, gm = counts.to_host(), mono.to_host()
    assert np.array_equal(gm, wm), "triplets: first difference at %d" % np.flatnonzero(gm != wm)[0]
    bad = np.argwhere(gc != wc)
    assert len(bad) == 0, "gap %d key %d: %d, the model %d (%d entries differ)" % (bad[0][0], bad[0][1], gc[tuple(bad[0])], wc[tuple(bad[0])], len(bad))
    return int(wc.sum())


def test_symbol():
    assert hasattr(pk.lib(), "pengk_dyad_count")


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("G", [0, 1, 20, 26])
def test_lengths_at_the_edges(ctx, G, both):
    lengths = dy.edge_lengths(G)
    seqs = dy.random_sequences(10 + G, lengths)
    assert check_tables(ctx, seqs, G, both) > 0
    check_tables(ctx, seqs, G, both, all_valid=True)
    for c in seqs[1:]:   # every one alone (but the empty one: a set without a word)
        check_tables(ctx, [c], G, both)


@pytest.mark.parametrize("both", [False, True])
def test_one_invalid_base_at_every_position(ctx, both):
    base = dy.random_sequences(21, [40])[0]
    seqs = []
    for p in range(40):
        c = base.copy()
        c[p] = 0
        seqs.append(c)
    for G in (0, 20, 26):
        check_tables(ctx, seqs, G, both)
    for c in seqs[::7]:
        check_tables(ctx, [c], 20, both)


def test_a_dyad_that_is_its_own_reverse_complement(ctx):
    c = dy.codes_of("CGG" + "ACGTACGTACG" + "CCG")
    check_tables(ctx, [c], 11, True, all_valid=True)
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten([c])))
    counts, mono = ctx.dyad_count(scan, 11, True)
    h = counts.to_host()
    assert h[11, dy.key_of("CGG", "CCG")] == 1 and h[11].sum() == 1 and mono.to_host().sum() == 15
    counts, _ = ctx.dyad_count(scan, 11, False)
    assert counts.to_host()[11, dy.key_of("CGG", "CCG")] == 1
    check_tables(ctx, [dy.codes_of("ACGT" * 16)], 26, True)   # (ACGT is its own reverse complement: so are its dyads at the gaps 4k + 2)


@pytest.mark.parametrize("both", [False, True])
def test_70000_bases_of_one_letter(ctx, both):
    """every lane bumps one bin"""
    c = dy.codes_of("A" * 70000)
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten([c])))
    counts, mono = ctx.dyad_count(scan, 20, both, all_valid=True)
    h = counts.to_host()
    for g in range(21):
        assert h[g, 0] == 70000 - 5 - g and h[g].sum() == h[g, 0]
    assert mono.to_host()[0] == 69998
    check_tables(ctx, [dy.codes_of("T" * 70000)], 26, both)   # (TTT n TTT folds onto AAA n AAA on both strands)


@pytest.mark.parametrize("both", [False, True])
def test_70000_random_bases(ctx, both):
    c = dy.random_sequences(22, [70000])[0]
    check_tables(ctx, [c], 20, both, all_valid=True)
    c[np.random.default_rng(23).integers(0, 70000, 50)] = 0
    check_tables(ctx, [c], 26, both)


@pytest.fixture(scope="module")
def many():
    seqs, idx, pool = dy.many_sequences()
    return seqs, idx, pool


def pool_tables(pool, idx, G, both):
    return dy.tables(pool, G, both, weights=np.bincount(idx, minlength=len(pool)))


@pytest.mark.parametrize("both", [False, True])
def test_100000_sequences(ctx, many, both):
    seqs, idx, pool = many
    assert len(seqs) == 100000 and {len(s) for s in seqs} == set(range(301))
    check_tables(ctx, seqs, 20, both, want=pool_tables(pool, idx, 20, both))


@pytest.fixture(scope="module")
def many_on_device(ctx, many):
    seqs, idx, pool = many
    lay = pk.ScanLayout(*ms.flatten(seqs))
    return lay, ctx.to_device(lay.words), ctx.to_device(lay.valid), pool_tables(pool, idx, 26, True)


@pytest.mark.parametrize("cut", [1, 255, 256, 257, 50001])
def test_two_calls_give_the_tables_of_one(ctx, many_on_device, cut):
    lay, words, valid, (wc, wm) = many_on_device
    n = len(lay.lens)
    counts = ctx.to_device(np.zeros((27, 4096), np.uint64))
    mono = ctx.to_device(np.zeros(64, np.uint64))
    for a, b in ((0, cut), (cut, n)):
        part = (words, valid, ctx.to_device(lay.offs[a:b]), ctx.to_device(lay.lens[a:b]), b - a)
        ctx.dyad_count(part, 26, True, counts=counts, mono=mono)
    assert np.array_equal(counts.to_host(), wc) and np.array_equal(mono.to_host(), wm)


def test_a_subset_that_is_not_contiguous(ctx, many, many_on_device):
    seqs, idx, pool = many
    lay, words, valid, _ = many_on_device
    pick = np.flatnonzero(np.random.default_rng(24).random(len(seqs)) < 0.3)[::-1].copy()   # (and in another order)
    part = (words, valid, ctx.to_device(lay.offs[pick]), ctx.to_device(lay.lens[pick]), len(pick))
    counts, mono = ctx.dyad_count(part, 20, False)
    wc, wm = pool_tables(pool, idx[pick], 20, False)
    assert np.array_equal(counts.to_host(), wc) and np.array_equal(mono.to_host(), wm)


def test_no_sequence_and_argument_errors(ctx):
    seqs = [dy.codes_of("A" * 40)]
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    counts = ctx.to_device(np.full((21, 4096), 7, np.uint64))
    mono = ctx.to_device(np.full(64, 9, np.uint64))
    ctx.dyad_count(scan, 20, True, counts=counts, mono=mono, n_seq=0)
    assert (counts.to_host() == 7).all() and (mono.to_host() == 9).all()
    ctx.dyad_count(scan, 20, True, counts=counts, mono=mono)   # added to, not written
    h = counts.to_host()
    assert h[0, 0] == 7 + 35 and h[20, 0] == 7 + 15 and h.sum() == 7 * 21 * 4096 + sum(35 - g for g in range(21))
    assert mono.to_host()[0] == 9 + 38
    for G in (-1, 27, 100):
        with pytest.raises(pk.PengkError) as e:
            ctx.dyad_count(scan, G, True)
        assert e.value.code == pk.ERR_ARG
    for both in (2, -1):
        with pytest.raises(pk.PengkError) as e:
            ctx.dyad_count(scan, 20, both)
        assert e.value.code == pk.ERR_ARG
    with pytest.raises(pk.PengkError) as e:
        ctx.dyad_count(scan, 20, True, n_seq=1 << 32)
    assert e.value.code == pk.ERR_ARG
