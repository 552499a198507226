"""The shared tile walk of csrc/tile_walk.h -- tile counts, their exclusive sums, a wave's share and its cursor -- held to
the four entries that walk tiles in static shares (the mask plans with it and keeps its own written-out copy of the share
and the walk, which these cases hold to the same behaviour), each against the model it already has: the mask (tests/motif_dust_model.py), the dyad
count (tests/motif_dyads_model.py), the positional count (tests/motif_positional_model.py) and the positional pair table
(tests/positional_null_model.py), bit for bit.  The inputs are small sets built so that sequences WITHOUT a tile -- empty for
the mask, shorter than 3 bases for the dyads, shorter than K for the positional entries -- sit where the two binary searches
and the walk could go wrong: one sequence with one tile (most workgroups of the grid return early), 256, 257 and 513
sequences with tile-less ones at the indices 0, 255, 256, 511, 512 and at the end, 300 tile-less ones in a row so that a
whole group of 256 sums to zero, and nothing but tile-less ones (the total is 0: nothing written, nothing added).  Every
entry is called twice on the same tables: what it adds to doubles, what it writes stays.

At most 600 sequences of at most 200 bases are far fewer tiles than the grid has waves, so there every share is one tile and
the cursor is located, never advanced.  One more input, 25 000 sequences drawn from a small pool with two runs of 300
tile-less ones, gives every wave a share of several tiles that the cursor walks across sequences and across the empty
groups."""
import numpy as np
import pytest

import peng_motif_amd as pk
import motif_dust_model as md
import motif_dyads_model as dy
import motif_erase_model as me
import motif_positional_model as mp
import motif_score_model as ms
import positional_null_model as pn

pytestmark = pytest.mark.gpu

T, G, K, S, B = 20, 20, 6, 10, 20   # the mask's threshold; the dyads' largest gap; the positional word, bin size and bins
POISON = 0xDEADBEEF                 # what the mask's output holds before the call
KINDS = ("one", 256, 257, 513, "gap", "none", "shares")


class Mask:
    less, lo = (0,), 1

    def buffers(self, ctx, lay, fill):
        return [ctx.to_device(np.full(len(lay.valid), POISON, np.uint32)), ctx.to_device(np.full(2, fill, np.uint64))]

    def call(self, ctx, scan, bufs):
        ctx.mask_low_complexity(scan, T, out_valid=bufs[0], masked=bufs[1])

    def want(self, lay, pool, idx):
        """[(array, added to)]: the validity words (written; the layout's spare word is not) and the two counters"""
        pm, _, _ = md.mask_codes(pool, T)
        lost = np.array([int((np.asarray(a) != np.asarray(b)).sum()) for a, b in zip(pool, pm)], np.int64)[idx]
        words = np.full(len(lay.valid), POISON, np.uint32)
        w = me.valid_words([pm[i] for i in idx])
        words[:len(w)] = w
        return [(words, False), (np.array([lost.sum(), (lost > 0).sum()], np.uint64), True)]


class Dyads:
    less, lo = (0, 1, 2), 3

    def buffers(self, ctx, lay, fill):
        return [ctx.to_device(np.full((G + 1, 4096), fill, np.uint64)), ctx.to_device(np.full(64, fill, np.uint64))]

    def call(self, ctx, scan, bufs):
        ctx.dyad_count(scan, G, True, counts=bufs[0], mono=bufs[1])

    def want(self, lay, pool, idx):
        return [(t, True) for t in dy.tables(pool, G, True, weights=np.bincount(idx, minlength=len(pool)))]


class Positional:
    less, lo = tuple(range(K)), K

    def buffers(self, ctx, lay, fill):
        return [ctx.to_device(np.full((B, 4 ** K), fill, np.uint64))]

    def call(self, ctx, scan, bufs):
        ctx.position_count(scan, K, mp.CENTER, S, B, True, counts=bufs[0])

    def want(self, lay, pool, idx):
        return [(mp.tables(pool, K, mp.CENTER, S, B, True, weights=np.bincount(idx, minlength=len(pool))), True)]


class Pairs(Positional):
    def buffers(self, ctx, lay, fill):
        return [ctx.to_device(np.full((B, 16), fill, np.uint64))]

    def call(self, ctx, scan, bufs):
        ctx.position_pairs(scan, K, mp.END, S, B, True, pairs=bufs[0])

    def want(self, lay, pool, idx):
        return [(pn.pair_tables(pool, K, mp.END, S, B, True, weights=np.bincount(idx, minlength=len(pool))), True)]


USERS = dict(mask=Mask(), dyads=Dyads(), positional=Positional(), pairs=Pairs())


def sequences(rng, lengths):
    """random letters; a poly-A run in every third one that has room (something for the mask to take), an invalid base in
    every fifth"""
    out = []
    for n, L in enumerate(lengths):
        c = rng.integers(1, 5, int(L)).astype(np.uint8)
        if L >= 40 and n % 3 == 0:
            c[5:35] = 1
        if L and n % 5 == 0:
            c[rng.integers(0, L)] = 0
        out.append(c)
    return out


def make_input(kind, user, rng):
    """(pool, idx): the input is [pool[i] for i in idx]"""
    less = lambda n: [user.less[i % len(user.less)] for i in range(n)]
    tiled = lambda n: [200, user.lo, 200] + list(rng.integers(user.lo, 201, n - 3))   # (both ends of the range among them)
    if kind == "shares":
        pool = sequences(rng, less(len(user.less)) + tiled(48))
        n_less = len(user.less)
        with_tile = lambda n: rng.integers(n_less, len(pool), n)
        without = np.arange(300) % n_less
        # (the mask has one tile a sequence here: 5000 and 10001 tiles in front of the runs, which no share size divides both)
        return pool, np.concatenate([with_tile(5000), without, with_tile(5001), without, with_tile(14399)])
    if kind == "one":
        lengths = [40]
    elif kind == "gap":
        lengths = tiled(250) + less(300) + tiled(50)
    elif kind == "none":
        lengths = less(300)
    else:
        lengths = tiled(kind)
        for i in (0, 255, 256, 511, 512, kind - 1):
            if i < kind:
                lengths[i] = user.less[i % len(user.less)]
    pool = sequences(rng, lengths)
    return pool, np.arange(len(pool))


@pytest.fixture(scope="module")
def ctx():
    c = pk.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("kind", KINDS, ids=str)
@pytest.mark.parametrize("name", list(USERS))
def test_tiles_are_walked_once_each(ctx, name, kind):
    user = USERS[name]
    pool, idx = make_input(kind, user, np.random.default_rng(KINDS.index(kind)))
    seqs = [pool[i] for i in idx]
    assert len(seqs) <= 600 and max(len(c) for c in seqs) <= 200 or kind == "shares"
    lay = pk.ScanLayout(*ms.flatten(seqs))
    scan = ctx.upload_scan(lay)
    want = user.want(lay, pool, idx)
    if kind == "none":
        assert all(not w.any() for w, added in want if added)
    else:
        assert all(w.any() for w, _ in want)
    fill = 7 if kind == "none" else 0   # (a total of 0 tiles: the tables keep what they held)
    bufs = user.buffers(ctx, lay, fill)
    for calls in (1, 2):
        user.call(ctx, scan, bufs)
        for k, (buf, (w, added)) in enumerate(zip(bufs, want)):
            got, exp = buf.to_host(), (fill + calls * w if added else w)
            bad = np.argwhere(got != exp)
            assert len(bad) == 0, "%s, %s, call %d, buffer %d at %s: %d, the model %d (%d entries differ)" % (
                name, kind, calls, k, tuple(bad[0]), got[tuple(bad[0])], exp[tuple(bad[0])], len(bad))
