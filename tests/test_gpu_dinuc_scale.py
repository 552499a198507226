"""The first-order scan (pengk_motif_scan_dinuc) value by value against the vectorised model of tests/motif_dinuc_model.py at
the sizes tests/test_gpu_motif_dinuc.py only samples: a sequence of many words, more motifs than one LDS group holds, and
many more sequences than one pass of the grid takes.  (The scale cases of the other scan kernels are in
tests/test_gpu_scan_scale.py.)"""
import numpy as np
import pytest

import peng_motif_amd as pk
import motif_dinuc_model as md
from test_motif_dinuc_cpu import random_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = pk.Context(0)
    yield c
    c.close()


def upload(ctx, codes):
    n, L = codes.shape
    return ctx.upload_scan(pk.ScanLayout(codes.reshape(-1), np.arange(n + 1, dtype=np.int64) * L))


def scan_both_ways(ctx, scan, models, widths, both, **kw):
    return ctx.motif_scan_dinuc(scan, [m[0] for m in models], [m[1] for m in models], widths, both, **kw).to_host()


@pytest.mark.parametrize("both", [True, False], ids=["both", "plus"])
def test_one_long_sequence_with_n_runs(ctx, both):
    rng = np.random.default_rng(301 + both)
    L = 200_000
    codes = rng.integers(1, 5, (1, L)).astype(np.uint8)
    for a in rng.integers(0, L, 40):
        codes[0, a:a + int(rng.integers(1, 200))] = 0
    codes[0, :3] = 0
    codes[0, -70:-5] = 0  # (the last windows of the widest motif are not valid ones)
    widths = [1, 5, 16, 17, 33, 64]
    models = [random_model(rng, w) for w in widths]
    got = scan_both_ways(ctx, upload(ctx, codes), models, widths, both)
    want = np.stack([md.best_scores_batch(codes, S0, D, both) for S0, D in models]).astype(np.int32)
    assert got.tobytes() == want.tobytes()
    assert np.all(got != pk.SCORE_SENTINEL)


def test_a_hundred_motifs_in_several_lds_groups(ctx):
    """a motif of width w takes 2 ceil(w / 4) x 272 of a group's 10240 table entries with both strands: widths 4..24 put
    three to eighteen motifs into a group, and the hundred into more than ten groups with boundaries all along the run"""
    rng = np.random.default_rng(311)
    n, L = 1500, 50
    codes = rng.integers(1, 5, (n, L)).astype(np.uint8)
    codes[rng.random((n, L)) < 0.004] = 0
    widths = rng.integers(4, 25, 100).tolist()
    models = [random_model(rng, w) for w in widths]
    got = scan_both_ways(ctx, upload(ctx, codes), models, widths, True)
    want = np.stack([md.best_scores_batch(codes, S0, D, True) for S0, D in models]).astype(np.int32)
    assert got.tobytes() == want.tobytes()
    groups, used = 1, 0
    for w in widths:
        need = 2 * ((w + 3) // 4) * 272
        if used + need > 40 * 256:
            groups, used = groups + 1, 0
        used += need
    assert groups > 10


def test_two_hundred_thousand_short_sequences(ctx):
    rng = np.random.default_rng(321)
    n, L = 200_000, 40
    codes = rng.integers(1, 5, (n, L)).astype(np.uint8)
    codes[rng.random((n, L)) < 0.002] = 0
    codes[::997, 5::8] = 0  # (no window of nine bases)
    widths = [9, 13]
    models = [random_model(rng, w) for w in widths]
    scan = upload(ctx, codes)
    got = scan_both_ways(ctx, scan, models, widths, True)
    want = np.stack([md.best_scores_batch(codes, S0, D, True) for S0, D in models]).astype(np.int32)
    assert got.tobytes() == want.tobytes()
    assert n // 997 <= np.count_nonzero(got[0] == pk.SCORE_SENTINEL) < n // 100
    # the sampled sequences' layout: no validity words, every letter a base
    got = scan_both_ways(ctx, scan, models[:1], widths[:1], False, all_valid=True)
    want = md.best_scores_batch(np.where(codes == 0, 1, codes), *models[0], False).astype(np.int32)
    assert got[0].tobytes() == want.tobytes()
