"""pengk_motif_enrich at the sizes the per-feature module only sums over (the comparison README asks of a new scan
kernel): a million short sequences through the batched model of tests/scan_batch_model.py -- more than one trip of the
grid-stride loop, a ragged last one, every workgroup flushing its private bins -- and sequences of 200 000 bases."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import peng_motif_amd as pk
import motif_enrich_model as me
import motif_score_model as ms
import scan_batch_model as sbm
from test_gpu_motif_enrich import assert_equal, run, threshold_at
from test_gpu_motif_qvalue import random_S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = pk.Context(0)
    yield c
    c.close()


def test_a_million_short_sequences(ctx):
    n, L = 1_000_003, 20
    assert n > ctx.info("num_cu") * 8 * 256 and n % 256  # more than one trip of the grid-stride loop, a ragged last one
    rng = np.random.default_rng(606)
    codes = rng.integers(1, 5, (n, L), dtype=np.uint8)
    codes[rng.integers(0, 100, (n, L), dtype=np.uint8) == 0] = 0
    S = [random_S(rng, 4), random_S(rng, 10)]
    thr = [threshold_at(S[0], 0.02), int(S[1].min(axis=1).sum())]
    scan = ctx.upload_scan(pk.ScanLayout(codes.reshape(-1), np.arange(n + 1, dtype=np.int64) * L))
    got = run(ctx, scan, S, True, thr)
    with ThreadPoolExecutor(2) as ex:  # (numpy releases the GIL in its inner loops)
        best = list(ex.map(lambda m: sbm.best_scores(codes, S[m], True), range(2)))
    want = [me.histogram(best[m], thr[m], me.score_hi(S[m])) for m in range(2)]
    assert 10 ** 5 < int(want[0][0].sum()) < want[0][1] <= n and int(want[1][0].sum()) == want[1][1] < n  # (1 % invalid bases)
    assert_equal(got, ([h for h, _ in want], [s for _, s in want]))


def test_long_sequences(ctx):
    rng = np.random.default_rng(4242)
    seqs = [rng.integers(1, 5, L).astype(np.uint8) for L in [65535, 65536, 65537, 200000, 300]]
    seqs[2][65530:65546] = 0
    S = [random_S(rng, w) for w in [10, 33]]
    seqs[3][-10:] = np.argmax(S[0], axis=1) + 1  # the top bin, from the last window of the longest sequence
    thr = [threshold_at(s, 0.04) for s in S]
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    packed = me.Packed(seqs)
    want = [me.histogram(me.best_scores(packed, s, True), t, me.score_hi(s)) for s, t in zip(S, thr)]
    assert int(want[0][0][-1]) >= 1 and want[0][1] == want[1][1] == 5
    assert_equal(run(ctx, scan, S, True, thr), ([h for h, _ in want], [s for _, s in want]))
