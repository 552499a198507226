"""The batched model of tests/scan_batch_model.py against the per-sequence models it restates
(motif_score_model.best_scores, motif_sites_model.all_sites, motif_centrality_model.best_sites,
motif_refine_model.site_profile), array for array, on a few hundred small equal-length sets and on mixed-length ones.
No GPU: this is what makes the large comparisons of tests/test_gpu_scan_scale.py trustworthy."""
import numpy as np
import pytest

import motif_centrality_model as mc
import motif_refine_model as mr
import motif_score_model as ms
import motif_sites_model as mst
import scan_batch_model as sbm

WIDTHS = [1, 4, 5, 13, 64]
KINDS = ["random", "zero", "two_valued"]


def motif(rng, w, kind):
    if kind == "zero":
        return np.zeros((w, 4), np.int32)
    if kind == "two_valued":
        return rng.integers(0, 2, (w, 4)).astype(np.int32)
    S = rng.integers(-300, 301, (w, 4)).astype(np.int32)
    S[rng.random((w, 4)) < 0.05] = -2000
    S[rng.random((w, 4)) < 0.02] = 2000
    return S


def equal_length_set(rng, n, L):
    """n sequences of L bases: some clean, some with N runs, one without any valid base, one with every third base N"""
    codes = rng.integers(1, 5, (n, L)).astype(np.uint8)
    for i in range(n):
        for _ in range(int(rng.integers(0, 3)) if i % 3 else 0):  # (every third sequence stays clean)
            if L:
                a = int(rng.integers(0, L))
                codes[i, a:a + int(rng.integers(1, 20))] = 0
    if n > 2:
        codes[1] = 0
        codes[2, ::3] = 0
    return codes


def lengths_for(w):
    return sorted({1, max(w - 1, 1), w, 31, 32, 33, 64, 65, 97})


def a_threshold(codes, S, both, q):
    sc, good = sbm.window_scores(codes, S, both)
    v = sc[:, good]
    return int(np.percentile(v, q)) if v.size else 0


def check_set(codes, S, both, m, seq0, flanks=(0, 3, 40)):
    seqs = list(codes)
    w = len(S)
    r = sbm.scan(codes, S, both, thr=a_threshold(codes, S, both, 60), m=m, seq0=seq0)
    assert np.array_equal(r["best"] if both else r["best_plus"], ms.best_scores(seqs, S, both))
    assert np.array_equal(r["best_plus"], ms.best_scores(seqs, S, False))
    assert np.array_equal(sbm.best_scores(codes, S, both), ms.best_scores(seqs, S, both))
    for q in [60, 99]:
        t = a_threshold(codes, S, both, q)
        want = mst.all_sites(seqs, [S, S], [t, t + 1], both)
        got = sbm.all_sites(codes, [S, S], [t, t + 1], both)
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
        cnt = sbm.site_counts(codes, S, t, both)
        assert np.array_equal(cnt, np.bincount(want["seq"][want["motif"] == 0].astype(np.int64), minlength=len(seqs)))
    wb, ws = mc.best_sites(seqs, S, both, m, seq0)
    gb, gs = sbm.best_sites(codes, S, both, m, seq0)
    assert gb.dtype == wb.dtype and gs.dtype == ws.dtype
    assert gb.tobytes() == wb.tobytes() and gs.tobytes() == ws.tobytes()
    assert r["best_site"].tobytes() == wb.tobytes() and r["site"].tobytes() == ws.tobytes()
    ok = wb[wb > ms.SENTINEL]
    t = int(np.percentile(ok, 30)) if len(ok) else 0
    for flank in flanks:
        want = mr.site_profile(seqs, wb, ws, w, t, flank)
        got = sbm.site_profile(codes, wb, ws, w, t, flank)
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    return len(ok)


@pytest.mark.parametrize("both", [True, False], ids=["both", "plus"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w", WIDTHS)
def test_equal_length_sets_equal_the_per_sequence_models(w, kind, both):
    rng = np.random.default_rng(1000 * w + 10 * KINDS.index(kind) + both)
    scored = 0
    for k, L in enumerate(lengths_for(w)):  # 5 widths x 3 kinds x 2 strand modes x 7..9 lengths: 250 sets
        codes = equal_length_set(rng, 9, L)
        scored += check_set(codes, motif(rng, w, kind), both, m=k, seq0=[0, 5, 2 ** 40 + 12345][k % 3])
    assert scored > 10


def test_ties_are_broken_by_the_key_not_by_the_scan_order():
    rng = np.random.default_rng(7)
    codes = rng.integers(1, 5, (200, 33)).astype(np.uint8)
    _, site = sbm.best_sites(codes, np.zeros((5, 4), np.int32), True, 3, seq0=11)
    assert np.count_nonzero(site > 1) > 150 and len(np.unique(site)) > 40
    assert site.tobytes() == mc.best_sites(list(codes), np.zeros((5, 4), np.int32), True, 3, 11)[1].tobytes()


def test_chunks_change_nothing(monkeypatch):
    rng = np.random.default_rng(8)
    codes = equal_length_set(rng, 57, 40)
    S = motif(rng, 7, "two_valued")
    whole = sbm.scan(codes, S, True, thr=4, m=2, seq0=9)
    monkeypatch.setattr(sbm, "CHUNK_CELLS", 40 * 5)  # 5 sequences a chunk: 12 chunks, the last one short
    parts = sbm.scan(codes, S, True, thr=4, m=2, seq0=9)
    assert len(whole["sites"]) > 100 and sorted(whole) == sorted(parts)
    for k in whole:
        assert whole[k].tobytes() == parts[k].tobytes(), k
    check_set(codes, S, True, 2, 9)


@pytest.mark.parametrize("both", [True, False], ids=["both", "plus"])
def test_a_mixed_length_set_equals_the_per_sequence_models(both):
    rng = np.random.default_rng(9 + both)
    lens = np.array([0, 3, 20, 31, 32, 33, 47, 65])[rng.integers(0, 8, 150)]
    seqs = [equal_length_set(rng, 4, L)[int(rng.integers(0, 4))] for L in lens]  # clean, all N, every third N, N runs
    seqs[17][:] = 0
    codes, offs = ms.flatten(seqs)
    seq0 = 2 ** 33 + 77
    for m, (w, kind) in enumerate([(4, "random"), (10, "random"), (6, "zero"), (13, "two_valued"), (60, "random")]):
        S = motif(rng, w, kind)
        t = int(np.percentile(ms.best_scores(seqs, S, both)[lens >= w], 20))
        r = sbm.scan_mixed(codes, offs, S, both, thr=t, m=m, seq0=seq0)
        assert np.array_equal(r["best"] if both else r["best_plus"], ms.best_scores(seqs, S, both))
        want = mst.all_sites(seqs, [S], [t], both)
        assert len(want) > (20 if w < 60 else 0)
        for f in ["seq", "pos", "strand", "score"]:
            assert np.array_equal(r["sites"][f].astype(np.int64), want[f].astype(np.int64)), f
        assert np.array_equal(r["counts"], np.bincount(want["seq"].astype(np.int64), minlength=len(seqs)))
        wb, ws = mc.best_sites(seqs, S, both, m, seq0)
        assert r["best_site"].tobytes() == wb.tobytes() and r["site"].tobytes() == ws.tobytes()
        for flank in [0, 3, 40]:
            got = sbm.site_profile_mixed(codes, offs, wb, ws, w, t, flank)
            assert got.tobytes() == mr.site_profile(seqs, wb, ws, w, t, flank).tobytes()
            assert got.any()
