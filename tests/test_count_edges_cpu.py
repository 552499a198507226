"""The constructed count inputs of tests/count_edges_model.py, checked where no GPU is needed: the sparse reference
against the oracle, every class against what it is built to hold, every re-split item list against the packer's, and
the host packer's figures on every class.  tests/test_gpu_count_edges.py runs the same inputs through csrc/count.hip."""
import numpy as np
import pytest

import count_edges_model as cm
import peng_motif_amd as pk
from oracle import oracle as po

ALL_W = cm.WS + (14,)
CLS = list(cm.CLASSES)


def parts(cls, W):
    return list(zip(cm.CLASSES[cls](W), cm.packed(cls, W)))


def per_sequence(part, W, both):
    """(suppressed windows, start of the last suppressed window or -1) of every sequence, by the sparse reference"""
    kept, pos = cm.sparse_count_arrays(part["codes"], part["offs"], W, both)[3:5]
    offs = part["offs"]
    s = np.searchsorted(offs, pos, "right") - 1
    n = len(offs) - 1
    sup = np.bincount(s[~kept], minlength=n)
    last = np.full(n, -1, np.int64)
    last[s[~kept]] = (pos - offs[s])[~kept]  # ascending positions: the last write wins
    return sup, last


def items_of(part, p, si):
    """indices of the items whose windows lie in sequence si"""
    ws = cm.item_fields(p.items)[0] - pk.FRONT_PAD_BASES
    return np.flatnonzero((ws >= part["offs"][si]) & (ws < part["offs"][si + 1]))


@pytest.mark.parametrize("W", cm.WS)
@pytest.mark.parametrize("cls", CLS)
def test_sparse_reference_equals_the_oracle(cls, W):
    for part, p in parts(cls, W):
        for both in (False, True):
            want, ltot = po.count(part["codes"], part["offs"], W, both)
            got, lt = cm.sparse_count(part["codes"], part["offs"], W, both)
            assert lt == ltot, (part["name"], both)
            if both:
                x = np.fromiter(got.keys(), np.int64, len(got))
                assert np.all(x <= cm.revcomp_ids(x, W)), "canonical ids only"
            assert np.array_equal(cm.dense(got, W, both), want), (part["name"], both)
            # the same count from the packed stream and the packer's items
            assert cm.replay_count(p.words, p.items, W, both) == (got, lt), (part["name"], both)


@pytest.mark.parametrize("W", ALL_W)
@pytest.mark.parametrize("cls", CLS)
def test_packer_figures_hold_on_every_class(cls, W):
    for part, p in parts(cls, W):
        got, lt = cm.sparse_count(part["codes"], part["offs"], W, False)
        assert p.n_windows == lt, part["name"]
        assert p.max_bin_bound >= max(got.values(), default=0), part["name"]
        assert np.array_equal(p.bg_counts, po.bg_counts(part["codes"], part["offs"], 2)), part["name"]
        if W <= 12:
            assert p.max_bin_bound >= int(po.count(part["codes"], part["offs"], W, True)[0].max()), part["name"]


@pytest.mark.parametrize("W", ALL_W)
@pytest.mark.parametrize("cls", CLS)
def test_every_resplit_replays_to_the_packers_windows(cls, W):
    for part, p in parts(cls, W):
        pos, run = cm.replay_windows(p.items)
        for name, items in cm.resplits(p.items):
            ws, nw, cont = cm.item_fields(items)
            q, r = cm.replay_windows(items)  # (asserts nw in 1 .. 65535 and that continuing items continue)
            assert np.array_equal(q, pos) and np.array_equal(r, run), (part["name"], name)
            if name.startswith("every"):
                c = int(name.split()[1])
                assert nw.max(initial=0) <= c and (c > 1 or len(items) == len(pos))
        whole = cm.item_fields(cm.resplit(p.items))
        runs = cm.item_runs(p.items)[1]
        assert int((whole[2] == 0).sum()) == len(runs) and len(whole[0]) == int(((runs + cm.NW_MAX - 1) // cm.NW_MAX).sum())


@pytest.mark.parametrize("W", ALL_W)
def test_item_lengths_holds_its_class(W):
    (a, pa), (b, pb), (c, pc) = parts("item_lengths", W)
    for part, p, M in ((a, pa, 64), (b, pb, 256), (c, pc, cm.NW_MAX)):
        assert p.all_whole == 1
        ws, nw, cont = cm.item_fields(p.items)
        assert cm.item_runs(p.items)[1].tolist() == list(part["windows"])  # one run per sequence, as long as listed
        assert nw.max() == M
        have = set(nw.tolist())
        if M < cm.NW_MAX:
            assert have >= set(cm.LENGTHS + (M - 1, M)), sorted(have)
            # M + 1, 2M, 2M + 1 windows: M | 1, M | M, M | M | 1
            k = part["windows"].index(2 * M + 1)
            first = int(np.flatnonzero(cont == 0)[k])
            assert nw[first:first + 3].tolist() == [M, M, 1] and cont[first:first + 3].tolist() == [0, 1, 1]
        else:
            assert have >= {65534, 65535, 1, 2, 140000 - 2 * 65535}
    # the copies carry a repeat on every cut: the item behind it cannot certify its ring
    for part, p in ((a, pa), (b, pb), (c, pc)):
        d = cm.deferral_model(p.words, p.items, W, False)
        half = (len(part["offs"]) - 1) // 2
        cont = cm.item_fields(p.items)[2]
        for si in range(half, 2 * half):
            it = items_of(part, p, si)
            assert d[it][cont[it] == 1].all(), (part["name"], si)


@pytest.mark.parametrize("W", ALL_W)
def test_alignment_holds_its_class(W):
    (part, p), = parts("alignment", W)
    ws, nw, cont = cm.item_fields(p.items)
    heads = np.flatnonzero(cont == 0)
    run_nw = dict(zip(ws[heads].tolist(), cm.item_runs(p.items)[1].tolist()))
    seen = {}
    for n, off in part["targets"]:
        assert run_nw[off] == n  # a run starts there and is n windows long
        seen.setdefault(n, set()).add(off % 32)
    assert set(seen) == set(cm.LENGTHS + (63, 64, 65, 128, 129))
    assert all(v == set(range(32)) for v in seen.values())
    assert {n % 16 for n in seen} >= {0, 1, 2, 15}
    lens = np.diff(part["offs"])
    lo = max(10, W)
    assert set(lens[0::2].tolist()) == set(range(lo, lo + 32)) and p.all_whole == 1


@pytest.mark.parametrize("W", ALL_W)
def test_periods_holds_its_class(W):
    (part, p), = parts("periods", W)
    sup, _ = per_sequence(part, W, False)
    sup_b, _ = per_sequence(part, W, True)
    lens = np.diff(part["offs"])
    seen = set()
    for si, kind, period in part["alone"]:
        assert lens[si] >= 6 * W and lens[si] - W + 1 > 64  # several items at M = 64
        unit = part["codes"][part["offs"][si]:part["offs"][si] + period]
        assert np.array_equal(part["codes"][part["offs"][si]:part["offs"][si + 1]], cm.tile(unit, lens[si]))
        if kind == "random":
            seen.add(period)
            assert cm.primitive(unit)
            assert (sup[si] > 0) == (period < W), (period, sup[si])  # from the reference, not assumed
            if period < W:  # the copy in random flanks (which may hold a chance twin of their own at any period)
                assert sup[si - 1] > 0
        elif kind.startswith("rc-periodic"):
            # the reverse complement of the repeat is a shift of the repeat: twins at odd distances under both strands
            assert sup_b[si] >= sup[si] and (sup_b[si] > 0 or period >= W)
        else:
            core = unit[:period - period % 2]
            assert np.array_equal(core, cm.revcomp_codes(core))
    assert seen == set(range(1, W + 3))
    hair = part["codes"][part["offs"][-2]:]
    assert len(hair) == 4 * W + 4 and np.array_equal(hair[:2 * W], cm.revcomp_codes(hair[-2 * W:]))
    if W >= 4:  # the arms are each other's twins, at even distances: only both strands suppress
        assert sup_b[-1] > sup[-1] == 0


@pytest.mark.parametrize("W", ALL_W)
def test_prologue_edge_holds_its_class(W):
    (part, p), = parts("prologue_edge", W)
    P = cm.prologue_bases(W)
    _, last = per_sequence(part, W, False)
    assert np.all(np.diff(part["offs"]) == 400)
    want = {(B, o) for B in range(64, 400 - W + 1, 64) for o in (-1, 0, 1)}  # every item boundary of a 400-base sequence
    assert len(part["exact"]) == len(want) * len(part["repeats"]) and {(B, o) for _, B, o in part["exact"]} == want
    for si, B, o in part["exact"]:
        assert B % 64 == 0 and last[si] == B - (P - W + 1) + o, (si, B, o, last[si])
    assert len(part["shifted"]) == (2 * P + 2) * len(part["repeats"])
    cont = cm.item_fields(p.items)[2]
    for both in (False, True):
        d = cm.deferral_model(p.words, p.items, W, both)
        for a, e in part["repeats"]:
            it = np.concatenate([items_of(part, p, si) for si in range(a, e)])
            it = it[cont[it] == 1]
            assert d[it].any() and not d[it].all(), (both, a, e)
        # the shifted series crosses from "not deferred" to "deferred" and back at item 2 (window 128) of its sequences
        for a, e in part["repeats"]:
            v = [bool(d[items_of(part, p, si)[2]]) for si in part["shifted"] if a <= si < e]
            assert True in v and False in v, (both, v)


@pytest.mark.parametrize("W", ALL_W)
def test_long_fixup_holds_its_class(W):
    (part, p), = parts("long_fixup", W)
    offs = part["offs"]
    assert np.all(np.diff(offs) == 20000) and len(part["cert"]) == (1 if W == 2 else 2)
    cont = cm.item_fields(p.items)[2]
    for both in (False, True):
        d = cm.deferral_model(p.words, p.items, W, both)
        for si in range(len(part["cert"])):  # the plain repeats: every continuing item is deferred ...
            it = items_of(part, p, si)
            assert len(it) == (20000 - W + 1 + 63) // 64 and d[it[1:]].all() and not d[it[0]]
        # ... and the fix-up of the last one reaches the head of the run without ever seeing 2(W-1) clean windows
        f = cm.fixup_model(p.words, p.items, int(items_of(part, p, 0)[-1]), W, both)
        assert f["at_head"] and len(f["levels"]) >= 5 and all(c < 2 * (W - 1) for _, c in f["levels"][:-1])
        for (fail, succ), clean in zip(part["cert"], part["clean"]):
            verdict = []
            for si in (fail, succ):
                q = pk.Packed(part["codes"][offs[si]:offs[si + 1]], np.array([0, 20000], np.int64), W, 64)
                it = cm._cert_item(q)
                assert cm.deferral_model(q.words, q.items, W, both)[it]
                verdict.append(cm.fixup_model(q.words, q.items, it, W, both))
            bad, good = verdict
            # certification just fails and just succeeds: one clean window short, and exactly enough
            assert bad["at_head"] and not good["at_head"], (both, bad, good)
            assert (max(c for _, c in bad["levels"][:-1]), good["max_clean"]) == clean, (both, bad, good)
    # one clean window short, and exactly enough -- but for the two repeats that cannot be cut that finely
    nearest = {2: [(1, 3)], 4: [(5, 6), (3, 7)]}
    assert part["clean"] == nearest.get(W, [(2 * (W - 1) - 1, 2 * (W - 1))] * 2)


@pytest.mark.parametrize("W", ALL_W)
def test_runs_and_N_holds_its_class(W):
    (part, p), (none, pn) = parts("runs_and_N", W)
    assert p.all_whole == 0 and pn.all_whole == 0
    want = [r for runs in part["runs"] for r in runs]
    assert {W, W + 1} <= set(want) and [] in part["runs"]  # (a stretch of W - 1 leaves no run)
    assert cm.item_runs(p.items)[1].tolist() == [r - W + 1 for r in want]
    starts, wins = cm.visited_runs(part["codes"], part["offs"], W)
    assert wins.tolist() == [r - W + 1 for r in want]
    lens = np.diff(part["offs"]).tolist()
    assert W - 1 in lens and W in lens
    assert pn.n_windows == 0 and len(pn.items) == 0 and len(cm.visited_runs(none["codes"], none["offs"], W)[0]) == 0
