"""The cases of tests/em_edges_model.py are what they claim to be -- by the oracle and the restated guard alone, no GPU."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import em_edges_model as em
from oracle import oracle as po


def _oracle(c, i, mode=0, max_iter=None):
    return po.em(c["W"], c["counts"].astype(np.uint64), c["bg"], c["pwms"][i], c["saturation"], c["threshold"],
                 c["max_iter"] if max_iter is None else max_iter, mode=mode, final_norm=False)


def _ok(c, i):
    b = em.bg_range(c["bg"])
    return em.lean_ranges_ok(c["pwms"][i], b[0], b[1], c["saturation"])


def test_restated_guard_on_ordinary_and_degenerate_input():
    W = 8
    pw = em.healthy_pwms(W, 1)[0]
    b = em.bg_range(em.healthy_bg(W))
    assert em.lean_ranges_ok(pw, b[0], b[1], 1e4)
    zero = pw.copy()
    zero[3, 1] = 0.0
    assert not em.lean_ranges_ok(zero, b[0], b[1], 1e4)
    for v in (0.0, -1.0, np.inf, np.nan):
        bg = em.healthy_bg(W)
        bg[77] = v
        r = em.bg_range(bg)
        assert not em.lean_ranges_ok(pw, r[0], r[1], 1e4), v
    assert not em.lean_ranges_ok(pw, b[0], b[1], 0.0) and not em.lean_ranges_ok(pw, b[0], b[1], 2.0 ** 100)


@pytest.mark.parametrize("W", em.WS)
def test_every_ladder_has_cases_on_both_sides_of_its_inequality(W):
    """Per ladder and form: the ladder's own inequality (of its own division) fails on the three rungs of the failing side
    and holds on the four of the passing side; a ladder that no other inequality shadows has the GUARD AS A WHOLE false on
    the failing side and true on the passing side (so one binade of slack on that inequality changes what the kernel does
    on rung -1); the two ordinary PWMs of a batch pass the guard.  And at W < 12 the twelve inequalities are all there."""
    seen = set()
    for c in em.class_G(W):
        b = em.bg_range(c["bg"])
        for i, pos in enumerate(c["rungs"]):
            if pos is None:
                continue
            d = em.lean_ranges_detail(c["pwms"][i], b[0], b[1], c["saturation"])
            assert d["positive"] and d["background"], c["tag"]
            assert d[c["division"]][c["inequality"]] == (pos >= 0), (c["tag"], pos, d)
            if c["shadowed"] is None:
                assert _ok(c, i) == (pos >= 0), (c["tag"], pos, d)
            else:
                assert not _ok(c, i) or pos >= 0, (c["tag"], pos, d)
            seen.add((c["ladder"], c["form"], pos))
        if len(c["pwms"]) == 9:
            assert _ok(c, 7) and _ok(c, 8), c["tag"]
    names = sorted(em.LADDERS) if W < 12 else em.W12_LADDERS
    for name in names:
        for form in (("pow2", "mant") if W in (8, 10) else ("pow2",)):
            assert {pos for n, f, pos in seen if (n, f) == (name, form)} == set(range(-em.fail_rungs(name), em.PASS_RUNGS)), (name, form)
    if W < 12:
        assert {(em.LADDERS[n][0], em.LADDERS[n][1]) for n in names} == {(d, i) for d in (1, 2, 3) for i in (1, 2, 3, 4)}
        assert sum(em.LADDERS[n][6] is None for n in names) == 8


def test_power_of_two_ladders_cross_where_the_derivation_says():
    """the table in the model's docstring: rung 0 of a power-of-two ladder is the nominal (P, B, S) itself"""
    for name in em.LADDERS:
        for W in (2, 10):
            assert [k for k, pos in em.ladder_rungs(name, W, "pow2") if pos == 0] == [0], (name, W)


@pytest.mark.parametrize("W", [2, 4, 6, 8, 10])
def test_flagged_cases_produce_what_they_are_built_for(W):
    """By kind: the first iteration's cell sums (fp64 accumulation of the reference's float32 terms) of the PWMs with a zero
    entry under the defect and of their ordinary neighbours; and what the oracle's two iterations make of them."""
    with ThreadPoolExecutor(8) as pool:
        for c in em.class_F(W):
            c64 = c["counts"].astype(np.uint64)
            acc = list(pool.map(lambda i: po.em_accumulate(W, c64, c["bg"], c["pwms"][i], c["saturation"]), range(9)))
            plain = [i for i in range(9) if i not in em.F_MATCHING]
            kind = c["kind"]
            if kind == "bg_zero":  # zero over zero: NaN; positive over zero: finite
                assert all(np.isnan(acc[i]).any() for i in em.F_MATCHING) and all(np.isfinite(acc[i]).all() for i in plain), c["tag"]
            elif kind == "bg_negative":
                rest64 = np.where(np.arange(4 ** W) != c["x"], c["counts"], 0).astype(np.uint64)
                rest = list(pool.map(lambda i: po.em_accumulate(W, rest64, c["bg"], c["pwms"][i], c["saturation"]), plain))
                for i, r in zip(plain, rest):  # the one negative weight: c s / (1 + s / odds) with odds < 0
                    assert (acc[i] - r).min() < 0 and np.isfinite(acc[i]).all(), c["tag"]
            elif kind == "bg_inf":  # weight 0, everything finite
                assert all(np.isfinite(a).all() for a in acc), c["tag"]
            elif kind == "bg_nan":
                assert all(np.isnan(a).any() for a in acc), c["tag"]
            elif kind == "count_max":  # inf over a finite denominator: +inf; with a zero product: inf / inf
                assert all(np.isposinf(acc[i]).any() and not np.isnan(acc[i]).any() for i in plain), c["tag"]
                assert all(np.isnan(acc[i]).any() for i in em.F_MATCHING), c["tag"]
            for i in em.F_ELSEWHERE:  # a zero entry over positive background entries: a cell of exactly 0
                if kind in ("bg_zero", "bg_inf"):
                    assert (acc[i] == 0).sum() == 1, c["tag"]
            (pw, it, ch), (pwm, itm, chm) = pool.map(lambda i: _oracle(c, i), (0, em.F_MATCHING[0]))
            assert it == 2
            if kind in ("bg_zero", "bg_inf"):
                assert np.isfinite(pw).all() and np.isfinite(ch), c["tag"]
            if kind != "bg_inf" and kind != "bg_negative":
                assert np.isnan(pwm).any() and np.isnan(chm), c["tag"]


def test_flagged_placements():
    """every kind at every placement, at every W but 12; nine PWMs; the placements are where they are said to be"""
    for W in em.WS:
        places = dict(em.f_placements(W))
        assert set(places) == ({"first_block", "last_block", "span_end", "span_start"} if W >= 8 else {"first_block", "last_block"})
        assert places["first_block"] < min(4096, 4 ** W) and 4 ** W - places["last_block"] <= 4
        if W >= 8:
            assert places["span_end"] == 16383 and places["span_start"] == 16384
        cs = em.class_F(W)
        for c in cs:
            assert len(c["pwms"]) == 9 and c["max_iter"] == (2 if W < 12 else 1)
            assert c["x"] in places.values()
        if W < 12:
            assert sorted((c["kind"], c["x"]) for c in cs) == sorted((k, x) for k in em.F_KINDS for x in places.values()), W
        else:
            assert [(c["kind"], c["x"]) for c in cs] == [("bg_zero", 16383)]


@pytest.mark.parametrize("W", [8, 10])
def test_cell_sum_cases_are_what_they_claim(W):
    cs = {c["tag"].split("/")[1]: c for c in em.class_S(W) if c["kind"] != "f"}
    u64 = lambda c: c["counts"].astype(np.uint64)
    # (a): exactly one zero cell after the first iteration, consumed by the second
    c = cs["a"]
    p0, a0 = c["cell"]
    pw1 = _oracle(c, 0, max_iter=1)[0]
    assert pw1[p0, a0] == 0 and (pw1 == 0).sum() == 1 and np.isfinite(pw1).all()
    pw2, it, ch = _oracle(c, 0)
    assert it == 2 and pw2[p0, a0] == 0 and np.isfinite(pw2).all()
    # (b): every row 0 / 0
    c = cs["b"]
    pw1, it, ch = _oracle(c, 0, max_iter=1)
    assert np.isnan(pw1).all() and np.isnan(ch)
    # (c): the oracle's cell is +inf, the fp64 accumulation of its terms beyond FLT_MAX -- and about half-way
    c = cs["c"]
    p0, a0 = c["cell"]
    acc = po.em_accumulate(W, u64(c), c["bg"], c["pwms"][0], c["saturation"])
    assert np.isfinite(acc).all() and acc[p0, a0] > float(em.FLT_MAX) and 1.7 < acc[p0, a0] / float(em.FLT_MAX) < 2.1
    others = np.delete(acc.reshape(-1), 4 * p0 + a0)
    assert others.max() < 0.6 * float(em.FLT_MAX)
    pw1 = _oracle(c, 0, max_iter=1)[0]
    assert np.isnan(pw1[p0, a0]) and (np.delete(pw1[p0], a0) == 0).all()  # inf / inf, finite / inf
    assert np.isfinite(np.delete(pw1, p0, axis=0)).all()
    # (d): every weight denormal
    for name in ("d1", "d2"):
        c = cs[name]
        for i in range(len(c["pwms"])):
            pr = em.products(c, i)
            with np.errstate(all="ignore"):
                s = np.float32(c["saturation"])
                w = (c["counts"].astype(np.float32) * s) / (np.float32(1) + s / (pr / c["bg"]))
            assert w.max() > 0 and w.max() < np.float32(2.0 ** -126), (name, i)
            assert np.isfinite(_oracle(c, i)[0]).all()
    # (e): the giant term lies in the last block of its chains
    c = cs["e"]
    big = np.flatnonzero(c["counts"] == 1 << 31)
    assert big.tolist() == [4 ** W - 2] and (np.delete(c["counts"], big) == 1).all()
    # (f): the ramp crosses many binades, under both saturations
    ramps = [c for c in em.class_S(W) if c["kind"] == "f"]
    assert [c["saturation"] for c in ramps] == [1.0, 2.0 ** 40]
    assert len(np.unique(np.floor(np.log2(ramps[0]["counts"])))) == 31


@pytest.mark.parametrize("W", [8, 10])
def test_stopping_rule_cases_differ_as_the_reference_rule_says(W):
    cs = {c["kind"]: c for c in em.class_T(W)}
    with ThreadPoolExecutor(8) as pool:
        its = dict(zip(cs, pool.map(lambda c: _oracle(c, 0)[1], cs.values())))
    k, m = em.T_K, em.T_MAX_ITER
    assert its["equal"] == k and its["above"] == k   # change <= threshold stops the loop: at equality too
    assert k < its["below"] <= m
    assert its["+inf"] == 0
    assert its["-0.0"] == m and its["nan"] == m      # nothing compares <= NaN; no change is <= -0.0 but 0
    assert its["nan_change"] == m                    # a NaN change never stops the loop early
    assert np.isnan(_oracle(cs["nan_change"], 0)[2])
    # the change of PWM 0 falls from iteration to iteration up to T_K, so that `equal` stops exactly there
    ch = [_oracle(cs["nan"], 0, max_iter=j)[2] for j in range(1, k + 1)]
    assert all(a > b for a, b in zip(ch, ch[1:])) and ch[-1] == cs["equal"]["change_k"]


def test_selection_and_w12_budget():
    assert em.classes(8) == em.classes(10) == ("G", "F", "S", "T")
    assert em.classes(2) == em.classes(4) == em.classes(6) == ("G", "F")
    assert em.w12_budget() == 33  # (the issue: under about 40)
    kinds = {c["kind"] for c in em.class_S(12)}
    assert kinds == {"c", "e"} and len(em.class_F(12)) == 1
    assert {c["division"] for c in em.class_G(12)} == {1, 2, 3}
    assert all(c["form"] == "pow2" for W in (2, 4, 6) for c in em.class_G(W))
    assert {c["form"] for c in em.class_G(10)} == {"pow2", "mant"}
    assert em.fast_mode_domain(em.class_T(8)[0], 0)
    assert not em.fast_mode_domain([c for c in em.class_G(8) if c["ladder"] == "D1-I2"][0], 0)
