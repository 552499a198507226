"""The control null of the sweep (tests/control_stats_model.py) on the CPU alone: the constructed cases hold the
classes they are built for -- so that tests/test_gpu_control_stats.py compares the device on what it claims to -- and
the definition does what it is for: on a planted scenario the k-mers of a contaminant that the control shares take
half of the seed slots under the Markov null and none under the control's counts."""
import numpy as np
import pytest

import control_stats_model as cm
import table_edges_model as tm
from oracle import oracle as po

# what the cases of one (W, strand setting) must hold between them
NEEDED = ("c = 0", "c = 1", "c = 2^32 - 1", "share == p_k in fp64", "share == p_0 in fp64",
          "share below p_k by less than a float ulp", "share above p_k by less than a float ulp",
          "share rounds one float ulp below p_k", "share rounds one float ulp above p_k",
          "control wins at order k", "Markov wins at order k", "q_k differs from p_k",
          "Markov wins at order 0, control at order max_k", "control wins at order 0, Markov at order max_k")


def _check_classes(W, both, cases):
    seen = {name: 0 for name in NEEDED}
    on_palindromes = {"control wins at order k": 0, "Markov wins at order k": 0, "share == p_k in fp64": 0}
    pal = cm.palindromes(W)
    r = tm.revcomp_ids(W)
    totals, pseudo, forms, branches = set(), set(), set(), {}
    for spec in cases:
        c = cm.case(W, both, spec)
        totals.add(c["Lc"])
        pseudo.add(c["a"])
        forms.add(c["ctrl_mirrored"])
        masks = cm.class_masks(c["p"], c["k"], c["ctrl"], c["Lc"], c["a"])
        for name in NEEDED:
            seen[name] += int(masks[name].sum())
        for name in on_palindromes:
            on_palindromes[name] += int((masks[name] & pal).sum())
        if c["Lc"] == 0:  # an empty control: the Markov tables, bit for bit
            for o in range(c["max_k"] + 1):
                assert c["bgp"][o].tobytes() == c["p"][o].tobytes()
        if both:
            same = c["ctrl"] == c["ctrl"][r]
            if c["ctrl_mirrored"]:
                assert same.all()
            elif c["Lc"] > 1:
                assert (~same).any() and (same & ~pal).any()  # twins with different and with equal control counts
        # the branches of the statistics, under the new expected counts
        for name, m in tm.count_classes(c).items():
            branches[name] = branches.get(name, 0) + int(m.sum())
    assert totals >= {0, 1, 2 ** 40} and pseudo == {0.0, 0.5, 1.0}
    if both:
        assert forms == {False, True}
    assert all(branches.values()), branches
    missing = [n for n in NEEDED if not seen[n]]
    assert not missing, (W, both, missing)
    if both and W >= 4:
        assert all(on_palindromes.values()), on_palindromes


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("W", [4, 8, 10])
def test_small_cases_hold_their_classes(W, both):
    cases = cm.small_cases(W, both)
    assert {(s[2], s[3]) for s in cases} == set(tm.legal_orders(W))
    _check_classes(W, both, cases)


def test_the_w12_case_holds_its_classes():
    W = 12
    c = cm.case(W, True, cm.big_case(W))
    masks = cm.class_masks(c["p"], c["k"], c["ctrl"], c["Lc"], c["a"])
    own = tm.own_twin_tile_mask(W)
    r = tm.revcomp_ids(W)
    differ = c["ctrl"] != c["ctrl"][r]
    for name in NEEDED:
        if name == "share == p_0 in fp64":
            continue
        assert (masks[name] & own).any() and (masks[name] & ~own).any(), name
    # pair tiles: twins whose control counts differ and twins whose counts agree; the input's counts are mirrored
    assert (differ & ~own).any() and (~differ & ~own & ~cm.palindromes(W)).any()
    assert (c["counts"] == c["counts"][r]).all()
    # ... and a twin's q differs from its partner's exactly where the definition says
    assert (c["bgp"][c["k"]] != c["bgp"][c["k"]][r]).any()


@pytest.mark.parametrize("both", [False, True])
def test_nothing_is_enriched_against_itself(both):
    c = cm.own_table_case(8, both)
    assert c["ctrl"] is c["counts"] and c["Lc"] == c["ltot"]
    assert (c["z"] <= 0).all()
    assert (c["logp"][c["counts"] > 0] == 0).all()


def test_the_definition_rounds_once():
    """(c + a) / Lc is formed in fp64 and rounded to float32 once: a share that float32 arithmetic would have rounded
    to p_k stays above it in the comparison, and the result is the share's own nearest float"""
    p = np.array([0.001, 0.001, 0.001, 0.0], np.float32)
    Lc = 2 ** 40
    t = int(np.float64(p[0]) * Lc)
    ctrl = np.array([t - 1, t, t + 1, 0], np.uint32)
    q = cm.control_null(p, ctrl, Lc, 0.0)
    assert q[0] == p[0] and q[1] == p[1] and q[2] == p[2]        # all within half a float ulp of p
    assert (np.float64(ctrl[2]) / Lc > np.float64(p[2]))          # ... though the third lies above p in fp64
    assert q[3] == 0.0
    assert cm.control_null(p, ctrl, Lc, 0.5)[3] == np.float32(0.5 / Lc)
    assert cm.control_null(p, ctrl, 0, 1.0).tobytes() == p.tobytes()


# ---- the planted scenario ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [8, 10])
def test_planted_contaminant_takes_no_seed_under_the_control_null(W):
    """2 000 x 100 bp of uniform random sequence, U in 30 % of the input and of the control, T in 30 % of the input only;
    both strands, order 2, default thresholds, numpy seeds 1 to 3.  Markov null: at least 10 seeds share a 6-mer with U.
    Control null: none does, and every seed shares one with T.  (The printed rows are README's table.)"""
    for seed in (1, 2, 3):
        markov, control, u_z = cm.planted_seeds(seed, W)
        m_u = sum(cm.shares_6mer(w, cm.U_MOTIF) for w in markov)
        c_u = sum(cm.shares_6mer(w, cm.U_MOTIF) for w in control)
        c_t = sum(cm.shares_6mer(w, cm.T_MOTIF) for w in control)
        print("| %d | %d | %d, %d | %d, %d, %d | %.1f |" % (W, seed, len(markov), m_u, len(control), c_u, c_t, u_z))
        assert m_u >= 10, (W, seed, markov)
        assert c_u == 0, (W, seed, [w for w in control if cm.shares_6mer(w, cm.U_MOTIF)])
        assert control and c_t == len(control), (W, seed, [w for w in control if not cm.shares_6mer(w, cm.T_MOTIF)])
