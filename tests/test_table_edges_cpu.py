"""The conditions that keep tests/test_gpu_table_edges.py from passing vacuously, asserted on the oracle's outputs alone:
the constructed tables of tests/table_edges_model.py really put patterns on every branch of the table-space kernels.

Which classes a sweep case CAN hold follows from its size, and the assertions say so:
  * `n > 5 and (float)n <= mu` needs expected counts of at least 6.  The tables take their own edges from the median and the
    99th percentile of mu: a case where half of the patterns expect 6 or more must hold the class; with small ltot and long
    patterns no pattern can, and over the cases of a (W, strand mode) the class must occur.
  * W = 2 has 16 patterns, and a mirrored table 10 free values (6 twin pairs, 4 palindromes) for 15 edges: there the classes
    are asked of a case's two table forms together.
  * W = 14 runs fewer cases than W = 12 (an oracle sweep takes a minute there): V kind "b" and two of the four ltot are
    left to W = 12, which runs the same two kernels; everything that depends on W = 14 itself -- products of 14 factors
    that reach the denormals and zero, z = +inf and NaN -- is asked of W = 14."""
import numpy as np
import pytest

import table_edges_model as tm
from oracle import oracle as po

F32_MIN_NORMAL = np.float32(1.1754944e-38)


def test_vectorised_reverse_complement_is_the_oracles():
    for W in (2, 4, 6, 8, 10, 12, 14):
        r = tm.revcomp_ids(W)
        for x in (0, 1, 6, 4 ** W - 1, 4 ** W // 3, 4 ** W // 7 * 5):
            assert int(r[x]) == po.revcomp(x, W), (W, x)
        assert r.dtype == np.uint32 and len(r) == 4 ** W
    own = tm.own_twin_tile_mask(12)
    assert int(own.sum()) == 4 ** 3 * 4096  # the 4^3 middles of 6 digits that are their own twins, 4096 patterns each


def test_edge_tables_hold_every_edge_in_both_forms():
    for W in (2, 4, 10):
        c = tm.edge_counts(W, (11, 12, 13, 14), mirrored=False, salt=W)
        assert set(np.unique(c).tolist()) == set(tm.FIXED_EDGES) | {11, 12, 13, 14}
        r = tm.revcomp_ids(W)
        assert (c != c[r]).any()  # as built, twins differ: the n_tw != n branch of the twin-tile kernel
        m = tm.edge_counts(W, (11, 12, 13, 14), mirrored=True, salt=W)
        assert np.array_equal(m, m[r])
        if W > 2:
            assert set(np.unique(m).tolist()) == set(np.unique(c).tolist())


def _assert_classes(W, both, case, c, partner=None):
    cls = tm.count_classes(c)
    other = tm.count_classes(partner) if partner is not None else None
    for name, mask in cls.items():
        if name == "n > 5, (float)n <= mu" and not (np.nan_to_num(c["expected"]) >= 6).mean() >= 0.5:
            continue
        have = mask.any() or (other is not None and other[name].any())
        assert have, (W, both, case, name)
    return cls


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("W", [2, 4, 6, 8, 10, 12])
def test_sweep_cases_put_patterns_on_every_branch(W, both):
    cases = tm.sweep_cases(W, both)
    if W <= 10:
        assert len(cases) == 3 * len(tm.LTOTS) * len(tm.legal_orders(W)) * 2  # the full cross product
    else:
        for kernel_cases in (tm.BIG_BOTH, tm.BIG_PLUS):  # what each kernel must see at W = 12
            assert {c[0] for c in kernel_cases} == set("abc") and {c[1] for c in kernel_cases} == set(tm.LTOTS)
            assert any(c[2] < c[3] for c in kernel_cases) and {c[4] for c in kernel_cases} == {False, True}
    seen = {}
    top_bin_above_mu = 0
    for case in cases:
        c = tm.sweep_case(W, both, case)
        partner = None
        if W == 2 and case[4]:
            partner = tm.sweep_case(W, both, case[:4] + (False,))
        cls = _assert_classes(W, both, case, c, partner)
        for name, mask in cls.items():
            seen[name] = seen.get(name, 0) + int(mask.any())
        # the case the device got wrong before (float)(n + 1) was formed in 64 bits: n = 2^32 - 1 above its expected count,
        # where the reference's log-p is finite (with (float)n <= mu both sides write 0 and the defect hides)
        hit = cls["n == 2^32 - 1"] & cls["n > 5, (float)n > mu"] & np.isfinite(c["logp"]) & (c["logp"] != 0)
        top_bin_above_mu += int(hit.any())
        if W >= 4 and np.nanmax(c["expected"]) < 2.0 ** 31:
            assert hit.any(), (W, both, case)
        if W == 12 and both:
            own, pal = tm.own_twin_tile_mask(W), tm.revcomp_ids(W) == np.arange(4 ** W, dtype=np.uint32)
            for name, mask in cls.items():
                if mask.any():
                    assert (mask & own).any(), (case, name, "own-twin tile")
                    assert (mask & pal).any(), (case, name, "palindrome")
    assert all(v > 0 for v in seen.values()) and len(seen) == 5, seen
    assert top_bin_above_mu > 0


@pytest.mark.parametrize("both", [False, True])
def test_w14_products_reach_the_denormals_and_zero(both):
    cases = tm.sweep_cases(14, both)
    assert any(c[0] == "c" for c in cases) and any(c[0] == "a" for c in cases)
    if both:
        assert any(c[2] < c[3] for c in cases) and {c[4] for c in cases} == {False, True}
    for case in cases:
        c = tm.sweep_case(14, both, case)
        cls = _assert_classes(14, both, case, c)
        assert (cls["n == 2^32 - 1"] & cls["n > 5, (float)n > mu"] & np.isfinite(c["logp"]) & (c["logp"] != 0)).any()
        if case[0] != "c":
            continue
        for o, b in enumerate(c["bgp"]):
            assert ((b > 0) & (b < F32_MIN_NORMAL)).any(), (case, o, "denormal")
            assert (b == 0).any(), (case, o, "zero")
        assert np.isposinf(c["z"]).any() and np.isnan(c["z"]).any(), case
        assert np.isneginf(c["logp"]).any(), case  # mu = 0 under a count above 5
        del c


def test_background_model_inputs_never_divide_zero_by_zero():
    cases = tm.bg_model_cases()
    assert len(cases) == len(tm.COUNTER_KINDS) * len(tm.ALPHAS) * 3
    sets = tm.counter_sets()
    assert (sets["no_T"][0][[3, 7, 11, 16, 17, 18, 19]] == 0).all() and sets["no_T"][0][:3].all()
    n = sets["no_context"][0]
    assert n[:4].all() and (n[4:20] == 0).sum() == 3
    assert sets["above_2_24"][0].max() > 2 ** 24 and sets["above_2_24"][0][:4].sum() < 2 ** 31
    assert sets["above_2_31"][0][4:20].max() > 2 ** 31 and sets["above_2_31"][1]
    for name, n, K, alpha, V in cases:
        assert min(alpha) > 0
        used = sum(4 ** (k + 1) for k in range(K + 1))
        assert np.isfinite(V).all() and (V[:used] > 0).all() and (V[used:] == 0).all(), name
    # below 2^31 bases the reference's `int` counters and the 64-bit ones agree
    assert np.array_equal(po.bg_V(sets["above_2_24"][0], 2), po.bg_V(sets["above_2_24"][0], 2, wide=True))
    assert not np.array_equal(po.bg_V(sets["above_2_31"][0], 2), po.bg_V(sets["above_2_31"][0], 2, wide=True))
    Vc = tm.hand_made_V()
    assert np.allclose(Vc.reshape(21, 4).sum(axis=1), 1.0, atol=2e-7)
    assert (Vc == 0).any() and ((Vc > 0) & (Vc <= np.float32(1e-4))).sum() >= 20


def test_seed_tables_hold_the_threshold_edges():
    for W in (2, 4, 10):
        z = tm.seed_z(W)
        c = tm.edge_counts(W, mirrored=False, salt=W)
        bits = set(z.view(np.uint32).tolist())
        for t in (10.0, 0.0):
            for v in (np.float32(t), np.nextafter(np.float32(t), np.float32(-np.inf)), np.nextafter(np.float32(t), np.float32(np.inf))):
                assert (int(np.float32(v).view(np.uint32)) in bits) or W == 2, (W, v)
        if W > 2:
            assert {0x7FC00000, 0xFFC00000, 0x80000000, 0x7F800000, 0xFF800000} <= bits
        sizes = [int(tm.seed_expected(z, c, zt, ct).sum()) for zt, ct in tm.SEED_THRESHOLDS]
        if W > 2:
            assert all(s > 0 for s in sizes[:5]), sizes
            assert sizes[2] < 4 ** W - int(np.isnan(z).sum())  # (-inf, 1): everything but NaN and the empty bins
            assert sizes[2] > sizes[0] and sizes[1] > sizes[0]
        assert sizes[5] == 0 and sizes[6] == 0  # a threshold above 2^32 - 1 admits no 32-bit bin


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("W", [10, 12])
def test_iupac_cases_hold_the_sizes_and_both_outcomes(W, both):
    z_gt2, c_gt5 = set(), set()
    for vkind in "ac":
        c = tm.iupac_case(W, both, vkind)
        members = {nm: tm.iupac_members(i, W) for nm, i in zip(c["names"], c["ids"])}
        assert members["all_N"] == 4 ** W and members["members_8192"] == 8192 and members["members_4096"] == 4096
        assert members["members_16384"] == 16384 == members["members_16384_spread"] and members["members_32768"] == 32768
        assert members["half_of_all"] == 4 ** W // 2
        assert sum(1 for v in members.values() if v == 1) >= 10
        for nm in ("members_8192", "own_rc_SW", "own_rc_N"):
            i = int(c["ids"][c["names"].index(nm)])
            ex = po.iupac_expand(i, W, both)
            assert len(ex) == members[nm]
            if nm.startswith("own_rc"):  # its own reverse complement: the set of members is closed under it
                plus = set(po.iupac_expand(i, W, False).tolist())
                assert {po.revcomp(x, W) for x in list(plus)[:64]} <= plus
        big = [members[nm] > 8192 for nm in c["names"]]
        assert any(a != b for a, b in zip(big, big[1:]))  # small and large mixed
        w = dict(zip(c["names"], c["want"]))
        assert w["all_N"].sites > 2 ** 32
        for st in c["want"]:
            if st.sites > 0 and float(st.sites) > st.expected:
                z_gt2.add(bool(st.zscore > 2))
            c_gt5.add(st.sites > 5)
    assert z_gt2 == {False, True} and c_gt5 == {False, True}


@pytest.mark.parametrize("both", [False, True])
def test_motif_set_covers_the_grid_and_fp64_stays_inside_the_bar(both):
    pw, cp, lens, sites = tm.motif_set()
    n = len(lens)
    assert sorted(lens.tolist()) == sorted(tm.MOTIF_LENGTHS) and min(lens) == 1 and max(lens) == 64
    assert len(set(sites.tolist())) == n - 2
    one_hot = pw[n - 1, :lens[n - 1]]
    assert set(np.unique(one_hot).tolist()) == {0.0, 1.0}
    pairs = tm.pair_list(n)
    want = tm.exact_grid(both)
    assert np.isneginf(want).any() and np.isfinite(want).any()
    assert max(tm.n_shift_pairs(lens[i], lens[j], both) for i, j in pairs) > 64
    worst = 0.0
    for q, (i, j) in enumerate(pairs):
        got = tm.fp64_S(pw[i, :lens[i]], cp[i, :lens[i]], sites[i], pw[j, :lens[j]], cp[j, :lens[j]], sites[j], both, tm.SIM_BG)
        assert np.isneginf(want[q]) == (tm.n_shift_pairs(lens[i], lens[j], both) == 0) == np.isneginf(got), (i, j)
        if np.isfinite(want[q]):
            worst = max(worst, abs(float(got) - float(want[q])))
    print("fp64 restatement against the float32 running sums: worst difference of the maxima %.3g" % worst)
    assert worst <= 5e-4, worst
