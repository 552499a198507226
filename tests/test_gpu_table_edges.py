"""The table-space kernels -- pengk_bg_model, pengk_pattern_stats (both kernels of csrc/stats.hip),
pengk_seed_candidates, pengk_iupac_aggregate, pengk_motif_similarity -- on CONSTRUCTED tables at their value edges
(tests/table_edges_model.py), against the oracle.  Tables go to the device as they are; no sequences are attached, no
count runs.  tests/test_table_edges_cpu.py asserts that the cases hold the classes they are built for.

Bars, the project's own (tests/test_gpu_parity.py): V, bgprob[0..max_k], expected, z and the IUPAC sums bit for bit; log-p
within 1 float ulp (device log against glibc's); infinities agree exactly; NaN agrees in position (x86 and gfx950
produce different NaN signs for 0/0, so not in bits); the similarity grid within 5e-4 of the reference's float32 running
sums, -inf exactly where they give -inf."""
import ctypes as C

import numpy as np
import pytest

import peng_motif_amd as pk
import table_edges_model as tm
from oracle import oracle as po

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = pk.Context(0)
    yield c
    c.close()


def _mismatch(g, w):
    """indices where two float32 arrays differ in bits, NaN against NaN excepted"""
    bad = np.flatnonzero(g.view(np.uint32) != w.view(np.uint32))
    if bad.size:
        bad = bad[~(np.isnan(g[bad]) & np.isnan(w[bad]))]
    return bad


def _ordered(a):
    """float32 bits as integers that ascend with the value (-0.0 and 0.0 one apart)"""
    i = a.view(np.int32).astype(np.int64)
    return np.where(i >= 0, i, -(i & 0x7FFFFFFF) - 1)


def _beyond_one_ulp(g, w):
    """indices where two float32 arrays differ by more than one ulp; infinities must agree exactly, NaN in position"""
    bad = _mismatch(g, w)
    if bad.size:
        gb, wb = g[bad], w[bad]
        fin = np.isfinite(gb) & np.isfinite(wb)
        ok = fin & (np.abs(_ordered(gb) - _ordered(wb)) <= 1)
        bad = bad[~ok]
    return bad


def _describe(c, what, x, got, want, kernel):
    x = int(x)
    return ("%s differs: W = %d, %s, kernel %s, V %s, ltot %d, k = %d, max_k = %d, %s table, pattern %d (%s), count %d: "
            "device %r (0x%08x), oracle %r (0x%08x)"
            % (what, c["W"], "both strands" if c["both"] else "plus strand", kernel, c["vkind"], c["ltot"], c["k"], c["max_k"],
               "mirrored" if c["mirrored"] else "as built", x, po.kmer_str(x, c["W"]), int(c["counts"][x]),
               float(got[x]), int(got[x:x + 1].view(np.uint32)[0]), float(want[x]), int(want[x:x + 1].view(np.uint32)[0])))


# ---- background model ------------------------------------------------------------------------------------------------
def test_background_model_on_constructed_counters(ctx):
    """Every V of the constructed counter sets bit for bit against po.bg_V (64-bit counters where they pass 2^31, the
    semantics the product documents); entries beyond the used orders are 0.0.  None of these inputs makes the reference
    divide 0 by 0: every alpha is positive, so every denominator n + alpha is (a context that never occurs gets the lower
    order's distribution).  An alpha of 0 with an empty context would, and is not part of the contract."""
    for name, n, K, alpha, want in tm.bg_model_cases():
        d_n = pk.DeviceArray.from_host(ctx, n.astype(np.uint64))
        d_V = pk.DeviceArray.from_host(ctx, np.full(84, np.float32(-7.0)))
        got = ctx.bg_model(d_n, K, alpha, out=d_V).to_host()
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        assert not bad.size, "V differs: %s, entry %d: device %r, oracle %r" % (name, bad[0], got[bad[0]], want[bad[0]])


# ---- sweep -----------------------------------------------------------------------------------------------------------
def _run_sweep_case(ctx, c, d_V, failures):
    W, both = c["W"], c["both"]
    d_lt = pk.DeviceArray.from_host(ctx, np.array([c["ltot"]], np.uint64))
    d_c = pk.DeviceArray.from_host(ctx, c["counts"])
    kernels = (("twin-tile", 1), ("per-pattern", 0)) if (W >= 12 and both) else (("per-pattern", 1),)
    for kernel, pairs in kernels:
        ctx.set_option("sweep_pairs", pairs)
        out = ctx.pattern_stats(W, both, c["k"], c["max_k"], d_V, d_lt, d_c)
        bgp = out[0].to_host()
        for o in range(c["max_k"] + 1):
            bad = _mismatch(bgp[o], c["bgp"][o])
            if bad.size:
                failures.append(_describe(c, "bgprob[%d]" % o, bad[0], bgp[o], c["bgp"][o], kernel) + " (%d patterns)" % bad.size)
        del bgp
        for what, d, want, cmp in (("expected", out[1], c["expected"], _mismatch), ("z", out[3], c["z"], _mismatch),
                                   ("log-p", out[2], c["logp"], _beyond_one_ulp)):
            got = d.to_host()
            bad = cmp(got, want)
            if bad.size:
                failures.append(_describe(c, what, bad[0], got, want, kernel) + " (%d patterns)" % bad.size)
            del got
        for d in out:
            d.free()
    d_lt.free()
    d_c.free()


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("W", [2, 4, 6, 8, 10, 12, 14])
def test_sweep_on_edge_tables(ctx, W, both):
    """pengk_pattern_stats on count tables that hold every value edge (0, 1, 5, 6, 7, 2^24 +- 1, 2^31, 2^32 - 2, 2^32 - 1,
    the case's own expected counts rounded down and up), V from natural counters, from constructed ones and hand-made with
    entries down to 1e-6 and exact zeros, ltot up to 2e10, every legal (k, max_k): the full cross product for W <= 10;
    at W = 12 and 14 the chosen cases of table_edges_model, the both-strand ones under the twin-tile kernel and under the
    per-pattern kernel (sweep_pairs = 0)."""
    failures = []
    try:
        d_V = {}
        for case in tm.sweep_cases(W, both):
            c = tm.sweep_case(W, both, case)
            if case[0] not in d_V:
                d_V[case[0]] = pk.DeviceArray.from_host(ctx, c["V"])
            _run_sweep_case(ctx, c, d_V[case[0]], failures)
            del c
            if len(failures) > 20:
                break
    finally:
        ctx.set_option("sweep_pairs", 1)
    assert not failures, "%d mismatches, the first ones:\n%s" % (len(failures), "\n".join(failures[:8]))


# ---- seed candidates ---------------------------------------------------------------------------------------------------
def _seed_call(ctx, W, d_z, d_c, zthr, cthr, cap, null=False):
    ids = np.full(max(cap, 1), 0xFFFFFFFF, np.uint32)
    zs = np.full(max(cap, 1), np.float32(-123.0))
    n = C.c_int64(-1)
    pk._check(pk.lib().pengk_seed_candidates(ctx.h, W, pk._ptr(d_z), pk._ptr(d_c), zthr, cthr, None if null else ids.ctypes.data,
                                             None if null else zs.ctypes.data, cap, C.byref(n)))
    return ids, zs, int(n.value)


@pytest.mark.parametrize("W", [2, 4, 10, 14])
def test_seed_candidates_on_constructed_z(ctx, W):
    """The header's sentence decides: candidates are the ids with z >= z_threshold and count >= count_threshold.  A NaN z
    is no candidate, a count threshold above 2^32 - 1 admits no bin (the reference compares size_t counts), -0.0 >= 0.0
    holds.  z holds each threshold, one ulp below and above, +-inf, -0.0, NaN of both signs; the counts are an edge
    table.  Capacity 0 with NULL buffers, exactly n, n - 1 and ample: *n_out is the full number every time, no id comes
    twice, every z is its id's in bits."""
    z = tm.seed_z(W)
    counts = tm.edge_counts(W, mirrored=False, salt=W)
    d_z, d_c = pk.DeviceArray.from_host(ctx, z), pk.DeviceArray.from_host(ctx, counts)
    zbits = z.view(np.uint32)
    for t, (zthr, cthr) in enumerate(tm.SEED_THRESHOLDS):
        want = tm.seed_expected(z, counts, zthr, cthr)
        n = int(want.sum())
        _, _, n0 = _seed_call(ctx, W, d_z, d_c, zthr, cthr, 0, null=True)
        assert n0 == n, (W, zthr, cthr, "capacity 0", n0, n)
        caps = [n, n - 1, n + 100] if (W < 14 or t == 0) else []  # (W = 14: ids by the hundred million; once is enough)
        for cap in caps:
            if cap < 0:
                continue
            ids, zs, got_n = _seed_call(ctx, W, d_z, d_c, zthr, cthr, cap)
            assert got_n == n, (W, zthr, cthr, cap, got_n, n)
            k = min(cap, n)
            got = ids[:k]
            hit = np.zeros(4 ** W, bool)
            hit[got] = True
            assert int(hit.sum()) == k, (W, zthr, cthr, cap, "an id came twice")
            extra = np.flatnonzero(hit & ~want)
            assert not extra.size, (W, zthr, cthr, cap, "not a candidate: id %d, z %r, count %d" % (extra[0], z[extra[0]], counts[extra[0]])) if extra.size else None
            if cap >= n:
                miss = np.flatnonzero(want & ~hit)
                assert not miss.size, (W, zthr, cthr, cap, "missing: id %d, z %r, count %d" % (miss[0], z[miss[0]], counts[miss[0]])) if miss.size else None
            assert np.array_equal(zs[:k].view(np.uint32), zbits[got]), (W, zthr, cthr, cap)
            if cap > k:
                assert (ids[k:cap] == 0xFFFFFFFF).all()  # nothing written beyond the candidates
            del hit, ids, zs


# ---- IUPAC aggregation -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vkind", ["a", "c"])
@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("W", [10, 12])
def test_iupac_aggregation_on_edge_tables(ctx, W, both, vkind):
    """pengk_iupac_aggregate on the edge count tables (mirrored under both strands, as callers hand them over) and the
    oracle's bgp / expected of the sweep cases: all-N (at W = 12 2^24 members, `sites` beyond 2^32), member counts at the
    LDS limit (4096, 8192 in a workgroup; 16384, 32768 through the list pipeline), patterns that are their own reverse
    complement, single k-mers at every count edge, small and large mixed; with the default scratch budget and one that
    forces several groups.  `sites` equal, the four floats bit for bit."""
    c = tm.iupac_case(W, both, vkind)
    d_counts = pk.DeviceArray.from_host(ctx, c["counts"])
    d_bgp = pk.DeviceArray.from_host(ctx, c["bgp"])
    d_exp = pk.DeviceArray.from_host(ctx, c["expected"])
    try:
        for budget in (0, (8 << 20) if W == 10 else (64 << 20)):
            ctx.set_option("iupac_group_bytes", budget)
            out = ctx.iupac_aggregate(W, both, c["ids"], d_counts, d_bgp, d_exp)
            for j, w in enumerate(c["want"]):
                where = (W, both, vkind, budget, c["names"][j], po.iupac_str(int(c["ids"][j]), W))
                assert int(out["sites"][j]) == w.sites, where
                for f in ("bg_p", "expected", "zscore", "log_pvalue"):
                    a = np.float32(out[f][j]).view(np.uint32)
                    b = np.float32(getattr(w, f)).view(np.uint32)
                    assert a == b, where + (f, float(out[f][j]), float(getattr(w, f)))
    finally:
        ctx.set_option("iupac_group_bytes", 0)


# ---- similarity grid ---------------------------------------------------------------------------------------------------
def _similarity(ctx, pw, cp, lens, sites, both, first_new, out):
    pk._check(pk.lib().pengk_motif_similarity(ctx.h, len(lens), pw.ctypes.data, cp.ctypes.data, lens.ctypes.data,
                                              sites.ctypes.data, int(both), tm.SIM_BG.ctypes.data, first_new, out.ctypes.data))


@pytest.mark.parametrize("both", [False, True])
def test_similarity_grid_from_1_to_64_columns(ctx, both):
    """pengk_motif_similarity on motifs of 1 .. 64 columns (the ABI's range; --max_merged_length lets a user get there):
    pairs without a qualifying shift (-inf), pairs with more (orientation, shift) pairs than a wave has lanes, PWM
    entries of exactly 0 and 1.  Every pair within 5e-4 of the reference's float32 running sums -- a quarter of the host
    mirror's selection margin, not scaled with the length: the fp64 restatement stays a factor of ten inside it at 64
    columns (tests/test_table_edges_cpu.py)."""
    pw, cp, lens, sites = tm.motif_set()
    n = len(lens)
    want = tm.exact_grid(both)
    pairs = tm.pair_list(n)
    full = np.full(len(pairs), np.float32(-77.0))
    _similarity(ctx, pw, cp, lens, sites, both, 0, full)
    worst = 0.0
    for q, (i, j) in enumerate(pairs):
        if np.isneginf(want[q]) or np.isneginf(full[q]):
            assert np.isneginf(want[q]) and np.isneginf(full[q]), (i, j, int(lens[i]), int(lens[j]), float(full[q]), float(want[q]))
            continue
        d = abs(float(full[q]) - float(want[q]))
        assert d <= 5e-4, (i, j, int(lens[i]), int(lens[j]), float(full[q]), float(want[q]))
        worst = max(worst, d)
    print("similarity grid, both = %d: worst difference %.3g" % (both, worst))
    # the columns that follow a merge: the same bits as the corresponding slices of the triangle
    for first_new in (n // 2, n - 1):
        m = len(tm.pair_list(n, first_new))
        col = np.full(m + 1, np.float32(-77.0))
        _similarity(ctx, pw, cp, lens, sites, both, first_new, col)
        assert col[:m].tobytes() == full[len(pairs) - m:].tobytes(), first_new
        assert col[m] == np.float32(-77.0)
    # no pair: first_new = n, and a single motif -- the output is untouched
    for nn, first_new in ((n, n), (1, 0), (1, 1)):
        col = np.full(4, np.float32(-77.0))
        _similarity(ctx, pw[:nn], cp[:nn], lens[:nn], sites[:nn], both, first_new, col)
        assert (col == np.float32(-77.0)).all(), (nn, first_new)
