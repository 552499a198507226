"""The table-space kernels -- pengk_bg_model, pengk_pattern_stats (both kernels of csrc/stats.hip),
pengk_seed_candidates, pengk_iupac_aggregate, pengk_motif_similarity -- on CONSTRUCTED tables at their value edges
(tests/table_edges_model.py), against the oracle.  Tables go to the device as they are; no sequences are attached, no
count runs.  tests/test_table_edges_cpu.py asserts that the cases hold the classes they are built for.

Bars, the project's own (tests/test_gpu_parity.py): V, bgprob[0..max_k], expected, z and the IUPAC sums bit for bit; log-p
within 1 float ulp (device log against glibc's); infinities agree exactly; NaN agrees in position (x86 and gfx950
produce different NaN signs for 0/0, so not in bits); the similarity grid within 5e-4 of the reference's float32 running
sums, -inf exactly where they give -inf.

And directly against the COMPILED REFERENCE at W <= 12 (tests/golden/edges_tables_*.npz, written by
tests/golden/make_edge_golden.py from the reference's own classes with these tables injected): V bit for bit; of every
sweep table the sha256 (NaN in canonical form, for the reason above) and the stored slices; log-p at the stored slices
within 1 ulp and without a hash (its bits are glibc's on the reference's side); the IUPAC sums bit for bit; the
similarity grid within the same 5e-4 of the compiled calculate_S.  W = 14 stays oracle-only: the reference's size_t
counter table alone is 2 GiB there.  These tests read tests/golden only, never the reference."""
import ctypes as C

import numpy as np
import pytest

import edge_fixtures as ef
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
_SWEEPS = {}  # (tag, kernel): {"idx": the fixture's slice indices, table: (sha256 of the device's table, its values at idx)}


def _note_sweep(c, kernel):
    """what the reference test needs of the device's tables of a case, taken while the oracle test has them in hand"""
    seen = {"idx": np.zeros(0, np.int64)}
    if c["W"] in ef.TABLE_WS:
        seen["sha_in"] = [ef.digest(a) for a in ef.sweep_inputs(c)]
        fix = ef.load(ef.table_file(c["W"]))
        tag = ef.sweep_tag(c["W"], c["both"], (c["vkind"], c["ltot"], c["k"], c["max_k"], c["mirrored"]))
        if tag in fix["index"]:
            idx = fix["slice_idx"][fix["index"][tag]].astype(np.int64)
            seen["idx"] = idx[idx >= 0]
        _SWEEPS[tag, kernel] = seen
    return seen


def _note_table(seen, name, got):
    seen[name] = (None if name == "logp" else ef.table_digest(got), got[seen["idx"]].copy())


def _sweep_kernels(W, both):
    return ("twin-tile", "per-pattern") if (W >= 12 and both) else ("per-pattern",)


def _run_sweep_case(ctx, c, d_V, failures):
    W, both = c["W"], c["both"]
    d_lt = pk.DeviceArray.from_host(ctx, np.array([c["ltot"]], np.uint64))
    d_c = pk.DeviceArray.from_host(ctx, c["counts"])
    kernels = (("twin-tile", 1), ("per-pattern", 0)) if (W >= 12 and both) else (("per-pattern", 1),)
    for kernel, pairs in kernels:
        ctx.set_option("sweep_pairs", pairs)
        out = ctx.pattern_stats(W, both, c["k"], c["max_k"], d_V, d_lt, d_c)
        bgp = out[0].to_host()
        seen = _note_sweep(c, kernel)
        for o in range(c["max_k"] + 1):
            _note_table(seen, "bgp%d" % o, bgp[o])
            bad = _mismatch(bgp[o], c["bgp"][o])
            if bad.size:
                failures.append(_describe(c, "bgprob[%d]" % o, bad[0], bgp[o], c["bgp"][o], kernel) + " (%d patterns)" % bad.size)
        del bgp
        for what, d, want, cmp in (("expected", out[1], c["expected"], _mismatch), ("z", out[3], c["z"], _mismatch),
                                   ("log-p", out[2], c["logp"], _beyond_one_ulp)):
            got = d.to_host()
            _note_table(seen, {"expected": "expected", "z": "z", "log-p": "logp"}[what], got)
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


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("W", ef.TABLE_WS)
def test_sweep_on_edge_tables_against_the_reference(ctx, W, both):
    """The device's tables of test_sweep_on_edge_tables (computed again only if that test did not run) against the
    compiled reference's fixture, for every case and kernel: inputs first ("inputs drifted" means regenerate); then
    bgprob[0..max_k], expected and z by sha256 and at the stored slices (zero-count bins, the mu edges and every other
    count edge, palindromes, own-twin tiles, seeds) bit for bit, NaN in position; log-p at the stored slices within 1
    ulp."""
    fix = ef.load(ef.table_file(W))
    cases = tm.sweep_cases(W, both)
    tags = [ef.sweep_tag(W, both, case) for case in cases]
    rerun = not all((t, k) in _SWEEPS and len(_SWEEPS[t, k]) > 2 for t in tags for k in _sweep_kernels(W, both))
    failures = []
    d_V = {}
    try:
        for case, tag in zip(cases, tags):
            if rerun:
                c = tm.sweep_case(W, both, case)
                if case[0] not in d_V:
                    d_V[case[0]] = pk.DeviceArray.from_host(ctx, c["V"])
                _run_sweep_case(ctx, c, d_V[case[0]], [])
                del c
            assert tag in fix["index"], "case %s has no fixture entry: regenerate with tests/golden/make_edge_golden.py" % tag
            r = fix["index"][tag]
            for kernel in _sweep_kernels(W, both):
                seen = _SWEEPS[tag, kernel]
                for j, d in enumerate(seen["sha_in"]):
                    assert np.array_equal(d, fix["sha_in"][r, j]), "inputs drifted: input %d of case %s; regenerate" % (j, tag)
                n = seen["idx"].size
                for j, name in enumerate(ef.SWEEP_TABLES):
                    if name not in seen:  # (an order beyond max_k)
                        assert not fix["sha_out"][r, j].any(), (tag, name)
                        continue
                    sha, vals = seen[name]
                    want = fix["slice_val"][r, j, :n].view(np.float32)
                    bad = _beyond_one_ulp(vals, want) if name == "logp" else _mismatch(vals, want)
                    if bad.size:
                        x = int(seen["idx"][bad[0]])
                        failures.append("%s, kernel %s: %s, pattern %d (%s): device %r (0x%08x), reference %r (0x%08x)"
                                        % (tag, kernel, name, x, po.kmer_str(x, W), float(vals[bad[0]]), int(vals[bad[0]:bad[0] + 1].view(np.uint32)[0]),
                                           float(want[bad[0]]), int(want[bad[0]:bad[0] + 1].view(np.uint32)[0])))
                    elif sha is not None and not np.array_equal(sha, fix["sha_out"][r, j]):
                        failures.append("%s, kernel %s: %s: the table's sha256 is not the reference's (the stored slice agrees)" % (tag, kernel, name))
    finally:
        ctx.set_option("sweep_pairs", 1)
    assert not failures, "%d mismatches, the first ones:\n%s" % (len(failures), "\n".join(failures[:8]))


def test_background_model_against_the_reference(ctx):
    """pengk_bg_model on the constructed counters that fit the reference's `int` (every kind but above_2_31, every alpha
    and order) against the V the compiled calculateV() made of them: bit for bit."""
    fix = ef.load(ef.MISC_FILE)
    rows = [t for t, cl in zip(fix["tags"], fix["classes"]) if cl == "bg"]
    done = 0
    for (name, n, K, alpha, _), (tag, used, _, _, in_range) in zip(tm.bg_model_cases(), ef.bg_cases()):
        assert tag == "bg/" + name
        if not in_range:
            continue
        drift = ef.inputs_match(fix, tag, ef.bg_inputs(used, K, alpha))
        assert drift is None, drift
        d_n = pk.DeviceArray.from_host(ctx, n.astype(np.uint64))
        d_V = pk.DeviceArray.from_host(ctx, np.full(84, np.float32(-7.0)))
        got = ctx.bg_model(d_n, K, alpha, out=d_V).to_host()
        want = fix["bg_V"][rows.index(tag)]
        bad = np.flatnonzero(got.view(np.uint32) != want)
        assert not bad.size, "V differs: %s, entry %d: device %r, reference %r" % (name, bad[0], got[bad[0]], want[bad[0]:bad[0] + 1].view(np.float32)[0]) if bad.size else None
        done += 1
    assert done == len(rows)


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
_IUPAC = {}  # (W, both, V, budget): (the device's columns, the ids' names, sha256 of the inputs)
_IUPAC_FIELDS = ("sites", "bg_p", "expected", "zscore", "log_pvalue")


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
            _IUPAC[W, both, vkind, budget] = ({f: np.array(out[f], copy=True) for f in _IUPAC_FIELDS}, list(c["names"]),
                                              [ef.digest(a) for a in ef.iupac_inputs(c)])
            for j, w in enumerate(c["want"]):
                where = (W, both, vkind, budget, c["names"][j], po.iupac_str(int(c["ids"][j]), W))
                assert int(out["sites"][j]) == w.sites, where
                for f in ("bg_p", "expected", "zscore", "log_pvalue"):
                    a = np.float32(out[f][j]).view(np.uint32)
                    b = np.float32(getattr(w, f)).view(np.uint32)
                    assert a == b, where + (f, float(out[f][j]), float(getattr(w, f)))
    finally:
        ctx.set_option("iupac_group_bytes", 0)


@pytest.mark.parametrize("vkind", ["a", "c"])
@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("W", [10, 12])
def test_iupac_aggregation_against_the_reference(ctx, W, both, vkind):
    """What the device returned in test_iupac_aggregation_on_edge_tables (run again only if that test did not) against
    the compiled reference's aggregate_attributes_from_basepatterns on the same injected tables: `sites` equal, bg_p,
    expected, z and log-p bit for bit, under both scratch budgets.  An id on which the reference's own assert aborts
    (tests/golden/make_edge_golden.py, UNDEFINED) has no reference row and is left to the oracle test."""
    budgets = (0, (8 << 20) if W == 10 else (64 << 20))
    if not all((W, both, vkind, b) in _IUPAC for b in budgets):
        test_iupac_aggregation_on_edge_tables(ctx, W, both, vkind)
    fix = ef.load(ef.MISC_FILE)
    tag = ef.iupac_tag(W, both, vkind)
    k = [t for t, cl in zip(fix["tags"], fix["classes"]) if cl == "iupac"].index(tag)
    a, e = int(fix["iupac_off"][k]), int(fix["iupac_off"][k + 1])
    for budget in budgets:
        out, names, shas = _IUPAC[W, both, vkind, budget]
        for j, d in enumerate(shas):
            assert np.array_equal(d, fix["sha_in"][fix["index"][tag], j]), "inputs drifted: input %d of case %s; regenerate" % (j, tag)
        assert fix["iupac_names"][a:e].tolist() == names
        for j, name in enumerate(names):
            if fix["iupac_died"][a + j]:
                continue
            where = (tag, budget, name)
            assert int(out["sites"][j]) == int(fix["iupac_sites"][a + j]), where
            got = np.array([out[f][j] for f in _IUPAC_FIELDS[1:]], np.float32).view(np.uint32)
            want = fix["iupac_stats"][4 * (a + j):4 * (a + j) + 4]
            assert np.array_equal(got, want), where + (got.view(np.float32).tolist(), want.view(np.float32).tolist())


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


@pytest.mark.parametrize("both", [False, True])
def test_similarity_grid_against_the_compiled_reference(ctx, both):
    """The same grid against IUPACPattern::calculate_S as the reference's compiler built it (the fixture), not its
    restatement: within the same 5e-4 (the values agree "to ~1e-4, NOT bit for bit", include/pengk.h), -inf exactly
    where the reference gives -inf."""
    fix = ef.load(ef.MISC_FILE)
    drift = ef.inputs_match(fix, ef.sim_tag(both), ef.sim_inputs())
    assert drift is None, drift
    want = fix["sim_S"][int(both)].view(np.float32)
    pw, cp, lens, sites = tm.motif_set()
    pairs = tm.pair_list(len(lens))
    got = np.full(len(pairs), np.float32(-77.0))
    _similarity(ctx, pw, cp, lens, sites, both, 0, got)
    for q, (i, j) in enumerate(pairs):
        if np.isneginf(want[q]) or np.isneginf(got[q]):
            assert np.isneginf(want[q]) and np.isneginf(got[q]), (i, j, float(got[q]), float(want[q]))
        else:
            assert abs(float(got[q]) - float(want[q])) <= 5e-4, (i, j, int(lens[i]), int(lens[j]), float(got[q]), float(want[q]))
