"""The oracle (oracle/peng_oracle.cpp) against what the COMPILED REFERENCE made of the constructed edge cases of
tests/em_edges_model.py, tests/table_edges_model.py and tests/count_edges_model.py -- from the fixtures
tests/golden/edges_*.npz alone (tests/golden/make_edge_golden.py writes them where the reference exists;
tests/edge_fixtures.py is the layout).  No GPU, no reference at test time.

Every test first regenerates its inputs from the model and compares their sha256 with the fixture's: a failure that
says "inputs drifted" means a model (or numpy's generators) changed and the fixtures need regenerating, not that
anything is wrong with the oracle.  Then: float32 bit patterns equal (NaN by bytes), integers equal.

W = 14 has no fixture: the reference's size_t counter table alone is 2 GiB there, a run takes many minutes; W = 14
stays oracle-only (tests/test_gpu_table_edges.py, tests/test_gpu_count_edges.py).

What the reference could not be asked: see UNDEFINED and NARROWED in tests/golden/make_edge_golden.py;
test_exclusions_stay_within_their_cap holds them to the issue's 5 % per class.

Disagreements found when the fixtures were first made: none in values.  The iteration-count recipe (smallest cap that
returns the final PWM) disagreed with the oracle on S/d1 (every weight denormal): there the PWM repeats IN BYTES after
one iteration under a threshold of 0.0, the loop goes on to max_iter and the returned PWMs cannot show it -- not
identifiable (edge_fixtures.em_reference_iterations), dropped below by name."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import edge_fixtures as ef
import em_edges_model as em
import table_edges_model as tm
from oracle import oracle as po

# ---- EM ----------------------------------------------------------------------------------------------------------------
# Dropped from the iteration comparison, by name: cases where a PWM's count cannot be read off the reference's returned
# PWMs (edge_fixtures.em_reference_iterations says why).  test_em_iteration_counts asserts that this list is exactly the
# set the fixture's own data marks, so nothing can be dropped for disagreeing.
EM_COUNT_NOT_IDENTIFIABLE = {
    "S/b": "every row 0 / 0 after the first iteration: NaN repeats in bytes, its change stops nothing",
    "S/c": "the overflowing cell's row is NaN after the first iteration",
    "S/d1": "all weights denormal: the PWM repeats in bytes after one iteration, threshold 0.0",
    "T/nan_change": "S/b under a threshold of 0.08",
    "F/bg_zero": "zero over zero: the PWMs with a zero entry under the defect are NaN after the first iteration",
    "F/bg_nan": "every PWM is NaN after the first iteration",
    "F/count_max": "inf over inf in the PWMs with a zero entry under the defect",
}


def _em_oracle(c, i, max_iter=None):
    return po.em(c["W"], c["counts"].astype(np.uint64), c["bg"], c["pwms"][i], c["saturation"], c["threshold"],
                 c["max_iter"] if max_iter is None else max_iter, mode=0)


def _em_setup(W):
    fix = ef.load(ef.em_file(W))
    cases = ef.em_cases(W)
    assert sorted(fix["index"]) == sorted(c["tag"] for _, c in cases), "the fixture's cases are not the model's: regenerate"
    for cls, c in cases:
        drift = ef.inputs_match(fix, c["tag"], ef.em_inputs(c))
        assert drift is None, drift
    return fix, cases


@pytest.mark.parametrize("W", ef.EM_WS)
def test_em_final_pwm_bit_for_bit(W):
    """Every class (G, F, S, T) the model has at W: po.em(..., mode=0) WITH its final normalisation against the PWM the
    reference returned at max_iter -- and, for class T, at every cap 0 .. max_iter.  The final normalisation is one more
    float32 row division (IUPACPattern's constructor): a difference confined to a row that this division maps to the same
    bits would be hidden."""
    fix, cases = _em_setup(W)
    jobs = []
    for cls, c in cases:
        caps = range(c["max_iter"] + 1) if cls == "T" else (c["max_iter"],)
        jobs += [(c, i, cap) for cap in caps for i in range(len(c["pwms"]))]
    with ThreadPoolExecutor(8) as pool:
        got = list(pool.map(lambda j: _em_oracle(j[0], j[1], j[2])[0], jobs))
    bad = []
    for (c, i, cap), pw in zip(jobs, got):
        want = ef.em_reference(fix, c)[cap, i]
        if pw.tobytes() != want.tobytes():
            j = int(np.flatnonzero(pw.view(np.uint32).reshape(-1) != want.view(np.uint32).reshape(-1))[0])
            bad.append("%s, PWM %d, cap %d, cell (%d, %s): oracle %r (0x%08x), reference %r (0x%08x)"
                       % (c["tag"], i, cap, j >> 2, "ACGT"[j & 3], float(pw.reshape(-1)[j]), int(pw.view(np.uint32).reshape(-1)[j]),
                          float(want.reshape(-1)[j]), int(want.view(np.uint32).reshape(-1)[j])))
    assert not bad, "%d PWMs differ, the first ones:\n%s" % (len(bad), "\n".join(bad[:8]))


def _dropped(tag):
    return next((k for k in EM_COUNT_NOT_IDENTIFIABLE if tag.startswith(k + "/")), None)


@pytest.mark.parametrize("W", ef.EM_WS)
def test_em_iteration_counts(W):
    """The stopping rule's reference-side pin.  The reference never reports its count; it is the smallest cap m whose PWM
    equals the PWM at max_iter byte for byte -- asserted identifiable on the fixture alone first (caps 0 .. m pairwise
    different, no fixed point in bytes before max_iter), PWM by PWM; the PWMs that are not are exactly those of the
    cases named in EM_COUNT_NOT_IDENTIFIABLE.  Then the oracle's `it` equals m.  Class T: `equal` and `above` stop at
    T_K, `below` goes on, +inf never starts, -0.0 and NaN run to max_iter."""
    fix, cases = _em_setup(W)
    jobs = []
    for cls, c in cases:
        derived = ef.em_reference_iterations(ef.em_reference(fix, c), c["threshold"])
        # the counts the fixture stores (what the GPU tests compare h_iters with) are this derivation's
        assert ef.em_reference_counts(fix, c).tolist() == [m if ok else -1 for m, ok in derived], c["tag"]
        for i, (m, ok) in enumerate(derived):
            if ok:  # (in a named case too: the PWMs the defect does not reach)
                jobs.append((c, i, m))
            else:
                assert _dropped(c["tag"]) is not None, "%s, PWM %d: the count is not identifiable and the case is not named" % (c["tag"], i)
    with ThreadPoolExecutor(8) as pool:
        its = list(pool.map(lambda j: _em_oracle(j[0], j[1])[1], jobs))
    bad = ["%s, PWM %d: oracle %d iterations, reference %d" % (c["tag"], i, it, m) for (c, i, m), it in zip(jobs, its) if it != m]
    assert not bad, "\n".join(bad[:8])
    if "T" in em.classes(W):
        ref_its = {c["kind"]: ef.em_reference_iterations(ef.em_reference(fix, c), c["threshold"])[0] for cls, c in cases if cls == "T"}
        k, mx = em.T_K, em.T_MAX_ITER
        assert ref_its["equal"] == (k, True) and ref_its["above"] == (k, True)
        assert ref_its["below"][1] and k < ref_its["below"][0] <= mx
        assert ref_its["+inf"] == (0, True) and ref_its["-0.0"] == (mx, True) and ref_its["nan"] == (mx, True)


def test_em_cases_dropped_from_the_iteration_comparison_are_the_unidentifiable_ones():
    """every name in EM_COUNT_NOT_IDENTIFIABLE is marked by the fixtures' own data at some W, and nothing else is"""
    marked = set()
    for W in ef.EM_WS:
        fix = ef.load(ef.em_file(W))
        for cls, c in ef.em_cases(W):
            if not all(ok for _, ok in ef.em_reference_iterations(ef.em_reference(fix, c), c["threshold"])):
                assert _dropped(c["tag"]) is not None, c["tag"]
                marked.add(_dropped(c["tag"]))
    assert marked == set(EM_COUNT_NOT_IDENTIFIABLE), (sorted(marked), sorted(EM_COUNT_NOT_IDENTIFIABLE))


# ---- counts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", ef.COUNT_WS)
def test_count_tables(W):
    """Every class of count_edges_model, both strand modes: the oracle's table (mirrored under both strands, as the
    reference stores it), ltot and the background counters against what the reference counted on the same sequences
    written as FASTA (invalid bases as N): sha256 of the table, the stored bins, the table in full for W <= 6."""
    import count_edges_model as cm  # (imports the product package for its packer; no device)
    fix = ef.load(ef.count_file(W))
    cases = ef.count_cases(W)
    assert sorted(fix["index"]) == sorted(ef.count_tag(cls, part, W, both) for cls, _, part, both in cases)
    assert set(fix["classes"].tolist()) == set(cm.CLASSES)
    for cls, _, part, both in cases:
        tag = ef.count_tag(cls, part, W, both)
        drift = ef.inputs_match(fix, tag, ef.count_inputs(part))
        assert drift is None, drift
        r = fix["index"][tag]
        got, ltot = po.count(part["codes"], part["offs"], W, both)
        assert ltot == int(fix["ltot"][r]), tag
        idx = fix["slice_idx"][fix["slice_off"][r]:fix["slice_off"][r + 1]].astype(np.int64)
        want = fix["slice_val"][fix["slice_off"][r]:fix["slice_off"][r + 1]]
        if 4 ** W <= ef.FULL_LIMIT:
            assert idx.size == 4 ** W
        bad = np.flatnonzero(got[idx] != want)
        assert not bad.size, "%s: bin %d: oracle %d, reference %d" % (tag, idx[bad[0]], got[idx[bad[0]]], want[bad[0]]) if bad.size else None
        assert np.array_equal(ef.digest(got), fix["sha_counts"][r]), tag
        assert np.array_equal(po.bg_counts(part["codes"], part["offs"], 2), fix["bgcounts"][r]), tag


# ---- tables ------------------------------------------------------------------------------------------------------------
def sweep_against_fixture(fix, tag, tables, failures, logp=None, who="oracle"):
    """tables: name -> float32 table of one case.  sha256 (canonical NaN) and the stored slice of every table; `logp`:
    None = like the others, or a function (got, want) -> bad indices that replaces both for log-p."""
    r = fix["index"][tag]
    idx = fix["slice_idx"][r].astype(np.int64)
    idx = idx[idx >= 0]
    for j, name in enumerate(ef.SWEEP_TABLES):
        if name not in tables:
            assert not fix["sha_out"][r, j].any(), (tag, name)
            continue
        t = np.ascontiguousarray(tables[name], np.float32)
        want = fix["slice_val"][r, j, :idx.size]
        if name == "logp" and logp is not None:
            bad = logp(t[idx], want.view(np.float32))
        else:
            bad = np.flatnonzero(ef.canonical(t[idx]) != ef.canonical(want.view(np.float32)))
            if not bad.size and not np.array_equal(ef.table_digest(t), fix["sha_out"][r, j]):
                failures.append("%s: %s: sha256 of the %s's table is not the reference's (the stored slice agrees)" % (tag, name, who))
        if len(bad):
            x = int(idx[bad[0]])
            failures.append("%s: %s, pattern %d (%s): %s %r (0x%08x), reference %r (0x%08x)"
                            % (tag, name, x, po.kmer_str(x, int(tag.split("/")[1][1:])), who, float(t[x]), int(t[x:x + 1].view(np.uint32)[0]),
                               float(want.view(np.float32)[bad[0]]), int(want[bad[0]])))
        if "full" in fix and not (name == "logp" and logp is not None):
            assert np.array_equal(ef.canonical(t), ef.canonical(fix["full"][r, j].view(np.float32))), (tag, name)


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("W", ef.TABLE_WS)
def test_sweep_tables(W, both):
    """Every sweep case the model has at W (the full cross product up to W = 10, the chosen ones at 12): bgprob[0..max_k]
    (from V through the reference's own calculate_bg_probabilities and aggregate_double_strand_background), expected,
    log-p and z bit for bit -- sha256 of each table plus the stored slice (zero-count bins, the mu edges and every other
    count edge, palindromes, own-twin tiles, seeds, a strided sample); W <= 4 in full.  The two seed selections of oracle/ref_dump.cpp
    where the reference's own z table holds no NaN (std::sort with `>` on NaN is undefined: src/base_pattern.cpp:458)."""
    fix = ef.load(ef.table_file(W))
    cases = [case for b, case in ef.sweep_cases(W) if b == both]
    mine = [t for t in fix["index"] if t.split("/")[2] == ("both" if both else "plus")]
    assert sorted(mine) == sorted(ef.sweep_tag(W, both, case) for case in cases), "the fixture's cases are not the model's: regenerate"
    failures = []
    for case in cases:
        tag = ef.sweep_tag(W, both, case)
        c = tm.sweep_case(W, both, case)
        drift = ef.inputs_match(fix, tag, ef.sweep_inputs(c))
        assert drift is None, drift
        r = fix["index"][tag]
        assert np.array_equal(ef.sweep_slice(c, _seed_head(fix, r, 0)), fix["slice_idx"][r]), tag
        sweep_against_fixture(fix, tag, ef.sweep_tables(c), failures)
        if fix["seeds_defined"][r]:
            for i, (zt, ct, flt) in enumerate(ef.SEED_SELECTIONS):
                got = po.select(W, c["z"], c["counts"].astype(np.uint64), zt, ct, not both, bool(flt))
                if not (np.array_equal(ef.digest(got), fix["seed_sha"][r, i]) and np.array_equal(got[:64], _seed_head(fix, r, i))):
                    failures.append("%s: seed selection %d differs (oracle %d seeds: %s ...)" % (tag, i, len(got), got[:4].tolist()))
        else:
            assert np.isnan(c["z"]).any(), tag
        del c
    assert not failures, "%d mismatches, the first ones:\n%s" % (len(failures), "\n".join(failures[:8]))


def _seed_head(fix, r, i):
    off = fix["seeds%d_off" % i]
    return fix["seeds%d_head" % i][off[r]:off[r + 1]].astype(np.uint64)


def test_background_model():
    """calculateV() on the constructed counters written into BackgroundModel::n_, every alpha and order: V bit for bit.
    The counter sets beyond 2^31 have no fixture (NARROWED: the reference's counters are `int`)."""
    fix = ef.load(ef.MISC_FILE)
    want = {name: V for name, _, _, _, V in tm.bg_model_cases()}
    rows = [t for t, cl in zip(fix["tags"], fix["classes"]) if cl == "bg"]
    n = 0
    for tag, counters, K, alpha, in_range in ef.bg_cases():
        if not in_range:
            assert any(tag.startswith(p) for p in fix["narrowed"]), tag
            continue
        drift = ef.inputs_match(fix, tag, ef.bg_inputs(counters, K, alpha))
        assert drift is None, drift
        ref = fix["bg_V"][rows.index(tag)]
        assert np.array_equal(want[tag[3:]].view(np.uint32), ref), tag
        n += 1
    assert n == len(rows) == 36


@pytest.mark.parametrize("W,both,v", ef.IUPAC_CASES)
def test_iupac_aggregation(W, both, v):
    """aggregate_attributes_from_basepatterns and count_combined_occurences on the injected edge tables, per id of the
    model (all-N, the LDS-limit member counts, own reverse complements, single k-mers at every count edge): sites and the
    combined count equal, bg_p / expected / z / log-p bit for bit."""
    fix = ef.load(ef.MISC_FILE)
    tag = ef.iupac_tag(W, both, v)
    c = tm.iupac_case(W, both, v)
    drift = ef.inputs_match(fix, tag, ef.iupac_inputs(c))
    assert drift is None, drift
    k = [t for t, cl in zip(fix["tags"], fix["classes"]) if cl == "iupac"].index(tag)
    a, e = fix["iupac_off"][k], fix["iupac_off"][k + 1]
    assert e - a == len(c["ids"])
    c64 = c["counts"].astype(np.uint64)
    assert fix["iupac_names"][a:e].tolist() == list(c["names"])
    excluded = set(ef.load("edges_excluded")["tags"].tolist())
    for j, w in enumerate(c["want"]):
        where = (tag, c["names"][j])
        if fix["iupac_died"][a + j]:  # the reference's own assert aborted on this id (make_edge_golden.UNDEFINED)
            assert "%s#%s" % where in excluded, where
            continue
        assert w.sites == int(fix["iupac_sites"][a + j]), where
        assert po.iupac_count(int(c["ids"][j]), W, both, c64) == int(fix["iupac_cc"][a + j]), where
        got = np.array([w.bg_p, w.expected, w.zscore, w.log_pvalue], np.float32).view(np.uint32)
        assert np.array_equal(got, fix["iupac_stats"][4 * (a + j):4 * (a + j) + 4]), where + (got.view(np.float32).tolist(),)


@pytest.mark.parametrize("both", [False, True])
def test_similarity(both):
    """IUPACPattern::calculate_S on the model's motifs of 1 .. 64 columns: the values agree with the reference "to ~1e-4,
    NOT bit for bit" (include/pengk.h), so the restated float32 running sums and the fp64 formula the kernel implements
    are held to the margin tests/test_gpu_parity.py uses (5e-4) against the compiled reference's values, -inf exactly
    where it gives -inf."""
    fix = ef.load(ef.MISC_FILE)
    drift = ef.inputs_match(fix, ef.sim_tag(both), ef.sim_inputs())
    assert drift is None, drift
    ref = fix["sim_S"][int(both)].view(np.float32)
    pw, cp, lens, sites = tm.motif_set()
    pairs = tm.pair_list(len(lens))
    assert len(ref) == len(pairs)
    exact = tm.exact_grid(both)
    for q, (i, j) in enumerate(pairs):
        f64 = tm.fp64_S(pw[i, :lens[i]], cp[i, :lens[i]], sites[i], pw[j, :lens[j]], cp[j, :lens[j]], sites[j], both, tm.SIM_BG)
        for what, got in (("float32 running sums", exact[q]), ("fp64 formula", f64)):
            if np.isneginf(ref[q]) or np.isneginf(got):
                assert np.isneginf(ref[q]) and np.isneginf(got), (what, i, j)
            else:
                assert abs(float(got) - float(ref[q])) <= 5e-4, (what, i, j, int(lens[i]), int(lens[j]), float(got), float(ref[q]))


# ---- exclusions ----------------------------------------------------------------------------------------------------------
def test_exclusions_stay_within_their_cap():
    """The cases left out of the reference comparison because the reference's own behaviour is undefined there: at most
    5 % of any class, no class empty, every one named with its reason; and every class of the three models at every
    W <= 12 has fixture entries."""
    ex = ef.load("edges_excluded")
    excluded = [str(t) for t in ex["tags"]]
    assert len(excluded) == len(ex["reasons"]) and all(len(str(r)) > 10 for r in ex["reasons"])
    classes = {}
    for W in ef.EM_WS:
        for cls, c in ef.em_cases(W):
            classes.setdefault("em " + cls, []).append(c["tag"])
    for W in ef.COUNT_WS:
        for cls, _, part, both in ef.count_cases(W):
            classes.setdefault("count " + cls, []).append(ef.count_tag(cls, part, W, both))
    for W in ef.TABLE_WS:
        classes.setdefault("sweep", []).extend(ef.sweep_tag(W, both, case) for both, case in ef.sweep_cases(W))
    classes["bg"] = [c[0] for c in ef.bg_cases() if c[4]]
    misc = ef.load(ef.MISC_FILE)
    classes["iupac"] = []
    for k, case in enumerate(ef.IUPAC_CASES):  # (an IUPAC case is a list of ids: the unit is the id)
        names = misc["iupac_names"][misc["iupac_off"][k]:misc["iupac_off"][k + 1]]
        classes["iupac"] += ["%s#%s" % (ef.iupac_tag(*case), nm) for nm in names]
    classes["sim"] = [ef.sim_tag(b) for b in (False, True)]
    have = {t for t, d in zip(classes["iupac"], misc["iupac_died"]) if not d}
    for name in [ef.em_file(W) for W in ef.EM_WS] + [ef.count_file(W) for W in ef.COUNT_WS] + [ef.table_file(W) for W in ef.TABLE_WS] + [ef.MISC_FILE]:
        have |= {t for t in ef.load(name)["index"] if not t.startswith("iupac/")}
    everything = {t for tags in classes.values() for t in tags}
    assert set(excluded) <= everything
    assert have == everything - set(excluded)
    assert not have & set(excluded)
    for cls, tags in classes.items():
        out = [t for t in tags if t in excluded]
        assert len(out) <= 0.05 * len(tags), (cls, out)
        assert len(out) < len(tags), cls
