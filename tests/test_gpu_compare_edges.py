"""The kernels of csrc/compare.hip on the constructed cases of tests/compare_edges_model.py (held to their classes by
tests/test_compare_edges_cpu.py): the whole tail table through pengk_test_compare_tails against integer arithmetic, bit
for bit; every record of the dyadic databases against the model's best alignment with no near-tie band; the all-ones
records in closed form; and the host plan at its chunk and batch seams.  A new comparison of a compare kernel with an
exact reference belongs here."""
import functools

import numpy as np
import pytest

import peng_motif_amd as pk
import compare_edges_model as ce
import motif_compare_model as mc
from test_gpu_motif_compare import check_records, padded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = pk.Context(0)
    yield c
    c.close()


def where(w, e):
    """(i0, n, S) of element e of a table of width w"""
    for i0 in range(w):
        for n in range(1, w - i0 + 1):
            s = ce.tail_slice(w, i0, n)
            if s.start <= e < s.stop:
                return i0, n, e - s.start
    raise AssertionError(e)


def assert_same_table(got, want, w):
    assert got.dtype == want.dtype == np.float64 and got.shape == want.shape == (ce.table_size(w),)
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
        e = int(bad[0])
        raise AssertionError("%d of %d cells differ; the first at (i0, n, S) = %s: device %r, exact %r"
                             % (len(bad), len(got), where(w, e), float(got[e]), float(want[e])))


def assert_within_the_records_bound(got, want):
    """check_records' bound, in every cell"""
    bad = np.flatnonzero(~(np.abs(got - want) <= 1e-9 * want + 1e-300))
    assert len(bad) == 0, (len(bad), int(bad[0]), float(got[bad[0]]), float(want[bad[0]]))


# ---- the hook: whole tables ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ce.VARIANTS)
@pytest.mark.parametrize("k,w", ce.DYADIC)
def test_tail_table_of_a_dyadic_null_is_exact_in_every_cell(ctx, k, w, variant):
    h = ce.dyadic_histogram(k, w, variant)
    assert_same_table(ctx.compare_tails(h), ce.exact_table(h), w)


@pytest.mark.parametrize("N", ce.DELTA_N)
@pytest.mark.parametrize("pattern", ce.DELTA_PATTERNS)
def test_tail_table_of_deltas_is_one_up_to_the_sum_of_the_bins(ctx, pattern, N):
    h = ce.delta_histogram(pattern, N)
    assert_same_table(ctx.compare_tails(h), ce.delta_table(h), 64)


@pytest.mark.parametrize("k", ce.ONE_COUNT_K)
def test_one_count_at_the_top_down_to_the_denormals(ctx, k):
    """the top cell of every (i0, n) is 2^-(k n), bit for bit: k = 16: 2^-1024 at n = 64, a denormal in the 17th slot;
    k = 32: a denormal at n = 33 and 0 from n = 34 on.  The other cells: the yardstick's, within check_records' bound"""
    h = ce.one_count_histogram(k)
    got = ctx.compare_tails(h)
    for i0 in range(64):
        for n in range(1, 64 - i0 + 1):
            top = got[ce.tail_slice(64, i0, n)][-1]
            assert top.tobytes() == np.float64(ce.one_count_top(k, n)).tobytes(), (i0, n, float(top))
    assert got[ce.tail_slice(64, 0, 64)][-1] == (2.0 ** -1024 if k == 16 else 0.0)
    assert_within_the_records_bound(got, ce.null_table(h))


def test_tail_table_of_a_realistic_null_of_width_64(ctx):
    """all 11.7 M cells: the yardstick's within check_records' bound, in [0, 1], every (i0, n) non-increasing in S and
    exactly 1 up to the smallest sum; and tail(i0, n) of the table is tail(0, n) of the table of h[i0:], bit for bit"""
    h = ce.realistic_histogram()
    got = ctx.compare_tails(h)
    assert len(got) == ce.table_size(64)
    assert_within_the_records_bound(got, ce.null_table(h))
    assert np.all(got >= 0.0) and np.all(got <= 1.0)
    smin = [int(np.flatnonzero(r)[0]) for r in h]
    for i0 in range(64):
        for n in range(1, 64 - i0 + 1):
            t = got[ce.tail_slice(64, i0, n)]
            vmin = sum(smin[i0:i0 + n])
            assert np.all(t[:vmin + 1] == 1.0), (i0, n)
            assert np.all(np.diff(t) <= 0.0), (i0, n, "rises by up to %.3e" % float(np.diff(t).max()))
    assert sum(smin) > 0
    for i0 in (1, 17, 40, 63):
        sub = ctx.compare_tails(h[i0:])
        for n in range(1, 64 - i0 + 1):
            assert sub[ce.tail_slice(64 - i0, 0, n)].tobytes() == got[ce.tail_slice(64, i0, n)].tobytes(), (i0, n)


# ---- the hook against the real path -----------------------------------------------------------------------------------
def realistic_database():
    queries, targets = mc.alignment_case()
    return queries, targets, True


@pytest.mark.parametrize("case", ["n64_both", "realistic"])
def test_the_hooks_table_is_the_table_the_alignments_look_up(ctx, case):
    queries, targets, both = ce.dyadic_database(case) if case != "realistic" else realistic_database()
    hist = ctx.compare_nulls(queries, targets, both)
    align, p = ctx.compare_motifs(queries, targets, both, 1)
    for q, Q in enumerate(queries):
        w = len(Q)
        table = ctx.compare_tails(hist[q, :w])
        for t in range(len(targets)):
            k, o, n, S, _ = (int(v) for v in align[q, t])
            assert table[ce.tail_slice(w, max(k, 0), n)][S].tobytes() == p[q, t].tobytes(), (q, t)


# ---- databases: no near-tie band -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def database_model(name, M):
    queries, targets, both = ce.dyadic_database(name)
    return [mc.compare_query(Q, targets, both, M) for Q in queries]


@pytest.mark.parametrize("M", ce.DB_OVERLAPS)
@pytest.mark.parametrize("name", sorted(ce.DATABASES))
def test_records_of_a_dyadic_database_are_the_models_best(ctx, name, M):
    queries, targets, both = ce.dyadic_database(name)
    align, p = ctx.compare_motifs(queries, targets, both, M)
    for q, rec in enumerate(database_model(name, M)):
        for t in range(len(targets)):
            want = tuple(int(rec[f][t]) for f in ("offset", "orientation", "overlap", "score", "n_offsets"))
            assert tuple(int(v) for v in align[q, t]) == want, (q, t, float(p[q, t]), float(rec["p_offset"][t]))
            assert p[q, t].tobytes() == rec["p_offset"][t].tobytes(), (q, t, float(p[q, t]), float(rec["p_offset"][t]))


def test_all_ones_every_candidate_ties(ctx):
    """every candidate has p = 1: the largest overlap, +, the smallest offset -- out of up to 254 candidates, four trips
    of the lane loop"""
    queries, targets = ce.all_ones_database()
    align, p = ctx.compare_motifs(queries, targets, True, 1)
    for q, Q in enumerate(queries):
        for t, wt in enumerate(ce.ALL_ONES_WIDTHS):
            assert tuple(int(v) for v in align[q, t]) == ce.all_ones_record(Q, wt), (len(Q), wt)
            assert p[q, t].tobytes() == np.float64(1.0).tobytes()


# ---- the host plan's seams -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("total", ce.CHUNK_SEAMS)
def test_null_histograms_at_the_database_columns_around_a_chunk(ctx, total, both):
    rng = np.random.default_rng(2000 + total)
    targets = ce.columns_database(rng, total)
    queries = [mc.random_motif(rng, 1), mc.random_motif(rng, 64), mc.random_motif(rng, 17)]
    got = ctx.compare_nulls(queries, targets, both)
    for m, Q in enumerate(queries):
        assert got[m].tobytes() == padded(mc.null_histograms(Q, targets, both), len(Q)).tobytes(), m
        assert int(got[m, 0].sum()) == total * (2 if both else 1)


def test_a_chunk_of_identical_columns_fills_one_bin_to_16384(ctx):
    """8192 columns equal to the query's, which is its own letter reversal: both orientations of one workgroup's chunk land
    in bin 256, 16 384 in one 32-bit LDS bin"""
    col = ce.ALPHABET[1:2]
    targets = [np.repeat(col, 64, axis=0)] * 128
    for extra, n in (([], 8192), ([col.copy()], 8193)):
        got = ctx.compare_nulls([col.copy(), np.repeat(col, 64, axis=0)], targets + extra, True)
        assert got[0, 0, 256] == 2 * n and got[0].sum() == 2 * n
        assert np.all(got[1, :, 256] == 2 * n) and got[1].sum() == 64 * 2 * n
    assert 2 * 8192 == 16384


def test_a_batch_of_4096_queries_and_one_more(ctx):
    """4097 queries: query 4096 opens a second batch.  The sampled queries' records equal those of a call with the query
    alone, bit for bit, and the model's"""
    queries, targets = ce.batch_case()
    align, p = ctx.compare_motifs(queries, targets, True, 1)
    assert align.shape == (ce.BATCH_QUERIES, 3, 5)
    for q in ce.BATCH_SAMPLE:
        a1, p1 = ctx.compare_motifs(queries[q:q + 1], targets, True, 1)
        assert a1[0].tobytes() == align[q].tobytes() and p1[0].tobytes() == p[q].tobytes(), q
        check_records(align[q], p[q], mc.compare_query(queries[q], targets, True, 1))


def test_a_batch_that_ends_between_queries_of_different_widths(ctx):
    """widths 64, 64, 7, 64, 3: the tails of the first three fill the budget, the second batch is (64, 3)"""
    queries, targets = ce.mixed_width_case()
    align, p = ctx.compare_motifs(queries, targets, True, 5)
    for q in range(len(queries)):
        a1, p1 = ctx.compare_motifs(queries[q:q + 1], targets, True, 5)
        assert a1[0].tobytes() == align[q].tobytes() and p1[0].tobytes() == p[q].tobytes(), q
    check_records(align[4], p[4], mc.compare_query(queries[4], targets, True, 5))
    check_records(align[2], p[2], mc.compare_query(queries[2], targets, True, 5))


# ---- the hook's argument errors ------------------------------------------------------------------------------------------
def test_the_hooks_argument_errors_leave_the_context_usable(ctx):
    good = ce.dyadic_histogram(6, 8, "random")
    want = ce.exact_table(good)

    def refused(what, hist, w=None):
        with pytest.raises(pk.PengkError) as e:
            ctx.compare_tails(hist, w)
        assert e.value.code == pk.ERR_ARG and "pengk_test_compare_tails" in str(e.value) and what in str(e.value), str(e.value)
        assert_same_table(ctx.compare_tails(good), want, 8)

    unequal = good.copy()
    unequal[5, 256] += 1
    refused("row 5", unequal)
    refused("sum to 0", np.zeros((3, ce.BINS), np.uint64))
    over = np.zeros((2, ce.BINS), np.uint64)
    over[:, 7] = 2 ** 32 + 1
    refused("2^32", over)
    wrap = np.zeros((1, ce.BINS), np.uint64)
    wrap[0, :2] = 2 ** 63  # (sums to 0 in 64 bits)
    refused("2^32", wrap)
    refused("w = 0", good, w=0)
    refused("w = 65", np.repeat(good, 8, axis=0), w=65)
    L = pk.lib()
    out = np.zeros(ce.table_size(8), np.float64)
    assert L.pengk_test_compare_tails(ctx.h, 8, None, out.ctypes.data) == pk.ERR_ARG
    assert L.pengk_test_compare_tails(ctx.h, 8, good.ctypes.data, None) == pk.ERR_ARG
    assert_same_table(ctx.compare_tails(good), want, 8)
