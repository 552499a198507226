"""The cases of tests/compare_edges_model.py held to their classes, without a device: the yardstick
(motif_compare_model.NullTails) equals integer arithmetic bit for bit on every dyadic and delta histogram and on every
alignment of the dyadic databases; those databases have the bit-equal ties the GPU module relies on; the all-ones records
are the model's; and the yardstick's distance from exact rational arithmetic on nulls that are not dyadic, which
check_records' docstring derives and nothing had measured."""
import fractions
import functools

import numpy as np
import pytest

import compare_edges_model as ce
import motif_compare_model as mc
import peng_motif_amd as pk


def same_bits(a, b):
    return a.dtype == b.dtype == np.float64 and a.tobytes() == b.tobytes()


# ---- the order of the table ---------------------------------------------------------------------------------------------
def test_table_layout():
    assert ce.table_size(1) == 257 and ce.table_size(2) == 257 + 513 + 257 and ce.table_size(64) == 11716640
    assert ce.table_size(64) * 8 > 92e6
    for w in (1, 2, 7, 64):
        at = 0
        for i0 in range(w):
            for n in range(1, w - i0 + 1):
                s = ce.tail_slice(w, i0, n)
                assert s.start == at and s.stop - s.start == 256 * n + 1
                at = s.stop
        assert at == ce.table_size(w) == sum(pk.compare_tails_before(w - i0 + 1) for i0 in range(w))
    assert [ce.tails_before(n) for n in (1, 2, 3)] == [pk.compare_tails_before(n) for n in (1, 2, 3)] == [0, 257, 770]


# ---- histograms: the yardstick is exact on them -------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ce.VARIANTS)
@pytest.mark.parametrize("k,w", ce.DYADIC)
def test_dyadic_histograms_are_exact_in_every_cell(k, w, variant):
    h = ce.dyadic_histogram(k, w, variant)
    assert h.shape == (w, ce.BINS) and np.all(h.sum(axis=1) == 2 ** k) and k * w <= 52
    assert np.all(np.count_nonzero(h, axis=1) <= min(2 ** k, 40))
    if variant == "ends":
        assert np.all(h[:, 0] > 0) and np.all(h[:, 256] > 0)
    if variant == "lifted":
        assert np.all(h[:, 0] == 0) and sum(ce.ExactTails(h).smin) >= w
    assert same_bits(mc.NullTails(h).tail(0, w), ce.ExactTails(h).expected(0, w))
    assert same_bits(ce.null_table(h), ce.exact_table(h))


def test_the_required_dyadic_case_and_its_top_cell():
    h = ce.dyadic_histogram(1, 52, "ends")
    assert np.count_nonzero(h) == 104 and np.all(h[:, 0] == 1) and np.all(h[:, 256] == 1)
    t = ce.ExactTails(h).expected(0, 52)
    assert len(t) - 1 == 13 * 1024 and t[-1] == 2.0 ** -52 and t[-257] == 53 * 2.0 ** -52 and t[0] == 1.0


def test_exact_tails_is_the_integer_convolution():
    h = ce.dyadic_histogram(6, 8, "random")
    count, D, vmin = ce.ExactTails(h).tail(2, 3)
    pmf = np.zeros(3 * 256 + 1, object)
    for a in np.flatnonzero(h[2]):
        for b in np.flatnonzero(h[3]):
            for c in np.flatnonzero(h[4]):
                pmf[a + b + c] += int(h[2, a]) * int(h[3, b]) * int(h[4, c])
    assert D == 64 ** 3 and [int(v) for v in count] == [sum(pmf[s:]) for s in range(len(pmf))]
    assert vmin == min(np.flatnonzero(pmf)) and count[vmin] == D and (vmin == len(pmf) - 1 or count[vmin + 1] < D)
    rng = np.random.default_rng(1)
    cur = rng.integers(0, 2 ** 20, size=700)
    for bins in (1, 16, 17, 257):
        col = np.zeros(ce.BINS, np.int64)
        col[rng.choice(ce.BINS, size=bins, replace=False)] = rng.integers(1, 2 ** 20, size=bins)
        assert np.array_equal(ce.int_convolve(cur, col), np.convolve(cur, col))


@pytest.mark.parametrize("N", ce.DELTA_N)
@pytest.mark.parametrize("pattern", ce.DELTA_PATTERNS)
def test_delta_histograms_are_one_up_to_the_sum_of_their_bins(pattern, N):
    h = ce.delta_histogram(pattern, N)
    want = ce.delta_table(h)
    assert set(np.unique(want)) <= {0.0, 1.0} and same_bits(ce.null_table(h), want)
    bins = ce.delta_bins(h)
    top = want[ce.tail_slice(64, 0, 64)]
    assert top[sum(bins)] == 1.0 and (sum(bins) == 16384 or top[sum(bins) + 1] == 0.0)
    if pattern == "all256":
        assert len(top) == 16 * 1024 + 1 and np.all(top == 1.0)  # (v = 16384: the 17th slot of thread 0)
    if pattern == "mix":
        assert len(set(bins)) == 5
    if N == 1:  # (the counts fit an int64: the closed form is the integer convolution's)
        assert same_bits(ce.exact_table(h), want)


@pytest.mark.parametrize("k", ce.ONE_COUNT_K)
def test_one_count_at_the_top_is_a_chain_of_exact_products(k):
    h = ce.one_count_histogram(k)
    nt = mc.NullTails(h)
    tops = [float(nt.tail(0, n)[-1]) for n in range(1, 65)]
    assert tops == [ce.one_count_top(k, n) for n in range(1, 65)]
    if k == 16:
        assert tops[63] == 2.0 ** -1024 and 0 < tops[63] < np.finfo(np.float64).tiny
    else:
        assert tops[32] == 2.0 ** -1056 > 0 and tops[33] == 0.0 and all(t > 0 for t in tops[:33])
    assert nt.tail(5, 3)[-1] == ce.one_count_top(k, 3)


def test_the_realistic_histogram():
    h = ce.realistic_histogram()
    N = int(h[0].sum())
    assert h.shape == (64, ce.BINS) and N == 140000 and N & (N - 1) and np.all(h.sum(axis=1) == N)


# ---- the yardstick's distance from exact arithmetic ---------------------------------------------------------------------
def test_the_yardstick_is_within_4e_12_of_exact_rational_arithmetic(capsys):
    """check_records derives: with at most 64 levels of at most 257 non-negative products and a tail of at most 16 385
    terms, either side is within a relative 4e-12 of the exact value.  Held here in every cell of non-dyadic nulls of
    w <= 6 against Python integers; below 1e-290 the absolute 1e-300 of check_records takes over.
    Measured: worst relative difference 1.6e-15 (N = 1000) and 1.7e-15 (N = 139 999)."""
    worst = {}
    for N, h in ce.yardstick_histograms():
        w = len(h)
        assert int(h[0].sum()) == N and N & (N - 1)
        nt = mc.NullTails(h)
        hi = [[int(v) for v in r] for r in h]
        for i0 in range(w):
            cur = None
            for n in range(1, w - i0 + 1):
                col = hi[i0 + n - 1]
                if cur is None:
                    cur = list(col)
                else:
                    new = [0] * (len(cur) + 256)
                    for u, c in enumerate(col):
                        if c:
                            for v, x in enumerate(cur):
                                if x:
                                    new[u + v] += x * c
                    cur = new
                D = N ** n
                assert sum(cur) == D
                vmin = sum(nt.smin[i0:i0 + n])
                got = nt.tail(i0, n)
                run = 0
                for S in range(len(cur) - 1, -1, -1):
                    run += cur[S]
                    exact = fractions.Fraction(run, D)
                    err = abs(fractions.Fraction(float(got[S])) - exact)
                    if S <= vmin:
                        assert run == D and got[S] == 1.0
                    elif exact >= fractions.Fraction(1e-290):
                        rel = float(err / exact)
                        worst[N] = max(worst.get(N, 0.0), rel)
                        assert rel <= 4e-12, (N, i0, n, S, float(exact), float(got[S]))
                    else:
                        assert err <= fractions.Fraction(1e-300), (N, i0, n, S)
    with capsys.disabled():
        for N in sorted(worst):
            print("\nNullTails against exact rationals, N = %d: worst relative difference %.3e" % (N, worst[N]))


# ---- databases ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def database_model(name, M):
    queries, targets, both = ce.dyadic_database(name)
    return [mc.compare_query(Q, targets, both, M) for Q in queries]


def tie_counts(name, M):
    """(pairs, tied, by_overlap, by_orientation, by_offset) of a database's pairs"""
    out = [0] * 5
    for rec in database_model(name, M):
        for al in rec["all"]:
            tied, by_n, by_o, by_k = ce.tie_stages(al)
            out[0] += 1
            out[1] += tied > 1
            out[2] += by_n
            out[3] += by_o
            out[4] += by_k
    return out


def test_the_alphabet():
    A = ce.ALPHABET
    assert np.array_equal(A[0], A[0][::-1]) and len(set(A[0])) == 1 and np.array_equal(A[1], A[1][::-1])
    assert np.array_equal(A[2][::-1], A[3]) and not np.array_equal(A[4], A[4][::-1])
    s = mc.column_scores(A, A)
    assert np.all(np.diag(s) == 256) and len(np.unique(s)) >= 5


@pytest.mark.parametrize("M", ce.DB_OVERLAPS)
@pytest.mark.parametrize("name", sorted(ce.DATABASES))
def test_dyadic_databases_have_exact_p_and_bit_equal_ties(name, M, capsys):
    queries, targets, both = ce.dyadic_database(name)
    assert [len(q) for q in queries] == list(ce.DB_QUERY_WIDTHS)
    for Q, rec in zip(queries, database_model(name, M)):
        ex = ce.ExactTails(mc.null_histograms(Q, targets, both))
        assert ex.N in (64, 256) and ex.N == sum(len(t) for t in targets) * (2 if both else 1)
        for t, al in enumerate(rec["all"]):
            for a in al:
                i0 = max(a["offset"], 0)
                want = ex.expected(i0, a["overlap"])[a["score"]]
                assert np.float64(a["p"]).tobytes() == np.float64(want).tobytes(), (t, a)
    pairs, tied, by_n, by_o, by_k = tie_counts(name, M)
    with capsys.disabled():
        print("\n%s, M = %d: %d of %d pairs tie at the best p; decided by overlap %d, orientation %d, offset %d"
              % (name, M, tied, pairs, by_n, by_o, by_k))
    assert pairs == len(queries) * len(targets) and 4 * tied >= pairs
    assert by_k >= 1
    if both:
        assert by_o >= 1


@pytest.mark.parametrize("wq", ce.ALL_ONES_WIDTHS)
def test_all_ones_every_candidate_ties_and_the_closed_form_is_the_models(wq):
    queries, targets = ce.all_ones_database()
    Q = queries[ce.ALL_ONES_WIDTHS.index(wq)]
    rec = mc.compare_query(Q, targets, True, 1)
    for t, wt in enumerate(ce.ALL_ONES_WIDTHS):
        al = rec["all"][t]
        assert all(a["p"] == 1.0 for a in al) and len(al) == 2 * (wq + wt - 1)
        got = tuple(int(rec[k][t]) for k in ("offset", "orientation", "overlap", "score", "n_offsets"))
        assert got == ce.all_ones_record(Q, wt), (wq, wt)
        tied, by_n, by_o, by_k = ce.tie_stages(al)
        assert tied == len(al) and by_o and by_n == (min(wq, wt) > 1) and by_k == (wq != wt)
    assert ce.all_ones_record(queries[0], 64)[4] == 254  # (four trips of the lane loop)
    assert ce.all_ones_record(queries[1], 64)[:3] == (-54, 0, 10) and ce.all_ones_record(queries[0], 10)[:3] == (0, 0, 10)


def test_the_seam_cases():
    queries, targets = ce.batch_case()
    assert len(queries) == 4097 and [len(q) for q in queries[:4]] == [1, 2, 1, 2] and len(targets) == 3
    assert set(ce.BATCH_SAMPLE) >= {0, 1, 4095, 4096} and len(set(ce.BATCH_SAMPLE)) == 14
    queries, targets = ce.mixed_width_case()
    assert [len(q) for q in queries] == [64, 64, 7, 64, 3]


# ---- the hook's argument errors that need no device ---------------------------------------------------------------------
def test_the_hook_refuses_null_arguments_before_it_touches_the_device():
    h = np.zeros((1, ce.BINS), np.uint64)
    h[0, 0] = 1
    out = np.zeros(257, np.float64)
    L = pk.lib()
    for args in ((None, 1, h.ctypes.data, out.ctypes.data),):
        assert L.pengk_test_compare_tails(*args) == pk.ERR_ARG
        assert b"pengk_test_compare_tails" in L.pengk_last_error() and b"NULL" in L.pengk_last_error()
