"""--compare on the device (csrc/compare.hip) against tests/motif_compare_model.py: the null histograms byte for byte,
every alignment record (integers exactly, p_offset to a derived tolerance), constructed pairs, the argument errors, and
the CLI's TSV against the model's rendering, beside the other outputs and over two ranks."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import peng_motif_amd as pk
import motif_compare_model as mc
from test_gpu_multirank import CLI, clean_env, run_plain, run_ranks

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ctx():
    c = pk.Context(0)
    yield c
    c.close()


def padded(h, w):
    """the model's w x 257 histogram as a row of the device's n_q x 64 x 257 array"""
    out = np.zeros((pk.MAX_MOTIF_LEN, mc.BINS), np.uint64)
    out[:w] = h
    return out


# ---- null histograms: integers, byte for byte --------------------------------------------------------------------------
def columns_database(rng, total):
    """motifs of random widths up to 64 with `total` columns in all"""
    out = []
    while total:
        w = min(total, int(rng.integers(1, 65)))
        out.append(mc.random_motif(rng, w))
        total -= w
    return out


@functools.lru_cache(maxsize=None)
def large():
    return mc.large_case()


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("total", [1, 63, 64, 65, 255, 256, 257])
def test_null_histograms_at_the_column_counts_around_a_wave_and_a_block(ctx, total, both):
    rng = np.random.default_rng(1000 + total)
    targets = columns_database(rng, total)
    queries = [mc.random_motif(rng, 1), mc.random_motif(rng, 64), mc.random_motif(rng, 17)]
    got = ctx.compare_nulls(queries, targets, both)
    for m, Q in enumerate(queries):
        assert got[m].tobytes() == padded(mc.null_histograms(Q, targets, both), len(Q)).tobytes(), m
        assert int(got[m, 0].sum()) == total * (2 if both else 1)


@pytest.mark.parametrize("both", [False, True])
def test_null_histograms_of_a_large_database(ctx, both):
    """about 70 000 columns: nine workgroups' bins meet in one 64-bit count"""
    q, targets, _ = large()
    queries = [q, q[:1]]
    got = ctx.compare_nulls(queries, targets, both)
    for m, Q in enumerate(queries):
        assert got[m].tobytes() == padded(mc.null_histograms(Q, targets, both), len(Q)).tobytes()


@pytest.mark.parametrize("both", [False, True])
def test_null_histograms_of_identical_columns_land_in_one_bin(ctx, both):
    col = np.array([[2048, 1024, 512, 512]], np.int16)
    targets = [np.repeat(col, 64, axis=0)] * 150 + [np.repeat(col, 37, axis=0)]  # 9637 columns: two chunks
    queries = [col.copy(), np.repeat(col[:, ::-1], 64, axis=0)]
    got = ctx.compare_nulls(queries, targets, both)
    n = 150 * 64 + 37
    for m, Q in enumerate(queries):
        want = mc.null_histograms(Q, targets, both)
        assert got[m].tobytes() == padded(want, len(Q)).tobytes()
        assert np.count_nonzero(got[m, 0]) == (2 if both else 1) and int(got[m, 0].max()) == n
    assert got[0, 0, 256] == n


def four_squares(d):
    """(a, b, c, e), each at most 4096, with a^2 + b^2 + c^2 + e^2 = d"""
    for a in range(min(math.isqrt(d), 4096), -1, -1):
        for b in range(min(math.isqrt(d - a * a), a), -1, -1):
            r = d - a * a - b * b
            for c in range(min(math.isqrt(r), b), -1, -1):
                e = math.isqrt(r - c * c)
                if e <= c and e * e == r - c * c:
                    return a, b, c, e
                if c * c * 2 < r:
                    break
    raise AssertionError(d)


def test_null_histograms_at_the_edges_of_the_score_bins(ctx):
    """column pairs with d = k 2^17 - 1 (the last d that scores 257 - k) and d = k 2^17 (the first that scores 256 - k);
    two different pure columns: d = 2^25, s = 0"""
    zero = np.zeros((1, 4), np.int16)
    for k in (1, 128, 255, 256):
        for d, s in ((k * 2 ** 17 - 1, 257 - k), (k * 2 ** 17, 256 - k)):
            x = np.array([four_squares(d)], np.int16)
            assert int((x.astype(np.int64) ** 2).sum()) == d and mc.column_scores(x, zero)[0, 0] == s
            for query, target in ((x, zero), (zero, x), (x[:, ::-1].copy(), zero)):
                got = ctx.compare_nulls([query], [target], False)
                assert got[0, 0, s] == 1 and got.sum() == 1, (k, d, s)
    pure = np.eye(4, dtype=np.int16) * 4096
    got = ctx.compare_nulls([pure[:1]], [pure[1:2], pure[:1]], True)
    assert got[0, 0, 0] == 3 and got[0, 0, 256] == 1 and got.sum() == 4  # (A against C, G, T and A)
    got = ctx.compare_nulls([np.full((1, 4), 4096, np.int16)], [zero], True)  # (d = 2^26: clamped to s = 0)
    assert got[0, 0, 0] == 2 and got.sum() == 2


# ---- alignments ------------------------------------------------------------------------------------------------------------
def check_records(align, p, rec, targets=None):
    """one query's device records against the model's compare_query: n_offsets; the score of the alignment the device
    reports; p_offset with |dev - model| <= 1e-9 model + 1e-300 -- every term of either side is non-negative, so with at
    most 64 levels of at most 257 products and a tail of at most 16 385 terms either side is within a relative 4e-12 of the
    exact value, and 1e-9 leaves a hundredfold margin; the absolute term covers underflow --; and the alignment itself: the
    model's, unless the model has a near tie, when it must lie in that band."""
    for t in (range(len(align)) if targets is None else targets):
        k, o, n, S, noff = (int(v) for v in align[t])
        al = rec["all"][t]
        assert noff == len(al) == rec["n_offsets"][t], t
        mine = [a for a in al if a["offset"] == k and a["orientation"] == o]
        assert len(mine) == 1, (t, k, o)
        assert (n, S) == (mine[0]["overlap"], mine[0]["score"]), (t, k, o)
        assert abs(p[t] - mine[0]["p"]) <= 1e-9 * mine[0]["p"] + 1e-300, (t, p[t], mine[0]["p"])
        best = (int(rec["offset"][t]), int(rec["orientation"][t]))
        if (k, o) != best:
            assert mine[0] in rec["near"][t], (t, (k, o), best, p[t], rec["p_offset"][t])


@functools.lru_cache(maxsize=None)
def alignment_model(M):
    queries, targets = mc.alignment_case()
    return [mc.compare_query(Q, targets, True, M) for Q in queries]


@pytest.mark.parametrize("M", mc.ALIGN_OVERLAPS)
def test_alignments_of_every_pair_of_widths(ctx, M):
    """(wq, wt) in {1, 4, 5, 6, 13, 63, 64}^2 (the targets of those widths lead the database), both orientations"""
    queries, targets = mc.alignment_case()
    align, p = ctx.compare_motifs(queries, targets, True, M)
    for m, rec in enumerate(alignment_model(M)):
        check_records(align[m], p[m], rec)
        for t, wt in enumerate(mc.ALIGN_WIDTHS):
            assert align[m, t, 4] == mc.n_offsets(len(queries[m]), wt, True, M)


@pytest.mark.parametrize("both", [True, False])
def test_constructed_pairs(ctx, both):
    queries, targets, names = mc.constructed_case()
    align, p = ctx.compare_motifs(queries, targets, both, 5)
    recs = [mc.compare_query(Q, targets, both, 5) for Q in queries]
    for m in range(2):
        check_records(align[m], p[m], recs[m])
    at = {n: align[0, names.index(n)].tolist() for n in mc.CONSTRUCTED}
    # the palindrome scores the same in both orientations at every offset: bit-equal p, + is reported (for both queries;
    # query 1 is cut out of it)
    assert at["palindrome"][1] == 0 and align[1, names.index("palindrome")].tolist()[:4] == [-3, 0, 9, 9 * 256]
    if both:
        assert at["revcomp"][:4] == [0, 1, 12, 12 * 256]
    else:
        assert at["revcomp"][1] == 0
    assert at["wide"][:4] == [-4, 0, 12, 12 * 256] and at["core"][:4] == [3, 0, 8, 8 * 256]
    a, b = names.index("twin_a"), names.index("twin_b")
    for m in range(2):
        assert align[m, a].tobytes() == align[m, b].tobytes() and p[m, a].tobytes() == p[m, b].tobytes()
    # one orientation: half the offsets
    assert at["wide"][4] == (2 if both else 1) * (12 + 18 - 10 + 1)


def test_a_database_of_one_target(ctx):
    queries, targets, _ = mc.constructed_case()
    for t in (2, 0, 7):
        for both in (True, False):
            align, p = ctx.compare_motifs(queries, [targets[t]], both, 5)
            for m, Q in enumerate(queries):
                check_records(align[m], p[m], mc.compare_query(Q, [targets[t]], both, 5))


def test_self_match_of_width_64_and_more_than_one_batch(ctx):
    """three queries of width 64 need 3 x 92 MB of tails: two batches.  Query 0 against itself: the full overlap, a p_offset
    far below anything a float would hold; every record of query 0 against the model; the batched records equal to the
    records of one call per query, bit for bit."""
    queries, targets = mc.self_match_case()
    align, p = ctx.compare_motifs(queries, targets, True, 5)
    rec = mc.compare_query(queries[0], targets, True, 5)
    check_records(align[0], p[0], rec)
    assert align[0, -1].tolist() == [0, 0, 64, 64 * 256, 2 * (64 + 64 - 10 + 1)]
    print("p_offset of the width-64 self-match: device %.6e, model %.6e" % (p[0, -1], rec["p_offset"][-1]))
    assert 0 < p[0, -1] < 1e-100
    for m in range(3):
        a1, p1 = ctx.compare_motifs(queries[m:m + 1], targets, True, 5)
        assert a1[0].tobytes() == align[m].tobytes() and p1[0].tobytes() == p[m].tobytes(), m


def test_self_match_in_a_large_database_underflows(ctx):
    q, targets, checked = large()
    align, p = ctx.compare_motifs([q], targets, True, 5)
    rec = mc.compare_query(q, targets, True, 5, only=checked)
    check_records(align[0], p[0], rec, targets=checked)
    assert align[0, 100].tolist()[:4] == [0, 0, 64, 64 * 256]
    print("p_offset of the self-match among 70 000 columns: device %.6e, model %.6e" % (p[0, 100], rec["p_offset"][100]))
    assert p[0, 100] <= 1e-300 and np.all(p[0] >= 0) and np.all(p[0] <= 1)
    assert np.array_equal(align[0, :, 4], [2 * (64 + len(t) - 2 * min(5, len(t)) + 1) for t in targets])


# ---- argument errors ---------------------------------------------------------------------------------------------------------
def test_argument_errors(ctx):
    q = [np.full((8, 4), 1024, np.int16)]
    t = [np.full((6, 4), 1024, np.int16)]

    def refused(who, what, **kw):
        args = {"queries": q, "targets": t, "both": True}
        args.update(kw)
        calls = {"pengk_compare_nulls": ctx.compare_nulls, "pengk_compare_motifs": ctx.compare_motifs}
        with pytest.raises(pk.PengkError) as e:
            calls[who](**args)
        assert e.value.code == pk.ERR_ARG and who in str(e.value) and what in str(e.value), str(e.value)

    bad_hi, bad_lo = q[0].copy(), t[0].copy()
    bad_hi[3, 2] = 4097
    bad_lo[5, 0] = -1
    for who in ("pengk_compare_nulls", "pengk_compare_motifs"):
        refused(who, "h_qlen", qlens=[0])
        refused(who, "h_qlen", qlens=[65])
        refused(who, "h_tlen", tlens=[0])
        refused(who, "h_tlen", tlens=[65])
        refused(who, "h_QX", queries=[bad_hi])
        refused(who, "h_TX", targets=[bad_lo])
        refused(who, "n_q", queries=[])
        refused(who, "n_t", targets=[])
    refused("pengk_compare_motifs", "min_overlap", min_overlap=0)
    # entries behind a motif's width are not read
    wide = np.full((8, 4), 9999, np.int16)
    wide[:2] = 1024
    align, p = ctx.compare_motifs([wide], t, True, 1, qlens=[2])
    assert align[0, 0, 4] == 2 * (2 + 6 - 2 + 1)
    with pytest.raises(pk.PengkError) as e:
        pk.compare_summary([0.5], [0])
    assert e.value.code == pk.ERR_ARG and "pengk_compare_summary" in str(e.value)


# ---- the CLI -------------------------------------------------------------------------------------------------------------------
def planted_db(tmp_path):
    names, rows = mc.planted_database()
    db = tmp_path / "planted.meme"
    mc.write_meme(db, names, rows)
    return str(db), names, [mc.quantize(r) for r in rows]


def read_queries(path):
    """PENGK_COMPARE_QUERIES' dump: (iupacs, quantised matrices)"""
    iupacs, mats = [], []
    lines = open(path).read().split("\n")
    i = 0
    while i < len(lines) and lines[i]:
        idx, w, iupac = lines[i].split()
        assert int(idx) == len(mats) + 1
        iupacs.append(iupac)
        mats.append(np.array([[int(x) for x in l.split()] for l in lines[i + 1:i + 1 + int(w)]], np.int16))
        i += 1 + int(w)
    return iupacs, mats


def assert_same_tsv(got, want):
    """strings and integers exactly; the floats (printed with %.6e) to the tolerance of check_records plus one unit of the
    last printed digit, 1e-6 relative: two doubles 1e-9 apart can round to neighbouring 7-digit decimals"""
    g, w = got.split("\n"), want.split("\n")
    assert g[0] == w[0] and len(g) == len(w), (len(g), len(w))
    for a, b in zip(g[1:], w[1:]):
        fa, fb = a.split("\t"), b.split("\t")
        assert fa[:9] == fb[:9], (a, b)
        for x, y in zip(fa[9:], fb[9:]):
            assert abs(float(x) - float(y)) <= (1e-9 + 1e-6) * float(y) + 1e-300, (a, b)


def test_cli_writes_the_models_table_and_changes_no_other_output(tmp_path):
    fa = os.path.join(GOLD, "MafK.fasta")
    db, names, targets = planted_db(tmp_path)
    rc, so0, se, meme0, js0 = run_plain([fa, "-w", "10"], tmp_path, tag="a")
    assert rc == 0, se.decode()[-2000:]
    out, dump = tmp_path / "c.tsv", tmp_path / "queries.txt"
    rc, so1, se, meme1, js1 = run_plain([fa, "-w", "10", "--compare", str(out), "--compare-db", db], tmp_path, tag="b",
                                        extra_env={"PENGK_COMPARE_QUERIES": str(dump)})
    assert rc == 0, se.decode()[-2000:]
    assert (so1, meme1, js1) == (so0, meme0, js0)
    iupacs, queries = read_queries(dump)
    assert iupacs == ["CTGASTCAGCAAW", "GTCAGCAWTTTT"] and [len(q) for q in queries] == [13, 12]
    got = out.read_text()
    assert_same_tsv(got, mc.render(queries, iupacs, targets, names, True))
    lines = [l.split("\t") for l in got.split("\n")[1:] if l]
    assert lines[0][:7] == ["1", "CTGASTCAGCAAW", "MARE", "13", "-2", "+", "11"] and lines[1][2] == "AP1"
    assert all(float(l[11]) <= 1.0 for l in lines)
    # --compare-evalue filters lines, --compare-min-overlap and --strand PLUS reach the device
    strict, plus = tmp_path / "strict.tsv", tmp_path / "plus.tsv"
    rc, _, se, _, _ = run_plain([fa, "-w", "10", "--compare", str(strict), "--compare-db", db, "--compare-evalue", "1e-5",
                                 "--compare-min-overlap", "7"], tmp_path, tag="c")
    assert rc == 0, se.decode()[-2000:]
    want = mc.render(queries, iupacs, targets, names, True, M=7, E=1e-5)
    assert_same_tsv(strict.read_text(), want)
    assert 2 <= len(want.split("\n")) - 2 < len(lines)
    rc, so2, se, meme2, js2 = run_plain([fa, "-w", "10", "--strand", "PLUS", "--compare", str(plus), "--compare-db", db], tmp_path,
                                        tag="d", extra_env={"PENGK_COMPARE_QUERIES": str(dump)})
    assert rc == 0, se.decode()[-2000:]
    iupacs, queries = read_queries(dump)
    got = plus.read_text()
    assert_same_tsv(got, mc.render(queries, iupacs, targets, names, False))
    assert all(l.split("\t")[5] == "+" for l in got.split("\n")[1:] if l)


def test_cli_two_ranks_write_what_one_process_writes(tmp_path):
    fa = os.path.join(GOLD, "MafK.fasta")
    db, _, _ = planted_db(tmp_path)
    one, many = tmp_path / "one.tsv", tmp_path / "many.tsv"
    rc, so, se, meme, js = run_plain([fa, "-w", "10", "--compare", str(one), "--compare-db", db], tmp_path)
    assert rc == 0, se.decode()[-2000:]
    res = run_ranks([fa, "-w", "10", "--compare", str(many), "--compare-db", db], 2, tmp_path)
    for rank, (rrc, rso, rse, rmeme, rjs) in enumerate(res):
        assert rrc == 0, (rank, rse.decode()[-2000:])
    assert (res[0][1], res[0][3], res[0][4]) == (so, meme, js) and res[1][1] == b""
    assert many.read_bytes() == one.read_bytes()


def run_args_last(args, tmp_path):
    """the flags under test behind -o / -j, so that a flag without its value is the last argument"""
    r = subprocess.run([CLI, os.path.join(GOLD, "MafK.fasta"), "-w", "10", "-o", str(tmp_path / "e.meme"), "-j", str(tmp_path / "e.json")]
                       + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=clean_env(), timeout=900)
    return r.returncode, r.stdout, r.stderr


@pytest.mark.parametrize("args", [["--compare", "c.tsv"], ["--compare-db", "DB"], ["--compare", "c.tsv", "--compare-db"],
                                  ["--compare", "c.tsv", "--compare-db", "DB", "--compare-evalue", "-1"],
                                  ["--compare", "c.tsv", "--compare-db", "DB", "--compare-evalue", "1x"],
                                  ["--compare", "c.tsv", "--compare-db", "DB", "--compare-min-overlap", "0"],
                                  ["--compare", "c.tsv", "--compare-db", "DB", "--compare-min-overlap", "65"]],
                         ids=lambda a: "_".join(a).replace("--", ""))
def test_cli_argument_errors_exit_4(tmp_path, args):
    """as --dinuc's: the help, an ERROR line, exit 4 (before the input is read: no device is needed for it)"""
    db, _, _ = planted_db(tmp_path)
    args = [str(tmp_path / a) if a.endswith(".tsv") else db if a == "DB" else a for a in args]
    rc, so, se = run_args_last(args, tmp_path)
    assert rc == 4 and b"ERROR" in se and b"--compare FILE" in so
    assert not list(tmp_path.glob("*.tsv")) and not (tmp_path / "e.meme").exists()


@pytest.mark.parametrize("text", [None, "MEME version 4\n\n", "MOTIF a\nletter-probability matrix: alength= 4\n1 0 0 0\n",
                                  "MOTIF a\nletter-probability matrix: w= 1\n0 0 0 0\n"],
                         ids=["missing", "no_motif", "no_w", "zero_row"])
def test_cli_refuses_a_database_it_cannot_use(tmp_path, text):
    db = tmp_path / "bad.meme"
    if text is not None:
        db.write_text(text)
    rc, so, se = run_args_last(["--compare", str(tmp_path / "c.tsv"), "--compare-db", str(db)], tmp_path)
    assert rc == 4 and b"ERROR: --compare-db: motif database" in se and b"bad.meme" in se
    assert not (tmp_path / "c.tsv").exists() and not (tmp_path / "e.meme").exists()
