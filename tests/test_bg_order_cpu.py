"""The Markov null of order K <= 5 on the CPU (tests/bg_order_model.py): pengk_bg_model_order against the numpy model bit
for bit and, at K <= 2, against the oracle's V; the model's counters at orders <= 2 against the oracle's; and the definition
doing what it is for on the scenario of the README's table -- 20 000 x 100 bp of a random order-4 chain: against the order-2
null hundreds of seeds are the chain's own words, against the order-4 null none is, and a planted motif leaves seeds that
all hold a 6-mer of it.  (Figures of the model at W = 8, both strands, seeds 1 / 2 / 3: README, "a Markov null of order
3 .. 5".)"""
import os
import subprocess

import numpy as np
import pytest

import bg_order_model as bm
import control_stats_model as cm
import peng_motif_amd as pk
import table_edges_model as tm
from oracle import oracle as po


def test_symbols_and_bindings():
    for name in ("pengk_bg_count_order", "pengk_bg_model_order", "pengk_pattern_stats_order"):
        assert hasattr(pk.lib(), name) and name in pk.EXPORTS
    assert [bm.at(k) for k in range(7)] == [0, 4, 20, 84, 340, 1364, 5460]
    assert pk.order_table_size(5) == bm.size(5) == 5460


# ---- the model --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [0, 1, 2, 3, 4, 5])
def test_model_entry_has_the_numpy_models_bits(K):
    n_cases = 0
    for kind in bm.COUNTER_KINDS:
        n = bm.counters(kind, K, seed=K)
        if kind == "zero_contexts" and K:
            assert (n[bm.at(K):].reshape(-1, 4).sum(axis=1) == 0).any()
        if kind == "near_2_24":
            assert n[bm.at(K):].min() >= 2 ** 24 - 3 and n[bm.at(K):].max() <= 2 ** 24 + 3
        for a in range(3):
            for interpolate in (True, False):
                got = pk.bg_model_order(n, K, bm.alphas(K, a), interpolate)
                want = bm.model(n, K, bm.alphas(K, a), interpolate)
                bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
                assert bad.size == 0, (kind, a, interpolate, int(bad[0]), float(got[bad[0]]), float(want[bad[0]]))
                n_cases += 1
    assert n_cases == 24


def test_model_without_a_count_anywhere_and_with_a_single_base():
    for K in (0, 3, 5):
        zero = np.zeros(bm.size(K), np.uint64)
        got = pk.bg_model_order(zero, K, (1.0,) * (K + 1), True)
        assert got.tobytes() == bm.model(zero, K, (1.0,) * (K + 1)).tobytes() and np.allclose(got, 0.25)
        one = bm.bg_count([cm.encode("G")], K)
        assert int(one.sum()) == 1
        assert pk.bg_model_order(one, K, (1.0,) * (K + 1), True).tobytes() == bm.model(one, K, (1.0,) * (K + 1)).tobytes()


@pytest.mark.parametrize("K", [0, 1, 2])
def test_model_at_low_orders_is_the_oracles_v(K):
    """on the 84 counters of tests/table_edges_model.py whose values fit an int, every alpha"""
    for kind in tm.COUNTER_KINDS[:4]:
        n84 = np.asarray(tm._counter_set(kind), np.int64)
        for alpha in tm.ALPHAS:
            want = po.bg_V(n84, K, alpha, wide=True)
            got = pk.bg_model_order(n84.astype(np.uint64), K, alpha[:K + 1], True)
            assert got.tobytes() == want[:bm.size(K)].tobytes(), (kind, alpha)
            assert bm.model(n84.astype(np.uint64), K, alpha[:K + 1]).tobytes() == got.tobytes()


def test_model_argument_errors():
    n = np.zeros(bm.size(5), np.uint64)
    V = np.zeros(bm.size(5), np.float32)
    a = np.ones(6, np.float32)
    for K in (-1, 6):
        assert pk.lib().pengk_bg_model_order(n.ctypes.data, K, a.ctypes.data, 1, V.ctypes.data) == pk.ERR_ARG
    assert pk.lib().pengk_bg_model_order(None, 3, a.ctypes.data, 1, V.ctypes.data) == pk.ERR_ARG
    assert pk.lib().pengk_bg_model_order(n.ctypes.data, 3, None, 1, V.ctypes.data) == pk.ERR_ARG
    assert pk.lib().pengk_bg_model_order(n.ctypes.data, 3, a.ctypes.data, 1, None) == pk.ERR_ARG
    assert not V.any()


# ---- the counters -----------------------------------------------------------------------------------------------------------
def random_seqs(seed, lengths, invalid=0.0):
    rng = np.random.default_rng(seed)
    out = []
    for L in lengths:
        c = rng.integers(1, 5, L).astype(np.uint8)
        if invalid:
            c[rng.random(L) < invalid] = 0
        out.append(c)
    return out


def test_counters_at_low_orders_are_the_oracles_on_inputs_without_invalid_bases():
    seqs = random_seqs(1, [0, 1, 2, 3, 5, 6, 7, 31, 32, 33, 64, 65, 200] * 30)
    want = po.bg_counts(*bm._flatten(seqs), 2)
    for K in range(6):
        n = bm.bg_count(seqs, K)
        assert np.array_equal(n[:min(84, bm.size(K))].astype(np.int64), want[:min(84, bm.size(K))])
        for k in range(K + 1):  # every order holds the positions with k bases behind them
            assert int(n[bm.at(k):bm.at(k + 1)].sum()) == sum(max(len(c) - k, 0) for c in seqs)
        for k in range(K):      # and sums to the one below, up to the words that begin a sequence
            assert (n[bm.at(k + 1):bm.at(k + 2)].reshape(4, -1).sum(axis=0) <= n[bm.at(k):bm.at(k + 1)]).all()


def test_counters_by_hand():
    # ACGTANTTACGT: the base behind the N starts over at order 0
    c = np.array(cm.encode("ACGTA").tolist() + [0] + cm.encode("TTACGT").tolist(), np.uint8)
    n = bm.bg_count([c], 5)
    assert n[:4].tolist() == [3, 2, 2, 4]
    assert [int(n[bm.at(k):bm.at(k + 1)].sum()) for k in range(6)] == [11, 9, 7, 5, 3, 1]
    word = lambda s: sum((int(b) - 1) * 4 ** (len(s) - 1 - i) for i, b in enumerate(cm.encode(s)))  # noqa: E731
    assert n[bm.at(5) + word("TTACGT")] == 1 and n[bm.at(4) + word("ACGTA")] == 1 and n[bm.at(4) + word("TTACG")] == 1
    assert n[bm.at(3) + word("ACGT")] == 2
    m = bm.bg_count([c], 5, all_valid=True)  # the N is a valid A
    assert [int(m[bm.at(k):bm.at(k + 1)].sum()) for k in range(6)] == [12, 11, 10, 9, 8, 7] and m[bm.at(5) + word("TAATTA")] == 1


# ---- the sweep --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("both", [False, True], ids=["plus", "both"])
def test_order_two_tables_give_the_plain_sweeps_bits(both):
    for W in (2, 4, 6):
        for kind in "abc":
            V = tm.sweep_V(kind)
            for K in range(min(2, W - 1) + 1):
                assert bm.order_prob(W, K, V[:bm.size(K)], both).tobytes() == po.bgprob(W, K, V, both).tobytes(), (W, kind, K)


@pytest.mark.parametrize("W", [2, 4, 8])
def test_constructed_cases_hold_their_classes(W):
    specs = bm.small_cases(W, True)
    assert {(sp[3], sp[4]) for sp in specs} == set(tm.legal_orders(W)) and {sp[0] for sp in specs} == set(bm.SWEEP_KS)
    assert {sp[1] for sp in specs} == set(bm.V_KINDS)
    for K in bm.SWEEP_KS:
        assert {sp[6] for sp in specs if sp[0] == K} == {False, True} or W == 2
    for k, mk in tm.legal_orders(W):
        assert {sp[6] for sp in specs if (sp[3], sp[4]) == (k, mk)} == {False, True}
    seen = set()
    for sp in specs:
        c = bm.case(W, True, sp)
        assert len(c["VK"]) == bm.size(c["K"]) and len(c["bgp"]) == c["max_k"] + 1
        for name, mask in tm.count_classes(c).items():
            if mask.any():
                seen.add(name)
    assert {"n == 0", "0 < n <= 5", "n == 2^32 - 1"} <= seen


# ---- the scenario -----------------------------------------------------------------------------------------------------------
W_SCENARIO = 8


@pytest.fixture(scope="module")
def nothing_planted():
    out = {}
    for seed in (1, 2, 3):
        seqs = bm.chain(seed)
        out[seed] = {K: bm.seeds(seqs, W_SCENARIO, K)[0] for K in (2, 3, 4, 5)}
    return out


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_chains_own_words_are_seeds_under_order_2_and_none_is_under_order_4(nothing_planted, seed):
    s = nothing_planted[seed]
    print("seed %d, nothing planted: seeds under order 2 / 3 / 4 / 5: %d / %d / %d / %d" % (
        seed, len(s[2]), len(s[3]), len(s[4]), len(s[5])))
    assert len(s[2]) >= 100
    assert len(s[4]) == 0


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_a_planted_motif_leaves_seeds_of_its_own_under_order_4(seed):
    seqs = bm.chain(seed, planted=True)
    row = {K: bm.seeds(seqs, W_SCENARIO, K) for K in (2, 3, 4, 5)}
    print("seed %d, %s in 5 %%: seeds (of the motif) under order 2 / 3 / 4 / 5: %s; largest z with the motif %s" % (
        seed, bm.MOTIF, " / ".join("%d (%d)" % (len(w), sum(bm.shares_6mer(x) for x in w)) for w, _ in row.values()),
        " / ".join("%.0f" % z for _, z in row.values())))
    words = row[4][0]
    assert len(words) >= 1
    assert all(bm.shares_6mer(w) for w in words)


MARE = "TGCTGACTCAGCA"


def test_mafk_row_is_recorded(record_property):
    """tests/golden/MafK.fasta, W = 10, both strands: the seeds under order 2 and K = 3, 4, 5, and how many of the first 50
    by z share a 6-mer with the MARE.  Recorded, no bar: a small real input, where the order-2 null is not the problem."""
    codes, offs = po.read_fasta(os.path.join(GOLD, "MafK.fasta"))
    seqs = [codes[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]
    counts, ltot = po.count(codes, offs, 10, True)
    V = po.bg_V(po.bg_counts(codes, offs, 2), 2)
    row = []
    for K in (2, 3, 4, 5):
        _, VK = bm.cli_model(seqs, K)
        _, _, _, z = bm.sweep(10, True, 2, 2, V, K, VK, counts, ltot)
        ids = po.select(10, z, counts, 10.0, 3, False, True)
        words = [po.kmer_str(int(x), 10) for x in sorted(ids, key=lambda x: (-float(z[x]), int(x)))[:50]]
        row.append((K, len(ids), sum(cm.shares_6mer(w, MARE) for w in words)))
    print("MafK.fasta, W = 10: (order, seeds, of the first 50 with a 6-mer of the MARE): %s" % row)
    record_property("mafk_row", str(row))
    assert row[0][1] > 0


# ---- the report -------------------------------------------------------------------------------------------------------------
def test_report_and_stdout_line_by_hand():
    c = np.array(cm.encode("ACGTA").tolist() + [0] + cm.encode("TTACGT").tolist(), np.uint8)
    n = bm.bg_count([c], 3)
    lines = bm.report(n, 3).splitlines()
    assert lines[0] == bm.REPORT_HEADER.rstrip("\n") and len(lines) == 5
    assert lines[1] == "0\t1\t1\t11\t11"
    assert lines[2] == "1\t4\t4\t2\t2"            # A 3, C 2, G 2, T 4: the lower median of four
    assert lines[3] == "2\t16\t5\t0\t0"           # AC CG GT TA (twice each) and TT
    assert lines[4].split("\t")[:3] == ["3", "64", "5"]
    assert bm.stdout_line(n, 3) == "high-order background: order 3, alpha 1, 11 model bases, 5 of 64 contexts seen"
    assert bm.stdout_line(n, 3, 2.5).startswith("high-order background: order 3, alpha 2.5, ")


# ---- the CLI's flags ---------------------------------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "peng-motif_amd", "host", "peng_motif")
GOLD = os.path.join(ROOT, "tests", "golden")


def clean_env():
    return {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PENGK_COMM_TRANSPORT")}


def test_help_lists_the_high_order_flags():
    r = subprocess.run([CLI, "-h"], stdout=subprocess.PIPE, env=clean_env(), timeout=60)
    assert r.returncode == 0
    for flag in (b"--high-order-background K", b"--high-order-alpha FLOAT", b"--high-order-report FILE"):
        assert flag in r.stdout, flag


@pytest.mark.parametrize("extra,message", [
    (["--high-order-background", "2"], b"--high-order-background must be an integer in [3, 5]"),
    (["--high-order-background", "6"], b"--high-order-background must be an integer in [3, 5]"),
    (["--high-order-background", "4x"], b"--high-order-background must be"),
    (["--high-order-background", "4", "-w", "4"], b"--high-order-background must be below the pattern length"),
    (["-w", "4", "--high-order-background", "5"], b"--high-order-background must be below the pattern length"),
    (["--high-order-background", "3", "--high-order-alpha", "0"], b"--high-order-alpha must be a finite number above 0"),
    (["--high-order-background", "3", "--high-order-alpha", "-1"], b"--high-order-alpha must be"),
    (["--high-order-background", "3", "--high-order-alpha", "inf"], b"--high-order-alpha must be"),
    (["--high-order-background", "3", "--high-order-alpha", "nan"], b"--high-order-alpha must be"),
    (["--high-order-background", "3", "--high-order-alpha", "1e-60"], b"--high-order-alpha must be"),
    (["--high-order-alpha", "2"], b"--high-order-alpha requires --high-order-background"),
    (["--high-order-report", "x.tsv"], b"--high-order-report requires --high-order-background"),
    (["--high-order-background", "3", "--stratified-background"], b"--high-order-background cannot be combined with --stratified-background"),
    (["--high-order-background", "3", "--bg-model-order", "1"], b"--high-order-background needs the default --bg-model-order 2"),
], ids=["order_2", "order_6", "order_not_a_number", "order_at_w", "order_above_w", "alpha_0", "alpha_negative", "alpha_inf", "alpha_nan",
        "alpha_below_float", "alpha_alone", "report_alone", "with_stratified", "with_bg_model_order_1"])
def test_flag_errors_exit_with_4_before_the_input_is_read(tmp_path, extra, message):
    r = subprocess.run([CLI, os.path.join(GOLD, "MafK.fasta"), "-o", str(tmp_path / "o.meme")] + extra, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, env=clean_env(), timeout=60)
    assert r.returncode == 4 and message in r.stderr and b"ERROR" in r.stderr, (r.returncode, r.stderr.decode()[-500:])
    assert b"--high-order-background K" in r.stdout  # (the help)
    assert not (tmp_path / "o.meme").exists()


def test_the_chain_is_the_one_the_file_states():
    a, b = bm.chain(7, 50), bm.chain(7, 50, planted=True)
    assert len(a) == 50 and all(len(c) == bm.SEQ_LEN and c.min() >= 1 and c.max() <= 4 for c in a)
    differ = [i for i in range(50) if not np.array_equal(a[i], b[i])]
    assert all("".join("ACGT"[v - 1] for v in b[i]).count(bm.MOTIF) >= 1 for i in differ)
    rng = np.random.default_rng(7)
    rng.dirichlet([8.0] * 4, 256)
    assert np.array_equal(np.stack(a)[:, :4], rng.integers(0, 4, (50, 4)) + 1)
