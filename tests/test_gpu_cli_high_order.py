"""peng_motif --high-order-background: the scenario of tests/bg_order_model.py -- 20 000 x 100 bp of a random order-4 chain,
TGACTCAGCA in 5 %, seed 1 -- as a FASTA file through the CLI at W = 8, K = 4.  With the flag the tables the run leaves
(PENGK_DUMP_TABLES) are the model's bits, the report is the model's file and every motif written is the planted one; without
it the chain's own words are reported as motifs, and the output is what the commit before the flag wrote
(tests/golden/high_order_parent.json).  Two ranks against one process; the counts beside --mask-low-complexity and
--holdout; the tables beside --discriminative."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import bg_order_model as bm
import cli_combined_model as cc
import control_stats_model as cm
import motif_dust_model as md
from oracle import oracle as po
from test_gpu_cli_stratified import motifs, write_fasta
from test_gpu_multirank import CLI, clean_env, run_plain, run_ranks

pytestmark = pytest.mark.gpu

W, K = 8, 4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "high_order_parent.json")


def of_the_motif(m):
    return bm.shares_6mer(m)


@pytest.fixture(scope="module")
def scenario(tmp_path_factory):
    d = tmp_path_factory.mktemp("high_order")
    seqs = bm.chain(1, planted=True)
    fa = str(d / "input.fa")
    write_fasta(fa, seqs)
    return dict(dir=d, fa=fa, seqs=seqs, args=[fa, "-w", str(W)])


@pytest.fixture(scope="module")
def runs(scenario, tmp_path_factory):
    """the run without the flag, and the run with it (which also leaves its tables and the report)"""
    d = tmp_path_factory.mktemp("runs")
    dump = d / "tables"
    dump.mkdir()
    plain = run_plain(scenario["args"], d, tag="order2")
    flagged = run_plain(scenario["args"] + ["--high-order-background", str(K), "--high-order-report", str(d / "order.tsv")], d,
                        tag="order4", extra_env={"PENGK_DUMP_TABLES": str(dump)})
    return plain, flagged, dump, d / "order.tsv"


def test_with_the_flag_every_motif_is_the_planted_one_and_without_it_the_chains_words_are_reported(runs):
    (rc0, so0, se0, _, js0), (rc1, so1, se1, _, js1), _, _ = runs
    assert rc0 == 0, se0.decode()[-2000:]
    assert rc1 == 0, se1.decode()[-2000:]
    order2, order4 = motifs(js0), motifs(js1)
    print("without the flag:", order2, "with it:", order4)
    assert order4 and all(of_the_motif(m) for m in order4), order4
    assert any(not of_the_motif(m) for m in order2), order2
    assert b"high-order background: order 4" in so1 and b"high-order background" not in so0


def test_the_dumped_tables_and_the_report_are_the_models(scenario, runs):
    _, (rc, so, se, _, _), dump, report = runs
    assert rc == 0, se.decode()[-2000:]
    seqs = scenario["seqs"]
    n, _ = bm.cli_model(seqs, K)
    counts, e, z, VK = bm.cli_sweep(seqs, seqs, W, K)
    assert report.read_text() == bm.report(n, K)
    assert bm.stdout_line(n, K).encode() + b"\n" in so
    assert np.fromfile(str(dump / "order_V.f32"), np.float32).tobytes() == VK.tobytes()
    assert np.array_equal(np.fromfile(str(dump / "counts.u32"), np.uint32).astype(np.uint64), counts)
    assert np.fromfile(str(dump / "expected.f32"), np.float32).tobytes() == e.tobytes()
    assert np.fromfile(str(dump / "z.f32"), np.float32).tobytes() == z.tobytes()
    # V.f32 stays the one model, which the reports' log-odds read
    codes, offs = bm._flatten(seqs)
    assert np.fromfile(str(dump / "V.f32"), np.float32).tobytes() == po.bg_V(po.bg_counts(codes, offs, 2), 2).tobytes()
    meta = dict(l.split(None, 1) for l in (dump / "meta.txt").read_text().splitlines())
    assert meta["order"].split() == [str(K)]
    # and the model's seeds are the ones the run printed: every one of the motif
    seeds = [po.kmer_str(int(x), W) for x in po.select(W, z, counts, 10.0, 3, False, True)]
    assert seeds and all(of_the_motif(s) for s in seeds)
    for s in seeds:
        assert s.encode() in so, s


def test_alpha_reaches_the_orders_above_two_only(scenario, tmp_path):
    dump = tmp_path / "tables"
    dump.mkdir()
    rc, so, se, _, _ = run_plain(scenario["args"] + ["--high-order-background", "5", "--high-order-alpha", "2.5"], tmp_path,
                                 extra_env={"PENGK_DUMP_TABLES": str(dump)})
    assert rc == 0, se.decode()[-2000:]
    seqs = scenario["seqs"]
    n, VK = bm.cli_model(seqs, 5, 2.5)
    assert bm.stdout_line(n, 5, 2.5).encode() + b"\n" in so
    assert np.fromfile(str(dump / "order_V.f32"), np.float32).tobytes() == VK.tobytes()
    assert VK[:84].tobytes() == bm.cli_model(seqs, 2)[1].tobytes() and VK[84:].tobytes() != bm.cli_model(seqs, 5)[1][84:].tobytes()
    _, e, z, _ = bm.cli_sweep(seqs, seqs, W, 5, alpha_high=2.5)
    assert np.fromfile(str(dump / "z.f32"), np.float32).tobytes() == z.tobytes()
    assert np.fromfile(str(dump / "expected.f32"), np.float32).tobytes() == e.tobytes()


def test_without_the_flag_the_output_is_the_parent_commits(scenario, tmp_path):
    """the files of this input from the commit before the flag existed, recorded once: stdout, the MEME and the JSON file byte
    for byte (by their SHA-256; the run names its files relative to its directory), the motifs in the clear"""
    dump = tmp_path / "tables"
    dump.mkdir()
    r = subprocess.run([CLI, os.path.relpath(scenario["fa"], str(tmp_path)), "-w", str(W), "-o", "out.meme", "-j", "out.json"],
                       cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=clean_env(PENGK_DUMP_TABLES="tables"), timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    meme, js = (tmp_path / "out.meme").read_bytes(), (tmp_path / "out.json").read_bytes()
    got = dict(motifs=motifs(js), stdout_sha256=hashlib.sha256(r.stdout).hexdigest(), meme_sha256=hashlib.sha256(meme).hexdigest(),
               json_sha256=hashlib.sha256(js).hexdigest(), z_sha256=hashlib.sha256((dump / "z.f32").read_bytes()).hexdigest(),
               expected_sha256=hashlib.sha256((dump / "expected.f32").read_bytes()).hexdigest())
    assert not (dump / "order_V.f32").exists() and "order" not in (dump / "meta.txt").read_text()
    with open(GOLDEN) as f:
        want = json.load(f)
    assert got == want


def test_two_ranks_write_what_one_process_writes(scenario, runs, tmp_path):
    _, (rc, so, se, meme, js), dump, report = runs
    assert rc == 0, se.decode()[-2000:]
    many = tmp_path / "tables"
    many.mkdir()
    res = run_ranks(scenario["args"] + ["--high-order-background", str(K), "--high-order-report", str(tmp_path / "order.tsv")], 2,
                    tmp_path, extra_env={"PENGK_DUMP_TABLES": str(many)})
    for rank, (rrc, rso, rse, rmeme, rjs) in enumerate(res):
        assert rrc == 0, (rank, rse.decode()[-2000:])
    assert (res[0][1], res[0][3], res[0][4]) == (so, meme, js) and res[1][1] == b""
    assert (tmp_path / "order.tsv").read_bytes() == report.read_bytes()
    for name in ("order_V.f32", "counts.u32", "z.f32", "expected.f32", "meta.txt"):
        assert (many / name).read_bytes() == (dump / name).read_bytes(), name


# ---- beside the flags that change what round 1 counts ---------------------------------------------------------------------------
def small_chain(seed, n=2000):
    """2000 x 100 bp of the chain, a tract of one letter in every seventh: something for the mask to take"""
    seqs = bm.chain(seed, n)
    rng = np.random.default_rng(seed + 100)
    for i in range(0, n, 7):
        at = int(rng.integers(0, 70))
        seqs[i][at:at + 25] = 1 + i % 4
    return seqs


def test_beside_mask_and_holdout_the_counts_are_the_masked_training_shares_and_the_model_the_whole_inputs(tmp_path):
    seqs = small_chain(4)
    fa = str(tmp_path / "small.fa")
    write_fasta(fa, seqs)
    dump = tmp_path / "tables"
    dump.mkdir()
    rc, so, se, _, _ = run_plain([fa, "-w", str(W), "--high-order-background", "3", "--high-order-report", str(tmp_path / "order.tsv"),
                                  "--mask-low-complexity", "--holdout", str(tmp_path / "holdout.tsv")], tmp_path,
                                 extra_env={"PENGK_DUMP_TABLES": str(dump)})
    assert rc == 0, se.decode()[-2000:]
    masked, bits, _ = md.mask_codes(seqs, cc.T)
    i0, _ = cc.split(len(seqs))
    assert bits > 0 and 0 < len(i0) < len(seqs)
    counted = [masked[i] for i in i0]
    n, VK = bm.cli_model(seqs, 3)
    assert not np.array_equal(n, bm.bg_count(counted, 3))
    assert np.fromfile(str(dump / "order_V.f32"), np.float32).tobytes() == VK.tobytes()   # (the model: the whole input, unmasked)
    assert (tmp_path / "order.tsv").read_text() == bm.report(n, 3)
    counts, e, z, _ = bm.cli_sweep(counted, seqs, W, 3)
    assert np.array_equal(np.fromfile(str(dump / "counts.u32"), np.uint32).astype(np.uint64), counts)
    assert np.fromfile(str(dump / "z.f32"), np.float32).tobytes() == z.tobytes()
    assert np.fromfile(str(dump / "expected.f32"), np.float32).tobytes() == e.tobytes()


def test_beside_discriminative_the_tables_are_the_models_with_the_control_on_top(tmp_path):
    """the control set is the model's source set, and its share is applied on top of the order-K null"""
    inp, ctl, offs = cm.planted(1)
    split = lambda c: [c[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]  # noqa: E731
    fa, bg = str(tmp_path / "input.fa"), str(tmp_path / "control.fa")
    write_fasta(fa, split(inp))
    write_fasta(bg, split(ctl))
    dump = tmp_path / "tables"
    dump.mkdir()
    rc, so, se, _, _ = run_plain([fa, "-w", str(W), "--background-sequences", bg, "--discriminative", "--high-order-background", "3"],
                                 tmp_path, extra_env={"PENGK_DUMP_TABLES": str(dump)})
    assert rc == 0, se.decode()[-2000:]
    ctrl, lc = po.count(ctl, offs, W, True)
    counts, e, z, VK = bm.cli_sweep(split(inp), split(ctl), W, 3, ctrl=ctrl, Lc=lc, a=1.0)
    plain = bm.cli_sweep(split(inp), split(ctl), W, 3)
    assert plain[2].tobytes() != z.tobytes()  # (the control's share moves something)
    assert np.fromfile(str(dump / "order_V.f32"), np.float32).tobytes() == VK.tobytes()
    assert np.fromfile(str(dump / "expected.f32"), np.float32).tobytes() == e.tobytes()
    assert np.fromfile(str(dump / "z.f32"), np.float32).tobytes() == z.tobytes()
