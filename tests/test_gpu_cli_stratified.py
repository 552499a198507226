"""peng_motif --stratified-background: the scenario of tests/strata_stats_model.py -- 20 000 x 100 bp, half at 30 % and half
at 70 % GC, TGACTCAGCA in 5 % -- as a FASTA file through the CLI at W = 8.  With the flag the tables the run leaves
(PENGK_DUMP_TABLES) are the model's bits, the report is the model's file and every motif written is the planted one;
without it composition is reported as a motif, and the output is what the commit before the flag wrote
(tests/golden/stratified_parent.json).  Two ranks against one process; the weights beside --mask-low-complexity and
--holdout; the tables beside --discriminative; the flag errors."""
import hashlib
import json
import os

import numpy as np
import pytest

import cli_combined_model as cc
import control_stats_model as cm
import motif_dust_model as md
import strata_stats_model as sm
from oracle import oracle as po
from test_gpu_multirank import run_plain, run_ranks

pytestmark = pytest.mark.gpu

W = 8
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stratified_parent.json")


def write_fasta(path, seqs):
    letters = np.frombuffer(b"NACGT", np.uint8)
    with open(path, "wb") as f:
        for i, c in enumerate(seqs):
            f.write(b">s%d\n" % i + letters[c].tobytes() + b"\n")


def motifs(js):
    return [p["iupac_motif"] for p in json.loads(js)["patterns"]]


def of_the_motif(m):
    return cm.shares_6mer(m, sm.MOTIF)


@pytest.fixture(scope="module")
def scenario(tmp_path_factory):
    d = tmp_path_factory.mktemp("stratified")
    seqs = sm.mixed(1, planted=True)
    fa = str(d / "input.fa")
    write_fasta(fa, seqs)
    return dict(fa=fa, seqs=seqs, args=[fa, "-w", str(W)])


@pytest.fixture(scope="module")
def runs(scenario, tmp_path_factory):
    """the run without the flag, and the run with it (which also leaves its tables and the report)"""
    d = tmp_path_factory.mktemp("runs")
    dump = d / "tables"
    dump.mkdir()
    plain = run_plain(scenario["args"], d, tag="markov")
    flagged = run_plain(scenario["args"] + ["--stratified-background", "--stratified-report", str(d / "strata.tsv")], d, tag="strata",
                        extra_env={"PENGK_DUMP_TABLES": str(dump)})
    return plain, flagged, dump, d / "strata.tsv"


def test_with_the_flag_every_motif_is_the_planted_one_and_without_it_composition_is_reported(runs):
    (rc0, so0, se0, _, js0), (rc1, so1, se1, _, js1), _, _ = runs
    assert rc0 == 0, se0.decode()[-2000:]
    assert rc1 == 0, se1.decode()[-2000:]
    markov, strata = motifs(js0), motifs(js1)
    print("without the flag:", markov, "with it:", strata)
    assert strata and all(of_the_motif(m) for m in strata), strata
    assert any(not of_the_motif(m) for m in markov), markov
    assert b"stratified background: 10 GC bins" in so1 and b"stratified background" not in so0


def test_the_dumped_tables_and_the_report_are_the_models(scenario, runs):
    _, (rc, so, se, _, _), dump, report = runs
    assert rc == 0, se.decode()[-2000:]
    seqs = scenario["seqs"]
    st = sm.stratified(seqs, seqs, W)
    assert report.read_text() == sm.report(st)
    assert np.fromfile(str(dump / "strata_windows.u64"), np.uint64).tolist() == st["windows"].tolist()
    assert np.fromfile(str(dump / "strata_V.f32"), np.float32).tobytes() == st["V"].tobytes()
    assert st["own"].sum() >= 2 and not st["own"].all()  # (both kinds of stratum are in the file)
    counts, z, e = sm.stratified_z(seqs, seqs, W)
    assert np.array_equal(np.fromfile(str(dump / "counts.u32"), np.uint32).astype(np.uint64), counts)
    assert np.fromfile(str(dump / "expected.f32"), np.float32).tobytes() == e.tobytes()
    assert np.fromfile(str(dump / "z.f32"), np.float32).tobytes() == z.tobytes()
    # V.f32 stays the one model, which the reports' log-odds read
    codes, offs = sm._flatten(seqs)
    assert np.fromfile(str(dump / "V.f32"), np.float32).tobytes() == po.bg_V(po.bg_counts(codes, offs, 2), 2).tobytes()
    meta = dict(l.split(None, 1) for l in (dump / "meta.txt").read_text().splitlines())
    assert meta["strata"].split() == ["10"] + [str(int(w)) for w in st["windows"]]
    # and the model's seeds are the ones the run printed: every one of the motif
    seeds = [po.kmer_str(int(x), W) for x in po.select(W, z, counts, 10.0, 3, False, True)]
    assert seeds and all(of_the_motif(s) for s in seeds)
    for s in seeds:
        assert s.encode() in so, s


def test_without_the_flag_the_output_is_the_parent_commits(scenario, runs, tmp_path):
    """the files of this input from the commit before the flag existed, recorded once: the MEME and the JSON file byte for
    byte (by their SHA-256), the motifs in the clear"""
    (rc, so, se, meme, js), _, _, _ = runs
    assert rc == 0, se.decode()[-2000:]
    dump = tmp_path / "tables"
    dump.mkdir()
    rc2, _, se2, meme2, js2 = run_plain(scenario["args"], tmp_path, extra_env={"PENGK_DUMP_TABLES": str(dump)})
    assert rc2 == 0 and (meme2, js2) == (meme, js)
    got = dict(motifs=motifs(js), meme_sha256=hashlib.sha256(meme).hexdigest(), json_sha256=hashlib.sha256(js).hexdigest(),
               z_sha256=hashlib.sha256((dump / "z.f32").read_bytes()).hexdigest(),
               expected_sha256=hashlib.sha256((dump / "expected.f32").read_bytes()).hexdigest())
    assert not (dump / "strata_V.f32").exists() and "strata" not in (dump / "meta.txt").read_text()
    with open(GOLDEN) as f:
        want = json.load(f)
    assert got == want


def test_two_ranks_write_what_one_process_writes(scenario, runs, tmp_path):
    _, (rc, so, se, meme, js), dump, report = runs
    assert rc == 0, se.decode()[-2000:]
    many = tmp_path / "tables"
    many.mkdir()
    res = run_ranks(scenario["args"] + ["--stratified-background", "--stratified-report", str(tmp_path / "strata.tsv")], 2, tmp_path,
                    extra_env={"PENGK_DUMP_TABLES": str(many)})
    for rank, (rrc, rso, rse, rmeme, rjs) in enumerate(res):
        assert rrc == 0, (rank, rse.decode()[-2000:])
    assert (res[0][1], res[0][3], res[0][4]) == (so, meme, js) and res[1][1] == b""
    assert (tmp_path / "strata.tsv").read_bytes() == report.read_bytes()
    for name in ("strata_V.f32", "strata_windows.u64", "counts.u32", "z.f32", "expected.f32", "meta.txt"):
        assert (many / name).read_bytes() == (dump / name).read_bytes(), name


# ---- beside the flags that change what round 1 counts ---------------------------------------------------------------------------
def small_mixed(seed, n=2000):
    """2000 x 100 bp of the same two compositions, a tract of one letter in every seventh: something for the mask to take"""
    seqs = sm.mixed(seed, n)
    rng = np.random.default_rng(seed + 100)
    for i in range(0, n, 7):
        at = int(rng.integers(0, 70))
        seqs[i][at:at + 25] = 1 + i % 4
    return seqs


def test_beside_mask_and_holdout_the_weights_are_those_of_the_masked_training_share(tmp_path):
    seqs = small_mixed(4)
    fa = str(tmp_path / "small.fa")
    write_fasta(fa, seqs)
    dump = tmp_path / "tables"
    dump.mkdir()
    rc, so, se, _, _ = run_plain([fa, "-w", str(W), "--stratified-background", "--stratified-report", str(tmp_path / "strata.tsv"),
                                  "--mask-low-complexity", "--holdout", str(tmp_path / "holdout.tsv")], tmp_path,
                                 extra_env={"PENGK_DUMP_TABLES": str(dump)})
    assert rc == 0, se.decode()[-2000:]
    masked, bits, _ = md.mask_codes(seqs, cc.T)
    i0, _ = cc.split(len(seqs))
    assert bits > 0 and 0 < len(i0) < len(seqs)
    st = sm.stratified([masked[i] for i in i0], seqs, W, strata_of=[seqs[i] for i in i0])
    plain = sm.stratified(seqs, seqs, W)
    assert st["windows"].tolist() != plain["windows"].tolist()
    assert np.fromfile(str(dump / "strata_windows.u64"), np.uint64).tolist() == st["windows"].tolist()
    assert np.fromfile(str(dump / "strata_V.f32"), np.float32).tobytes() == st["V"].tobytes()   # (the models: the whole input, unmasked)
    assert (tmp_path / "strata.tsv").read_text() == sm.report(st)
    counts, ltot = po.count(*sm._flatten([masked[i] for i in i0]), W, True)
    p = sm.markov_tables(W, st["V"], True, 2, st["windows"])
    _, e, _, z = sm.sweep(W, counts, ltot, p, st["windows"], 2)
    assert np.fromfile(str(dump / "z.f32"), np.float32).tobytes() == z.tobytes()
    assert np.fromfile(str(dump / "expected.f32"), np.float32).tobytes() == e.tobytes()


def test_beside_discriminative_the_tables_are_the_models(tmp_path):
    """the control set is the model's source set, and its share is applied on top of the mixed null"""
    inp, ctl, offs = cm.planted(1)
    split = lambda c: [c[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]  # noqa: E731
    fa, bg = str(tmp_path / "input.fa"), str(tmp_path / "control.fa")
    write_fasta(fa, split(inp))
    write_fasta(bg, split(ctl))
    dump = tmp_path / "tables"
    dump.mkdir()
    rc, so, se, _, _ = run_plain([fa, "-w", str(W), "--background-sequences", bg, "--discriminative", "--stratified-background",
                                  "--stratified-gc-bins", "4", "--stratified-min-bases", "20000"], tmp_path,
                                 extra_env={"PENGK_DUMP_TABLES": str(dump)})
    assert rc == 0, se.decode()[-2000:]
    st = sm.stratified(split(inp), split(ctl), W, G=4, min_bases=20000)
    assert st["own"].any() and not st["own"].all()
    assert np.fromfile(str(dump / "strata_windows.u64"), np.uint64).tolist() == st["windows"].tolist()
    assert np.fromfile(str(dump / "strata_V.f32"), np.float32).tobytes() == st["V"].tobytes()
    counts, ltot = po.count(inp, offs, W, True)
    ctrl, lc = po.count(ctl, offs, W, True)
    p = sm.markov_tables(W, st["V"], True, 2, st["windows"])
    _, e, _, z = sm.sweep(W, counts, ltot, p, st["windows"], 2, ctrl, lc, 1.0)
    assert np.fromfile(str(dump / "expected.f32"), np.float32).tobytes() == e.tobytes()
    assert np.fromfile(str(dump / "z.f32"), np.float32).tobytes() == z.tobytes()


@pytest.mark.parametrize("extra,message", [
    (["--stratified-background", "--stratified-gc-bins", "0"], b"--stratified-gc-bins must be an integer in [1, 16]"),
    (["--stratified-background", "--stratified-gc-bins", "17"], b"--stratified-gc-bins must be an integer in [1, 16]"),
    (["--stratified-background", "--stratified-gc-bins", "4x"], b"--stratified-gc-bins must be"),
    (["--stratified-background", "--stratified-min-bases", "-1"], b"--stratified-min-bases must be"),
    (["--stratified-gc-bins", "4"], b"--stratified-gc-bins requires --stratified-background"),
    (["--stratified-report", "x.tsv"], b"--stratified-report requires --stratified-background"),
], ids=["bins_0", "bins_17", "bins_not_a_number", "min_bases_negative", "bins_alone", "report_alone"])
def test_flag_errors_exit_with_4(scenario, tmp_path, extra, message):
    rc, so, se, meme, js = run_plain(scenario["args"] + extra, tmp_path)
    assert rc == 4 and message in se and b"ERROR" in se, (rc, se.decode()[-500:])
    assert meme is None and js is None
