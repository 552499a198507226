"""peng_motif --discriminative: the planted scenario of tests/control_stats_model.py as two FASTA files through the CLI
at W = 8.  Without the flag the contaminant the control shares is reported as a motif; with it no reported motif has
anything of it and the real motif comes first.  The tables the run leaves (PENGK_DUMP_TABLES) against the model; the
flag errors; two ranks against one process."""
import json

import numpy as np
import pytest

import control_stats_model as cm
from oracle import oracle as po
from test_gpu_multirank import run_plain, run_ranks

pytestmark = pytest.mark.gpu

W = 8


def write_fasta(path, codes, offs):
    letters = np.frombuffer(b"NACGT", np.uint8)[codes]
    with open(path, "wb") as f:
        for i in range(len(offs) - 1):
            f.write(b">s%d\n" % i + letters[offs[i]:offs[i + 1]].tobytes() + b"\n")


@pytest.fixture(scope="module")
def scenario(tmp_path_factory):
    d = tmp_path_factory.mktemp("discriminative")
    inp, ctl, offs = cm.planted(1)
    fa, bg = str(d / "input.fa"), str(d / "control.fa")
    write_fasta(fa, inp, offs)
    write_fasta(bg, ctl, offs)
    return dict(fa=fa, bg=bg, inp=inp, ctl=ctl, offs=offs, args=[fa, "-w", str(W), "--background-sequences", bg])


@pytest.fixture(scope="module")
def runs(scenario, tmp_path_factory):
    """the run without the flag, and the run with it (which also leaves its tables)"""
    d = tmp_path_factory.mktemp("runs")
    dump = d / "tables"
    dump.mkdir()
    plain = run_plain(scenario["args"], d, tag="markov")
    flagged = run_plain(scenario["args"] + ["--discriminative"], d, tag="control", extra_env={"PENGK_DUMP_TABLES": str(dump)})
    return plain, flagged, dump


def motifs(js):
    return [p["iupac_motif"] for p in json.loads(js)["patterns"]]


def test_the_contaminant_is_reported_without_the_flag_and_not_with_it(runs):
    (rc0, so0, se0, _, js0), (rc1, so1, se1, _, js1), _ = runs
    assert rc0 == 0, se0.decode()[-2000:]
    assert rc1 == 0, se1.decode()[-2000:]
    markov, control = motifs(js0), motifs(js1)
    print("without the flag:", markov, "with it:", control)
    assert any(cm.shares_6mer(m, cm.U_MOTIF) for m in markov), markov
    assert control and not any(cm.shares_6mer(m, cm.U_MOTIF) for m in control), control
    # the top motif is the planted one.  Under both strands a motif and its reverse complement are one motif, and which
    # strand a run names it on follows from the order of exact z ties (include/pengk.h, pengk_seed_candidates): this run
    # names it ACTGCTGAGTCA, the run without the flag TGACTCAGCAGT.  So the core is looked for on either strand, as the
    # contaminant is -- and the motif must be one the run without the flag reports too, up to the strand.
    top = control[0]
    assert "TGACTCA" in top or "TGACTCA" in cm.revcomp_str(top), control
    assert top in markov or cm.revcomp_str(top) in markov, (control, markov)
    # the line on stdout that names the mode
    assert b"discriminative mode" in so1 and b"discriminative mode" not in so0


def test_the_dumped_tables_equal_the_model(scenario, runs):
    _, (rc, so, se, _, _), dump = runs
    assert rc == 0, se.decode()[-2000:]
    NP = 4 ** W
    meta = dict(l.split() for l in (dump / "meta.txt").read_text().splitlines())
    counts, ltot = po.count(scenario["inp"], scenario["offs"], W, True)
    ctrl, lc = po.count(scenario["ctl"], scenario["offs"], W, True)
    assert int(meta["ltot"]) == ltot and int(meta["ctrl_ltot"]) == lc
    assert ("(%d control windows" % lc).encode() in so
    got_ctrl = np.fromfile(str(dump / "ctrl_counts.u32"), np.uint32)
    assert got_ctrl.size == NP and np.array_equal(got_ctrl.astype(np.uint64), ctrl)
    assert np.array_equal(np.fromfile(str(dump / "counts.u32"), np.uint32).astype(np.uint64), counts)
    V = np.fromfile(str(dump / "V.f32"), np.float32)
    assert V.tobytes() == po.bg_V(po.bg_counts(scenario["ctl"], scenario["offs"], 2), 2).tobytes()  # trained on the control, as without the flag
    p = [po.bgprob(W, o, V, True) for o in range(3)]
    _, e, _, z = cm.sweep(W, counts, ltot, p, 2, ctrl, lc, 1.0)
    assert np.fromfile(str(dump / "expected.f32"), np.float32).tobytes() == e.tobytes()
    assert np.fromfile(str(dump / "z.f32"), np.float32).tobytes() == z.tobytes()
    # and the model's seeds are the ones the run printed: none of the contaminant
    seeds = [po.kmer_str(int(x), W) for x in po.select(W, z, counts, 10.0, 3, False, True)]
    assert seeds and not any(cm.shares_6mer(s, cm.U_MOTIF) for s in seeds)
    for s in seeds:
        assert s.encode() in so, s


def test_the_pseudocount_reaches_the_sweep(scenario, tmp_path):
    dump = tmp_path / "tables"
    dump.mkdir()
    rc, so, se, _, _ = run_plain(scenario["args"] + ["--discriminative", "--discriminative-pseudocount", "0.5"], tmp_path,
                                 extra_env={"PENGK_DUMP_TABLES": str(dump)})
    assert rc == 0, se.decode()[-2000:]
    counts, ltot = po.count(scenario["inp"], scenario["offs"], W, True)
    ctrl, lc = po.count(scenario["ctl"], scenario["offs"], W, True)
    V = np.fromfile(str(dump / "V.f32"), np.float32)
    p = [po.bgprob(W, o, V, True) for o in range(3)]
    _, e, _, z = cm.sweep(W, counts, ltot, p, 2, ctrl, lc, 0.5)
    assert np.fromfile(str(dump / "expected.f32"), np.float32).tobytes() == e.tobytes()
    assert np.fromfile(str(dump / "z.f32"), np.float32).tobytes() == z.tobytes()


def test_without_the_flag_no_control_table_is_written(scenario, tmp_path):
    dump = tmp_path / "tables"
    dump.mkdir()
    rc, so, se, _, _ = run_plain(scenario["args"], tmp_path, extra_env={"PENGK_DUMP_TABLES": str(dump)})
    assert rc == 0, se.decode()[-2000:]
    assert not (dump / "ctrl_counts.u32").exists() and "ctrl_ltot" not in (dump / "meta.txt").read_text()


@pytest.mark.parametrize("extra,message", [
    (["--discriminative"], b"--discriminative requires --background-sequences"),
    (["--background-sequences", "BG", "--discriminative", "--discriminative-pseudocount", "-0.5"], b"--discriminative-pseudocount must be"),
    (["--background-sequences", "BG", "--discriminative", "--discriminative-pseudocount", "nan"], b"--discriminative-pseudocount must be"),
    (["--background-sequences", "BG", "--discriminative", "--discriminative-pseudocount", "inf"], b"--discriminative-pseudocount must be"),
    (["--background-sequences", "BG", "--discriminative", "--discriminative-pseudocount", "1x"], b"--discriminative-pseudocount must be"),
], ids=["no_control", "negative", "nan", "inf", "not_a_number"])
def test_flag_errors_exit_with_4(scenario, tmp_path, extra, message):
    args = [scenario["fa"], "-w", str(W)] + [scenario["bg"] if a == "BG" else a for a in extra]
    rc, so, se, meme, js = run_plain(args, tmp_path)
    assert rc == 4 and message in se and b"ERROR" in se, (rc, se.decode()[-500:])
    assert meme is None and js is None


def test_two_ranks_write_what_one_process_writes(scenario, runs, tmp_path):
    _, (rc, so, se, meme, js), dump = runs
    assert rc == 0, se.decode()[-2000:]
    many = tmp_path / "tables"
    many.mkdir()
    res = run_ranks(scenario["args"] + ["--discriminative"], 2, tmp_path, extra_env={"PENGK_DUMP_TABLES": str(many)})
    for rank, (rrc, rso, rse, rmeme, rjs) in enumerate(res):
        assert rrc == 0, (rank, rse.decode()[-2000:])
    assert (res[0][1], res[0][3], res[0][4]) == (so, meme, js) and res[1][1] == b""
    for name in ("ctrl_counts.u32", "counts.u32", "z.f32", "expected.f32", "meta.txt"):
        assert (many / name).read_bytes() == (dump / name).read_bytes(), name
