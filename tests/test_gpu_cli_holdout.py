"""peng_motif --holdout: the planted scenario of tests/test_motif_holdout_cpu.py at seed 1 (TGACTCAGCA in 30 % of 2 000
uniform sequences of 100 bp, shuffled negatives, W = 8) as a FASTA file through the CLI.  The report against the numpy
model of tests/motif_holdout_model.py, line for line; the tables round 1 leaves (PENGK_DUMP_TABLES) against the oracle's
count of the training share; the MEME file against a run without the flag on the training sequences alone; the outputs
without the flag against the reference's goldens; two ranks against one process."""
import json
import os
import re

import numpy as np
import pytest

import motif_dust_model as md
import motif_erase_model as mer
import motif_holdout_model as mh
import motif_score_model as ms
import motif_shuffle_model as msh
from oracle import oracle as po
from test_gpu_cli import compare_outputs, run_cli
from test_gpu_multirank import GOLD, run_plain, run_ranks

pytestmark = pytest.mark.gpu

W, F, SEED, P = 8, 0.1, 1, 1e-3
WORD = "TGACTCAGCA"


@pytest.fixture(scope="module")
def scenario(tmp_path_factory):
    d = tmp_path_factory.mktemp("holdout")
    seqs = md.tracts(1, f_word=0.3, f_tract=0.0)
    i0, i1 = mh.split(SEED, 0, len(seqs), mh.threshold_of(F))
    fa, train = str(d / "input.fa"), str(d / "train.fa")
    with open(fa, "w") as f:
        f.write(md.fasta_text(seqs))
    with open(train, "w") as f:
        f.write(md.fasta_text([seqs[i] for i in i0]))
    return dict(fa=fa, train=train, seqs=seqs, i0=i0, i1=i1, args=[fa, "-w", str(W), "--score-negatives", "shuffled"])


@pytest.fixture(scope="module")
def run(scenario, tmp_path_factory):
    """the run with the flag, its report and the tables it leaves"""
    d = tmp_path_factory.mktemp("run")
    dump = d / "tables"
    dump.mkdir()
    out = d / "holdout.tsv"
    res = run_plain(scenario["args"] + ["--holdout", str(out)], d, tag="held", extra_env={"PENGK_DUMP_TABLES": str(dump)})
    assert res[0] == 0, res[2].decode()[-2000:]
    return res, out, dump


def assert_same_tsv(got, want):
    """strings and integers exactly; the floating-point columns to the tolerance of the CPU module plus a unit of the last
    printed digit (three decimals), as tests/test_gpu_motif_enrich.py compares the --enrich file"""
    g, w = got.split("\n"), want.split("\n")
    assert g[:2] == w[:2] and len(g) == len(w), (g[:2], w[:2], len(g), len(w))
    assert g[-1] == w[-1] == ""
    for a, b in zip(g[2:-1], w[2:-1]):
        fa, fb = a.split("\t"), b.split("\t")
        assert len(fa) == len(fb) == 13, (a, b)
        assert fa[:5] == fb[:5] and fa[6:10] == fb[6:10], (a, b)
        for k in (5, 10, 11, 12):
            x, y = fa[k], fb[k]
            assert x == y or abs(float(x) - float(y)) <= 1e-9 * abs(float(y)) + 1e-9 + 1.001e-3, (a, b)


def test_the_report_equals_the_model(scenario, run):
    (rc, so, se, meme, js), out, dump = run
    seqs, i0, i1 = scenario["seqs"], scenario["i0"], scenario["i1"]
    ids = [p["iupac_motif"] for p in json.loads(js)["patterns"]]
    ln = np.fromfile(str(dump / "holdout_len.i32"), np.int32)
    S = np.fromfile(str(dump / "holdout_S.i32"), np.int32).reshape(len(ln), 64, 4)
    Ss = [S[m, :ln[m]] for m in range(len(ln))]
    assert len(ids) == len(Ss) >= 1 and [len(x) for x in ids] == ln.tolist()
    V = np.fromfile(str(dump / "V.f32"), np.float32)
    neg = [np.asarray(msh.shuffle(np.where(c >= 1, c - 1, 4), 1, g), np.uint8) + 1 for g, c in enumerate(seqs)]
    sets = [[seqs[i] for i in i0], [neg[i] for i in i0], [seqs[i] for i in i1], [neg[i] for i in i1]]
    res = mh.analyse(sets, Ss, V[:4], P, True)
    assert np.fromfile(str(dump / "holdout_thr.i32"), np.int32).tolist() == [r["thr"] for r in res]
    got = out.read_text()
    print(got)
    assert_same_tsv(got, mh.render(ids, Ss, res, F, SEED, [len(i0), len(i0), len(i1), len(i1)]))
    # the planted word is among the motifs, and the hold-out share confirms it (tests/test_motif_holdout_cpu.py's bound)
    lines = [l.split("\t") for l in got.split("\n")[2:] if l]
    of_word = [l for l in lines if mer.shares_kmer(l[1], WORD)]  # (six letters of it, on either strand)
    assert of_word and min(float(l[11]) for l in of_word) <= -5.0
    m = re.search(rb"holdout \(fraction 0\.1, seed 1\): (\d+) of (\d+) input sequences set aside, motifs are searched on the other (\d+)\n", so)
    assert m and [int(x) for x in m.groups()] == [len(i1), len(seqs), len(i0)], so[:800]


def test_round_1_counted_the_training_share_under_the_whole_inputs_model(scenario, run):
    _, _, dump = run
    seqs, i0 = scenario["seqs"], scenario["i0"]
    counts, ltot = po.count(*ms.flatten([seqs[i] for i in i0]), W, True)
    meta = dict(l.split() for l in (dump / "meta.txt").read_text().splitlines())
    assert int(meta["ltot"]) == ltot and int(meta["N"]) == len(i0)
    assert np.array_equal(np.fromfile(str(dump / "counts.u32"), np.uint32).astype(np.uint64), counts)
    V = np.fromfile(str(dump / "V.f32"), np.float32)
    assert V.tobytes() == po.bg_V(po.bg_counts(*ms.flatten(seqs), 2), 2).tobytes()


def test_the_motifs_are_those_of_the_training_sequences_alone(scenario, run, tmp_path):
    (rc, so, se, meme, js), _, _ = run
    rc2, _, se2, meme2, js2 = run_plain([scenario["train"], "-w", str(W), "--background-sequences", scenario["fa"]], tmp_path)
    assert rc2 == 0, se2.decode()[-2000:]
    assert meme is not None and meme == meme2
    assert js == js2


def test_without_the_flag_the_outputs_are_the_references(scenario, run, tmp_path):
    meme, js, stdout = run_cli(tmp_path, "cli_mafk100_w8")
    ref = os.path.join(GOLD, "cli", "cli_mafk100_w8")
    compare_outputs(meme, js, stdout, ref + ".meme", ref + ".json", open(ref + ".stdout").read(), True)
    # ... and on the scenario the flag's run differs from the run without it, whose stdout has no word of it
    (rc, so, se, meme1, js1), _, _ = run
    rc0, so0, se0, meme0, js0 = run_plain(scenario["args"], tmp_path, tag="plain")
    assert rc0 == 0 and b"holdout" not in so0 and b"holdout" in so
    assert not (tmp_path / "holdout.tsv").exists()


@pytest.mark.parametrize("match", ["none", "gc,length"])
def test_the_flag_beside_a_control_set_the_mask_and_the_erase_rounds(scenario, tmp_path, match):
    """--discriminative, --score-negatives control, --mask-low-complexity and --erase in one run with --holdout: the control
    set is split over its own indices (the sizes on stdout and in the report's header are the model's), round 1 counts the
    training shares, and the word is still found and confirmed"""
    control = md.tracts(11, n=3000, f_word=0.0, f_tract=0.0)
    bg = tmp_path / "control.fa"
    bg.write_text(md.fasta_text(control))
    dump = tmp_path / "tables"
    dump.mkdir()
    out = tmp_path / "holdout.tsv"
    rc, so, se, _, js = run_plain([scenario["fa"], "-w", str(W), "--background-sequences", str(bg), "--discriminative",
                                   "--score-negatives", "control", "--control-match", match, "--mask-low-complexity", "--erase",
                                   str(tmp_path / "erase.tsv"), "--holdout", str(out), "--holdout-seed", "5", "--holdout-fraction", "0.2"],
                                  tmp_path, extra_env={"PENGK_DUMP_TABLES": str(dump)})
    assert rc == 0, se.decode()[-2000:]
    t = mh.threshold_of(0.2)
    i0, i1 = mh.split(5, 0, len(scenario["seqs"]), t)
    c0, c1 = mh.split(5, 0, len(control), t)
    line = "holdout (fraction 0.2, seed 5): %d of %d input sequences set aside, motifs are searched on the other %d; control set: %d of %d set aside\n" % (
        len(i1), len(scenario["seqs"]), len(i0), len(c1), len(control))
    assert line.encode() in so, so[:800]
    head = out.read_text().split("\n")[0]
    print(head)
    sizes = [int(x) for x in re.match(r"# holdout fraction 0.2 seed 5 train_pos (\d+) train_neg (\d+) hold_pos (\d+) hold_neg (\d+)$", head).groups()]
    assert sizes[0::2] == [len(i0), len(i1)]
    if match == "none":
        assert sizes[1::2] == [len(c0), len(c1)]
    else:  # the kept control sequences (global indices), each on the side its index puts it
        kept = np.fromfile(str(dump / "match_kept.u64"), np.uint64)
        cls = mh.classes(5, 0, len(control), t)[kept.astype(np.int64)]
        assert len(kept) > 0 and sizes[1::2] == [int((cls == 0).sum()), int((cls == 1).sum())]
    # round 1 counted the two training shares behind the mask (a few hundred bases even of uniform letters)
    masked, bits, _ = md.mask_codes(scenario["seqs"], 20)
    cmasked, cbits, _ = md.mask_codes(control, 20)
    assert bits > 0 and cbits > 0
    counts, _ = po.count(*ms.flatten([masked[i] for i in i0]), W, True)
    assert np.array_equal(np.fromfile(str(dump / "counts.u32"), np.uint32).astype(np.uint64), counts)
    ctrl, lc = po.count(*ms.flatten([cmasked[i] for i in c0]), W, True)
    assert ("(%d control windows" % lc).encode() in so
    assert np.array_equal(np.fromfile(str(dump / "ctrl_counts.u32"), np.uint32).astype(np.uint64), ctrl)
    lines = [l.split("\t") for l in out.read_text().split("\n")[2:] if l]
    of_word = [l for l in lines if mer.shares_kmer(l[1], WORD)]
    assert of_word and min(float(l[11]) for l in of_word) <= -5.0


def test_two_ranks_write_what_one_process_writes(scenario, run, tmp_path):
    (rc, so, se, meme, js), out, _ = run
    res = run_ranks(scenario["args"] + ["--holdout", str(tmp_path / "holdout.tsv")], 2, tmp_path)
    for rank, (rrc, rso, rse, rmeme, rjs) in enumerate(res):
        assert rrc == 0, (rank, rse.decode()[-2000:])
    assert (res[0][1], res[0][3], res[0][4]) == (so, meme, js) and res[1][1] == b""
    assert (tmp_path / "holdout.tsv").read_bytes() == out.read_bytes()
