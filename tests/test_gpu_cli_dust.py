"""peng_motif --mask-low-complexity: the scenario of tests/motif_dust_model.py (a planted word in 30 % of the sequences, a
poly-A or (CA)n tract in 20 %) as a FASTA file through the CLI at W = 8.  Without the flag a tract's word is reported as
a motif; with it none is, and the planted motif is reported either way.  The validity words, the report, the stdout line
and the round-1 table the run leaves (PENGK_DUMP_TABLES) against the model and the oracle; the flag together with --erase
and with --discriminative; the flag errors; two ranks against one process."""
import json
import re

import numpy as np
import pytest

import motif_dust_model as md
import motif_erase_model as me
import motif_score_model as ms
from oracle import oracle as po
from test_gpu_multirank import run_plain, run_ranks

pytestmark = pytest.mark.gpu

W = 8
WORD = "TGACTCAGCA"


def revcomp_str(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


@pytest.fixture(scope="module")
def scenario(tmp_path_factory):
    d = tmp_path_factory.mktemp("dust")
    seqs = md.tracts(1)
    control = md.tracts(11, f_word=0.0)  # the same kind of tracts, no planted word
    fa, bg = str(d / "input.fa"), str(d / "control.fa")
    with open(fa, "w") as f:
        f.write(md.fasta_text(seqs))
    with open(bg, "w") as f:
        f.write(md.fasta_text(control))
    masked, bits, touched = md.mask_codes(seqs, 20)
    return dict(fa=fa, bg=bg, seqs=seqs, control=control, masked=masked, bits=bits, touched=touched, args=[fa, "-w", str(W)])


@pytest.fixture(scope="module")
def runs(scenario, tmp_path_factory):
    """the run without the flag, and the run with it (which also leaves its tables and its report)"""
    d = tmp_path_factory.mktemp("runs")
    dump = d / "tables"
    dump.mkdir()
    plain = run_plain(scenario["args"], d, tag="plain")
    flagged = run_plain(scenario["args"] + ["--mask-low-complexity", "--mask-report", str(d / "mask.bed")], d, tag="masked",
                        extra_env={"PENGK_DUMP_TABLES": str(dump)})
    return plain, flagged, dump, d / "mask.bed"


def consensus(js):
    """the most probable letter of every column of every reported motif"""
    return ["".join("ACGT"[int(np.argmax(row))] for row in p["pwm"]) for p in json.loads(js)["patterns"]]


def has_word(c):
    return any(WORD[i:i + 7] in c or WORD[i:i + 7] in revcomp_str(c) for i in range(len(WORD) - 6))


def stdout_figures(so, what=b"input"):
    m = re.search(rb"low-complexity mask \(threshold (\d+)\) of the " + what + rb": (\d+) of (\d+) bases masked in (\d+) of (\d+) sequences", so)
    assert m, so[:600]
    return [int(x) for x in m.groups()]


def test_the_tract_is_a_motif_without_the_flag_only(runs):
    (rc0, so0, se0, _, js0), (rc1, so1, se1, _, js1), _, _ = runs
    assert rc0 == 0, se0.decode()[-2000:]
    assert rc1 == 0, se1.decode()[-2000:]
    plain, masked = consensus(js0), consensus(js1)
    print("without the flag:", plain, "with it:", masked)
    assert any(md.period(c) <= 2 for c in plain), plain
    assert masked and not any(md.period(c) <= 2 for c in masked), masked
    assert any(has_word(c) for c in plain) and any(has_word(c) for c in masked)
    assert b"low-complexity mask" in so1 and b"low-complexity mask" not in so0


def test_the_mask_the_report_and_the_table_equal_the_model(scenario, runs):
    _, (rc, so, se, _, _), dump, report = runs
    assert rc == 0, se.decode()[-2000:]
    seqs, masked = scenario["seqs"], scenario["masked"]
    want = me.valid_words(masked)
    got = np.fromfile(str(dump / "mask_valid.u32"), np.uint32)
    assert np.array_equal(got[:len(want)], want)
    assert report.read_text() == md.render_report(md.masked_runs(seqs, masked))
    cnt = np.fromfile(str(dump / "mask_counts.u64"), np.uint64).tolist()
    n_valid = int(sum(int((c >= 1).sum()) for c in seqs))
    assert cnt == [scenario["bits"], n_valid, scenario["touched"], len(seqs)]
    assert stdout_figures(so) == [20] + cnt
    # round 1 counted what the mask left
    counts, ltot = po.count(*ms.flatten(masked), W, True)
    meta = dict(l.split() for l in (dump / "meta.txt").read_text().splitlines())
    assert int(meta["ltot"]) == ltot
    assert np.array_equal(np.fromfile(str(dump / "counts.u32"), np.uint32).astype(np.uint64), counts)
    # ... against the background model of the input as it is
    V = np.fromfile(str(dump / "V.f32"), np.float32)
    assert V.tobytes() == po.bg_V(po.bg_counts(*ms.flatten(seqs), 2), 2).tobytes()


def test_a_threshold_that_masks_nothing_attaches_nothing(scenario, runs, tmp_path):
    (rc0, so0, se0, meme0, js0), _, _, _ = runs
    rc, so, se, meme, js = run_plain(scenario["args"] + ["--mask-low-complexity", "--mask-threshold", "1000", "--mask-report",
                                                         str(tmp_path / "mask.bed")], tmp_path)
    assert rc == 0, se.decode()[-2000:]
    assert stdout_figures(so)[:2] == [1000, 0] and b"nothing to mask" in so
    assert (meme, js) == (meme0, js0) and (tmp_path / "mask.bed").read_bytes() == b""
    line = [l for l in so.splitlines(True) if l.startswith(b"low-complexity mask")]
    assert len(line) == 1 and so.replace(line[0], b"") == so0  # every other byte as without the flag


def test_erase_rounds_start_from_the_masked_input(scenario, tmp_path):
    dump = tmp_path / "tables"
    dump.mkdir()
    rc, so, se, _, js = run_plain(scenario["args"] + ["--mask-low-complexity", "--erase", str(tmp_path / "erase.tsv"),
                                                      "--max-optimized-patterns", "5"], tmp_path, extra_env={"PENGK_DUMP_TABLES": str(dump)})
    assert rc == 0, se.decode()[-2000:]
    assert b"erase round 2:" in so
    assert b"erase round 1: the input behind the low-complexity mask\n" in so and b"the input as it is" not in so
    lc = np.fromfile(str(dump / "mask_valid.u32"), np.uint32)
    r2 = np.fromfile(str(dump / "round2" / "erase_valid.u32"), np.uint32)
    assert len(lc) == len(r2) and not (r2 & ~lc).any() and (lc & ~r2).any()  # no bit comes back; round 2 masks more
    # round 2 counted the model's erase mask of the model's low-complexity mask
    ln = np.fromfile(str(dump / "round2" / "erase_len.i32"), np.int32)
    S = np.fromfile(str(dump / "round2" / "erase_S.i32"), np.int32).reshape(len(ln), 64, 4)
    thr = np.fromfile(str(dump / "round2" / "erase_thr.i32"), np.int32).tolist()
    twice, _, erased = me.mask(scenario["masked"], [S[m, :ln[m]] for m in range(len(ln))], thr, True)
    assert erased > 0
    want = me.valid_words(twice)
    assert np.array_equal(r2[:len(want)], want)
    counts, ltot = po.count(*ms.flatten(twice), W, True)
    assert np.array_equal(np.fromfile(str(dump / "round2" / "counts.u32"), np.uint32).astype(np.uint64), counts)
    assert not any(md.period(c) <= 2 for c in consensus(js)), consensus(js)  # the repeat does not come back in round 2


def test_discriminative_masks_the_control_by_the_same_rule(scenario, tmp_path):
    dump = tmp_path / "tables"
    dump.mkdir()
    rc, so, se, _, js = run_plain(scenario["args"] + ["--background-sequences", scenario["bg"], "--discriminative", "--mask-low-complexity"],
                                  tmp_path, extra_env={"PENGK_DUMP_TABLES": str(dump)})
    assert rc == 0, se.decode()[-2000:]
    cm, cbits, ctouched = md.mask_codes(scenario["control"], 20)
    want = me.valid_words(cm)
    got = np.fromfile(str(dump / "mask_control_valid.u32"), np.uint32)
    assert cbits > 0 and np.array_equal(got[:len(want)], want)
    assert stdout_figures(so, b"control set")[1::2] == [cbits, ctouched]
    ctrl, lc = po.count(*ms.flatten(cm), W, True)
    assert ("(%d control windows" % lc).encode() in so
    assert lc < po.count(*ms.flatten(scenario["control"]), W, True)[1]
    assert np.array_equal(np.fromfile(str(dump / "ctrl_counts.u32"), np.uint32).astype(np.uint64), ctrl)
    counts, _ = po.count(*ms.flatten(scenario["masked"]), W, True)
    assert np.array_equal(np.fromfile(str(dump / "counts.u32"), np.uint32).astype(np.uint64), counts)
    # the background model is trained on the control as it is
    V = np.fromfile(str(dump / "V.f32"), np.float32)
    assert V.tobytes() == po.bg_V(po.bg_counts(*ms.flatten(scenario["control"]), 2), 2).tobytes()


@pytest.mark.parametrize("extra,message", [
    (["--mask-low-complexity", "--mask-threshold", "0"], b"--mask-threshold must be"),
    (["--mask-low-complexity", "--mask-threshold", "1001"], b"--mask-threshold must be"),
    (["--mask-low-complexity", "--mask-threshold", "2x"], b"--mask-threshold must be"),
    (["--mask-threshold", "20"], b"--mask-threshold requires --mask-low-complexity"),
    (["--mask-report", "F"], b"--mask-report requires --mask-low-complexity"),
], ids=["threshold_0", "threshold_1001", "threshold_not_a_number", "threshold_without_the_flag", "report_without_the_flag"])
def test_flag_errors_exit_with_4(scenario, tmp_path, extra, message):
    args = scenario["args"] + [str(tmp_path / "mask.bed") if a == "F" else a for a in extra]
    rc, so, se, meme, js = run_plain(args, tmp_path)
    assert rc == 4 and message in se and b"ERROR" in se, (rc, se.decode()[-500:])
    assert meme is None and js is None and not (tmp_path / "mask.bed").exists()


def test_two_ranks_write_what_one_process_writes(scenario, runs, tmp_path):
    _, (rc, so, se, meme, js), dump, report = runs
    assert rc == 0, se.decode()[-2000:]
    many = tmp_path / "tables"
    many.mkdir()
    res = run_ranks(scenario["args"] + ["--mask-low-complexity", "--mask-report", str(tmp_path / "mask.bed")], 2, tmp_path,
                    extra_env={"PENGK_DUMP_TABLES": str(many)})
    for rank, (rrc, rso, rse, rmeme, rjs) in enumerate(res):
        assert rrc == 0, (rank, rse.decode()[-2000:])
    assert (res[0][1], res[0][3], res[0][4]) == (so, meme, js) and res[1][1] == b""
    assert (tmp_path / "mask.bed").read_bytes() == report.read_bytes()
    for name in ("counts.u32", "z.f32", "meta.txt", "mask_counts.u64"):
        assert (many / name).read_bytes() == (dump / name).read_bytes(), name
