"""peng_motif --erase: the planted scenario of tests/motif_erase_model.py (a strong motif A in half of the sequences, a weak
motif B in 3 %) as a FASTA file through the CLI at W = 8 with five optimised seeds.  Without the flag every reported
motif is a piece of A; with it the second round, on the input with A's sites masked, reports B.  The report and the
tables the rounds leave (PENGK_DUMP_TABLES) against the model and the oracle: one check that ties mask, pack and count
together; the run that stops by itself; the flag errors; two ranks against one process."""
import json

import numpy as np
import pytest

import motif_erase_model as me
import motif_score_model as ms
from oracle import oracle as po
from test_gpu_multirank import run_plain, run_ranks

pytestmark = pytest.mark.gpu

W = 8
A, B = "TGACTCAGCA", "GGCTGGAGTG"
IUPAC = {"A": "A", "C": "C", "G": "G", "T": "T", "S": "CG", "W": "AT", "R": "AG", "Y": "CT", "K": "GT", "M": "AC", "B": "CGT",
         "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}


def shares(motif, word, k=6):
    """an IUPAC motif and a word share a k-mer on either strand: every letter of a k-window of the motif admits the
    word's base"""
    rc = word[::-1].translate(str.maketrans("ACGT", "TGCA"))
    for x in (word, rc):
        for i in range(len(motif) - k + 1):
            for j in range(len(x) - k + 1):
                if all(x[j + t] in IUPAC[motif[i + t]] for t in range(k)):
                    return True
    return False


@pytest.fixture(scope="module")
def scenario(tmp_path_factory):
    d = tmp_path_factory.mktemp("erase")
    seqs = me.planted(1)
    fa = str(d / "input.fa")
    with open(fa, "wb") as f:
        for i, c in enumerate(seqs):
            f.write(b">s%d\n" % i + np.frombuffer(b"NACGT", np.uint8)[c].tobytes() + b"\n")
    return dict(fa=fa, seqs=seqs, args=[fa, "-w", str(W), "--max-optimized-patterns", "5"])


@pytest.fixture(scope="module")
def runs(scenario, tmp_path_factory):
    """the run without the flag, and the run with it (which also leaves its tables and its report)"""
    d = tmp_path_factory.mktemp("runs")
    dump = d / "tables"
    dump.mkdir()
    plain = run_plain(scenario["args"], d, tag="once")
    flagged = run_plain(scenario["args"] + ["--erase", str(d / "erase.tsv")], d, tag="erased", extra_env={"PENGK_DUMP_TABLES": str(dump)})
    return plain, flagged, dump, d / "erase.tsv"


def motifs(js):
    return [p["iupac_motif"] for p in json.loads(js)["patterns"]]


def dumped_mask(dump, r):
    """(S list, thresholds) that round r's mask was made with"""
    ln = np.fromfile(str(dump / ("round%d" % r) / "erase_len.i32"), np.int32)
    S = np.fromfile(str(dump / ("round%d" % r) / "erase_S.i32"), np.int32).reshape(len(ln), 64, 4)
    thr = np.fromfile(str(dump / ("round%d" % r) / "erase_thr.i32"), np.int32)
    return [S[m, :ln[m]] for m in range(len(ln))], thr.tolist()


def meta(path):
    return dict(l.split() for l in path.read_text().splitlines())


def test_the_weak_motif_is_reported_with_the_flag_only(runs):
    (rc0, so0, se0, _, js0), (rc1, so1, se1, _, js1), _, _ = runs
    assert rc0 == 0, se0.decode()[-2000:]
    assert rc1 == 0, se1.decode()[-2000:]
    once, erased = motifs(js0), motifs(js1)
    print("without the flag:", once, "with it:", erased)
    assert once and not any(shares(m, B) for m in once), once
    assert any(shares(m, B) for m in erased), erased
    # round 1 is the run without the flag: its motifs are all there, unchanged (the writers sort the union)
    p0 = {p["iupac_motif"]: p for p in json.loads(js0)["patterns"]}
    p1 = {p["iupac_motif"]: p for p in json.loads(js1)["patterns"]}
    assert set(p0) < set(p1) and all(p1[m] == p0[m] for m in p0)
    assert all(shares(m, B) for m in set(p1) - set(p0))
    # the lines on stdout that name the mode and the rounds; without the flag every byte as before
    assert so1.startswith(b"erase mode: up to 1 further round") and b"erase round 1:" in so1 and b"erase round 2:" in so1
    assert b"erase" not in so0
    trace1 = so1.split(b"erase round 1: the input as it is\n", 1)[1].split(b"\nerase round 2:", 1)[0]
    assert so0.startswith(trace1)


def test_the_report_and_the_tables_equal_the_model(scenario, runs):
    _, (rc, so, se, _, js), dump, report = runs
    assert rc == 0, se.decode()[-2000:]
    seqs = scenario["seqs"]
    # round 2 counted what the model's mask, made from the dumped matrices, leaves of the input
    Ss, thr = dumped_mask(dump, 2)
    masked, n2, erased = me.mask(seqs, Ss, thr, True)
    assert erased > 0
    counts, ltot = po.count(*ms.flatten(masked), W, True)
    m1, m2 = meta(dump / "meta.txt"), meta(dump / "round2" / "meta.txt")
    assert int(m1["ltot"]) == po.count(*ms.flatten(seqs), W, True)[1]
    assert int(m2["ltot"]) == ltot
    assert np.array_equal(np.fromfile(str(dump / "round2" / "counts.u32"), np.uint32).astype(np.uint64), counts)
    # the report: every round's motifs with the thresholds and sites of the mask made from them
    Ss3, thr3 = dumped_mask(dump, 3)
    n3 = me.mask(masked, Ss3, thr3, True)[1]
    lines = [l.split("\t") for l in report.read_text().splitlines()[1:]]
    ids = [[l[1] for l in lines if l[0] == str(r)] for r in (1, 2)]
    assert len(ids[0]) == len(Ss) and len(ids[1]) == len(Ss3) and len(lines) == len(Ss) + len(Ss3)
    seeds = [int(next(l[5] for l in lines if l[0] == str(r))) for r in (1, 2)]
    rounds = [dict(seeds=seeds[0], windows=int(m1["ltot"]), bases_erased=0,
                   motifs=[(i, len(S), t, int(n)) for i, S, t, n in zip(ids[0], Ss, thr, n2)]),
              dict(seeds=seeds[1], windows=ltot, bases_erased=erased,
                   motifs=[(i, len(S), t, int(n)) for i, S, t, n in zip(ids[1], Ss3, thr3, n3)])]
    assert report.read_text() == me.render_report(rounds)
    assert sorted(ids[0] + ids[1]) == sorted(motifs(js))
    assert ("erase round 2: %d bases" % erased).encode() in so
    # the seeds the report counts are the oracle's on the same codes
    V = np.fromfile(str(dump / "V.f32"), np.float32)
    assert V.tobytes() == np.fromfile(str(dump / "round2" / "V.f32"), np.float32).tobytes()  # the round-1 background model
    _, _, z = po.stats(W, counts, po.bgprob(W, 2, V, True), ltot)
    assert seeds[1] == len(po.select(W, z, counts))
    assert np.fromfile(str(dump / "round2" / "z.f32"), np.float32).tobytes() == z.tobytes()


def test_three_rounds_stop_by_themselves(scenario, tmp_path):
    report = tmp_path / "erase.tsv"
    rc, so, se, _, js = run_plain(scenario["args"] + ["--erase", str(report), "--erase-rounds", "3"], tmp_path)
    assert rc == 0, se.decode()[-2000:]
    lines = [l.split("\t") for l in report.read_text().splitlines()[1:]]
    last = int(lines[-1][0])
    print(report.read_text())
    assert 2 <= last <= 3 and b"erase round %d:" % (last + 1) not in so  # (a fourth round would have been allowed)
    assert lines[-1][1] == "-" and lines[-1][4] == "0"                   # the round that ran and reported nothing
    assert int(lines[-1][7]) > int(lines[0][7]) == 0


@pytest.mark.parametrize("extra,message", [
    (["--erase", "F", "--erase-rounds", "0"], b"--erase-rounds must be"),
    (["--erase", "F", "--erase-rounds", "9"], b"--erase-rounds must be"),
    (["--erase", "F", "--erase-rounds", "2x"], b"--erase-rounds must be"),
    (["--erase", "F", "--erase-pvalue", "0"], b"--erase-pvalue must be"),
    (["--erase", "F", "--erase-pvalue", "1.5"], b"--erase-pvalue must be"),
    (["--erase", "F", "--erase-pvalue", "nan"], b"--erase-pvalue must be"),
], ids=["rounds_0", "rounds_9", "rounds_not_a_number", "pvalue_0", "pvalue_above_1", "pvalue_nan"])
def test_flag_errors_exit_with_4(scenario, tmp_path, extra, message):
    args = scenario["args"] + [str(tmp_path / "erase.tsv") if a == "F" else a for a in extra]
    rc, so, se, meme, js = run_plain(args, tmp_path)
    assert rc == 4 and message in se and b"ERROR" in se, (rc, se.decode()[-500:])
    assert meme is None and js is None and not (tmp_path / "erase.tsv").exists()


def test_two_ranks_write_what_one_process_writes(scenario, runs, tmp_path):
    _, (rc, so, se, meme, js), dump, report = runs
    assert rc == 0, se.decode()[-2000:]
    many = tmp_path / "tables"
    many.mkdir()
    res = run_ranks(scenario["args"] + ["--erase", str(tmp_path / "erase.tsv")], 2, tmp_path, extra_env={"PENGK_DUMP_TABLES": str(many)})
    for rank, (rrc, rso, rse, rmeme, rjs) in enumerate(res):
        assert rrc == 0, (rank, rse.decode()[-2000:])
    assert (res[0][1], res[0][3], res[0][4]) == (so, meme, js) and res[1][1] == b""
    assert (tmp_path / "erase.tsv").read_bytes() == report.read_bytes()
    for name in ("counts.u32", "z.f32", "meta.txt", "erase_thr.i32"):
        assert (many / "round2" / name).read_bytes() == (dump / "round2" / name).read_bytes(), name
