"""peng_motif --positional: seed 1 of the README's scenario (TATAWAWR laid into 10 % of 2 000 sequences at 70 % A+T, at
60 +- 2) as a FASTA file through the CLI.  The TSV against the model's table and pengk_position_summary line for line, the
main outputs byte for byte without the flag, the flag beside --mask-low-complexity and --holdout (the masked training share
is what is counted), two ranks against one process, and the other options."""
import re

import pytest

import peng_motif_amd as pk
import motif_dust_model as md
import motif_holdout_model as mh
import motif_positional_model as mp
from test_gpu_multirank import run_plain, run_ranks

pytestmark = pytest.mark.gpu

W = 8
START = ["--positional-anchor", "start"]


@pytest.fixture(scope="module")
def scenario(tmp_path_factory):
    d = tmp_path_factory.mktemp("positional")
    seqs = mp.planted(1)
    fa = str(d / "input.fa")
    with open(fa, "w") as f:
        f.write(mp.fasta_text(seqs))
    return dict(fa=fa, seqs=seqs, args=[fa, "-w", str(W)])


@pytest.fixture(scope="module")
def runs(scenario, tmp_path_factory):
    d = tmp_path_factory.mktemp("runs")
    plain = run_plain(scenario["args"], d, tag="plain")
    flagged = run_plain(scenario["args"] + ["--positional", str(d / "positional.tsv")] + START, d, tag="positional")
    return plain, flagged, d / "positional.tsv"


def model_tsv(seqs, K=6, anchor=mp.START, S=10, B=20, both=True, min_count=5, E=0.01):
    counts = mp.tables(seqs, K, anchor, S, B, both)
    return mp.render_tsv(pk.position_summary(counts, K, both, min_count, E), counts, K)


def rows(tsv):
    lines = tsv.read_text().splitlines()
    assert lines[0].split("\t") == mp.COLUMNS
    return [dict(zip(mp.COLUMNS, l.split("\t"))) for l in lines[1:]]


def test_the_tsv_is_the_model_line_by_line(scenario, runs):
    _, (rc, so, se, _, _), tsv = runs
    assert rc == 0, se.decode()[-2000:]
    want = model_tsv(scenario["seqs"])
    got = tsv.read_text()
    for n, (g, w) in enumerate(zip(got.splitlines(), want.splitlines())):
        assert g == w, "line %d" % n
    assert got == want
    counts = mp.tables(scenario["seqs"], 6, mp.START, 10, 20, True)
    assert got == mp.render_tsv(mp.summary(counts, 6, True, pk.binomial_log10_sf), counts, 6)
    r = rows(tsv)
    assert r[0]["word"] == "TATAAA" and r[0]["bin"] == "6" and r[0]["is_head"] == "1" and len(r[0]["profile"].split(",")) == 20
    m = re.search(rb"^positional \(width 6, 20 bins of 10 from the start, both strands, (\d+) words\): (\d+) at E-value <= 0.01 in (\d+) "
                  rb"famil(?:y|ies); the first: TATAAA in bin 6, (\d+) times$", so, re.M)
    assert m, so[:1500]
    assert int(m.group(1)) == int(counts.sum()) and int(m.group(2)) == len(r) and m.group(4).decode() == r[0]["count"]
    assert int(m.group(3)) == sum(x["is_head"] == "1" for x in r)


def test_without_the_flag_the_outputs_are_what_they_were(runs):
    (rc0, so0, se0, meme0, js0), (rc1, so1, se1, meme1, js1), _ = runs
    assert rc0 == 0 and rc1 == 0
    assert (meme0, js0) == (meme1, js1) and meme0 is not None
    line = [l for l in so1.splitlines(True) if l.startswith(b"positional (")]
    assert len(line) == 1 and so1.replace(line[0], b"") == so0 and b"positional" not in so0


def test_behind_the_mask_and_beside_a_holdout_share_the_masked_training_share_is_counted(scenario, tmp_path):
    args = scenario["args"] + ["--mask-low-complexity", "--holdout", str(tmp_path / "holdout.tsv"), "--positional", str(tmp_path / "p.tsv")] + START
    rc, so, se, _, _ = run_plain(args, tmp_path)
    assert rc == 0, se.decode()[-2000:]
    seqs = scenario["seqs"]
    masked, bits, _ = md.mask_codes(seqs, 20)
    train, hold = mh.split(1, 0, len(seqs), mh.threshold_of(0.1))
    assert bits > 1000 and 100 < len(hold) < 300
    want = model_tsv([masked[i] for i in train])
    assert (tmp_path / "p.tsv").read_text() == want
    # ... and it is neither the whole input's, nor the unmasked share's, nor the masked whole's
    assert len({want, model_tsv(seqs), model_tsv([seqs[i] for i in train]), model_tsv(masked)}) == 4


def test_two_ranks_write_what_one_process_writes(scenario, runs, tmp_path):
    _, (rc, so, se, meme, js), tsv = runs
    res = run_ranks(scenario["args"] + ["--positional", str(tmp_path / "positional.tsv")] + START, 2, tmp_path)
    for rank, (rrc, rso, rse, rmeme, rjs) in enumerate(res):
        assert rrc == 0, (rank, rse.decode()[-2000:])
    assert (res[0][1], res[0][3], res[0][4]) == (so, meme, js) and res[1][1] == b""
    assert (tmp_path / "positional.tsv").read_bytes() == tsv.read_bytes()


def test_other_options_reach_the_report(scenario, tmp_path):
    """plus strand, five letters, the center anchor (the default), bins of 7, a looser E-value and a count floor"""
    rc, so, se, _, _ = run_plain(scenario["args"] + ["--strand", "PLUS", "--positional", str(tmp_path / "p.tsv"), "--positional-width", "5",
                                                     "--positional-bin-size", "7", "--positional-bins", "13", "--positional-evalue", "50",
                                                     "--positional-min-count", "30"], tmp_path)
    assert rc == 0, se.decode()[-2000:]
    want = model_tsv(scenario["seqs"], 5, mp.CENTER, 7, 13, False, 30, 50.0)
    assert len(want.splitlines()) > 4 and (tmp_path / "p.tsv").read_text() == want
    assert b"positional (width 5, 13 bins of 7 from the center, plus strand, " in so
    rc, so, se, _, _ = run_plain(scenario["args"] + ["--positional", str(tmp_path / "e.tsv"), "--positional-anchor", "end",
                                                     "--positional-width", "7", "--positional-evalue", "10"], tmp_path, tag="end")
    assert rc == 0, se.decode()[-2000:]
    assert (tmp_path / "e.tsv").read_text() == model_tsv(scenario["seqs"], 7, mp.END, 10, 20, True, 5, 10.0)
