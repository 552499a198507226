"""peng_motif --dyads: seed 1 of the README's scenario (CGG n11 CCG laid into 30 % of 2 000 uniform sequences, either
strand) as a FASTA file through the CLI.  The TSV against the model's tables and pengk_dyad_summary line for line, the one
family, the refined motif of --dyads-motifs, the main outputs byte for byte without the flag, two ranks against one
process, the flag behind --mask-low-complexity and beside --holdout, and the flag errors."""
import re

import numpy as np
import pytest

import peng_motif_amd as pk
import motif_dust_model as md
import motif_dyads_model as dy
import motif_holdout_model as mh
from test_gpu_multirank import run_plain, run_ranks

pytestmark = pytest.mark.gpu

W = 8


@pytest.fixture(scope="module")
def scenario(tmp_path_factory):
    d = tmp_path_factory.mktemp("dyads")
    seqs = dy.planted(1)
    fa = str(d / "input.fa")
    with open(fa, "w") as f:
        f.write(dy.fasta_text(seqs))
    return dict(fa=fa, seqs=seqs, args=[fa, "-w", str(W)])


@pytest.fixture(scope="module")
def runs(scenario, tmp_path_factory):
    d = tmp_path_factory.mktemp("runs")
    plain = run_plain(scenario["args"], d, tag="plain")
    flagged = run_plain(scenario["args"] + ["--dyads", str(d / "dyads.tsv"), "--dyads-motifs", str(d / "heads.meme")], d, tag="dyads")
    return plain, flagged, d / "dyads.tsv", d / "heads.meme"


def rows(tsv):
    lines = tsv.read_text().splitlines()
    assert lines[0].split("\t") == dy.COLUMNS
    return [dict(zip(dy.COLUMNS, l.split("\t"))) for l in lines[1:]]


def test_the_planted_dyad_is_line_1_and_the_only_family(runs):
    _, (rc, so, se, _, _), tsv, _ = runs
    assert rc == 0, se.decode()[-2000:]
    r = rows(tsv)
    assert r[0]["dyad"] == "CGG" + "n" * 11 + "CCG" and r[0]["gap"] == "11" and r[0]["is_head"] == "1"
    assert {x["family"] for x in r} == {"1"} and sum(x["is_head"] == "1" for x in r) == 1
    m = re.search(rb"^dyads \(gaps 0\.\.20, both strands, (\d+) triplets\): (\d+) at E-value <= 0.01 in 1 family; the first: CGGn{11}CCG, (\d+) times$",
                  so, re.M)
    assert m, so[:1500]
    assert int(m.group(1)) == 2000 * 98 and int(m.group(2)) == len(r) and m.group(3).decode() == r[0]["count"]


def test_the_tsv_is_the_model_and_the_summary(scenario, runs):
    _, _, tsv, _ = runs
    counts, mono = dy.tables(scenario["seqs"], 20, True)
    assert tsv.read_text() == dy.render_tsv(pk.dyad_summary(counts, mono, True))
    assert tsv.read_text() == dy.render_tsv(dy.summary(counts, mono, True, pk.binomial_log10_sf))


def test_the_refined_motif_has_17_columns_and_reads_the_half_sites(runs):
    _, _, _, meme = runs
    text = meme.read_text()
    names = re.findall(r"^MOTIF (\S+)$", text, re.M)
    assert names == ["CGG" + "n" * 11 + "CCG"]
    m = re.search(r"alength= 4 w= (\d+) nsites= (\d+) iterations= (\d+)", text)
    assert m and int(m.group(1)) == 17 and int(m.group(2)) > 500 and int(m.group(3)) >= 1
    pwm = np.array([[float(x) for x in l.split()] for l in text.split("letter-probability matrix")[1].splitlines()[1:18]])
    assert pwm.shape == (17, 4) and np.allclose(pwm.sum(axis=1), 1.0, atol=1e-6)
    cons = "".join("ACGT"[int(np.argmax(r))] for r in pwm)
    assert cons[:3] == "CGG" and cons[-3:] == "CCG"


def test_without_the_flag_the_main_outputs_are_what_they_were(runs):
    (rc0, so0, se0, meme0, js0), (rc1, so1, se1, meme1, js1), _, _ = runs
    assert rc0 == 0 and rc1 == 0
    assert (meme0, js0) == (meme1, js1) and meme0 is not None
    line = [l for l in so1.splitlines(True) if l.startswith(b"dyads (")]
    assert len(line) == 1 and so1.replace(line[0], b"") == so0 and b"dyads" not in so0


def test_two_ranks_write_what_one_process_writes(scenario, runs, tmp_path):
    _, (rc, so, se, meme, js), tsv, motifs = runs
    res = run_ranks(scenario["args"] + ["--dyads", str(tmp_path / "dyads.tsv"), "--dyads-motifs", str(tmp_path / "dyads.meme")], 2,
                    tmp_path)
    for rank, (rrc, rso, rse, rmeme, rjs) in enumerate(res):
        assert rrc == 0, (rank, rse.decode()[-2000:])
    assert (res[0][1], res[0][3], res[0][4]) == (so, meme, js) and res[1][1] == b""
    assert (tmp_path / "dyads.tsv").read_bytes() == tsv.read_bytes()
    assert (tmp_path / "dyads.meme").read_bytes() == motifs.read_bytes()


def test_behind_the_mask_the_tracts_dyads_are_gone(tmp_path):
    seqs = md.tracts(1)
    fa = str(tmp_path / "tracts.fa")
    with open(fa, "w") as f:
        f.write(md.fasta_text(seqs))
    out = {}
    for tag, extra in (("plain", []), ("masked", ["--mask-low-complexity"])):
        rc, so, se, _, _ = run_plain([fa, "-w", str(W), "--dyads", str(tmp_path / (tag + ".tsv"))] + extra, tmp_path, tag=tag)
        assert rc == 0, se.decode()[-2000:]
        out[tag] = [x["dyad"] for x in rows(tmp_path / (tag + ".tsv"))]
    poly = lambda names: {x for x in names if re.fullmatch(r"AAAn*AAA", x)}
    print("AAA n AAA dyads: %d without the mask, %d behind it" % (len(poly(out["plain"])), len(poly(out["masked"]))))
    assert len(poly(out["plain"])) >= 10 and not (poly(out["plain"]) & poly(out["masked"]))
    # ... and the count behind the mask is the model's count of the masked codes
    masked, _, _ = md.mask_codes(seqs, 20)
    counts, mono = dy.tables(masked, 20, True)
    assert (tmp_path / "masked.tsv").read_text() == dy.render_tsv(pk.dyad_summary(counts, mono, True))


def test_with_a_holdout_share_the_training_share_is_counted(scenario, tmp_path):
    """--holdout sets a tenth aside before anything is counted: the dyads are those of the rest, on one rank and on two"""
    args = scenario["args"] + ["--holdout", str(tmp_path / "holdout.tsv"), "--dyads", str(tmp_path / "d.tsv")]
    rc, so, se, _, _ = run_plain(args, tmp_path)
    assert rc == 0, se.decode()[-2000:]
    seqs = scenario["seqs"]
    train, hold = mh.split(1, 0, len(seqs), mh.threshold_of(0.1))
    assert 100 < len(hold) < 300
    counts, mono = dy.tables([seqs[i] for i in train], 20, True)
    want = dy.render_tsv(pk.dyad_summary(counts, mono, True))
    assert (tmp_path / "d.tsv").read_text() == want
    assert want != dy.render_tsv(pk.dyad_summary(*dy.tables(seqs, 20, True), True))
    two = tmp_path / "two"
    two.mkdir()
    res = run_ranks(scenario["args"] + ["--holdout", str(two / "holdout.tsv"), "--dyads", str(two / "d.tsv")], 2, two)
    assert [r[0] for r in res] == [0, 0], res[0][2].decode()[-2000:]
    assert (two / "d.tsv").read_text() == want


@pytest.mark.parametrize("extra,message", [
    (["--dyads", "F", "--dyads-max-gap", "27"], b"--dyads-max-gap must be"),
    (["--dyads", "F", "--dyads-max-gap", "-1"], b"--dyads-max-gap must be"),
    (["--dyads", "F", "--dyads-evalue", "0"], b"--dyads-evalue must be"),
    (["--dyads", "F", "--dyads-min-count", "0"], b"--dyads-min-count must be"),
    (["--dyads", "F", "--dyads-top", "0"], b"--dyads-top must be"),
    (["--dyads", "F", "--dyads-pvalue", "2"], b"--dyads-pvalue must be"),
    (["--dyads-max-gap", "10"], b"--dyads-max-gap requires --dyads"),
    (["--dyads-motifs", "F"], b"--dyads-motifs requires --dyads"),
], ids=["gap_27", "gap_negative", "evalue_0", "min_count_0", "top_0", "pvalue_2", "gap_without_the_flag", "motifs_without_the_flag"])
def test_flag_errors_exit_with_4(scenario, tmp_path, extra, message):
    args = scenario["args"] + [str(tmp_path / "dyads.out") if a == "F" else a for a in extra]
    rc, so, se, meme, js = run_plain(args, tmp_path)
    assert rc == 4 and message in se and b"ERROR" in se, (rc, se.decode()[-500:])
    assert meme is None and js is None and not (tmp_path / "dyads.out").exists()


def test_other_options_reach_the_report(scenario, tmp_path):
    """plus strand, gaps 0..12, a looser E-value and a count floor: the model under the same settings"""
    rc, so, se, _, _ = run_plain(scenario["args"] + ["--strand", "PLUS", "--dyads", str(tmp_path / "d.tsv"), "--dyads-max-gap", "12",
                                                     "--dyads-evalue", "5", "--dyads-min-count", "70"], tmp_path)
    assert rc == 0, se.decode()[-2000:]
    counts, mono = dy.tables(scenario["seqs"], 12, False)
    want = pk.dyad_summary(counts, mono, False, 70, 5.0)
    assert len(want) > 3 and (tmp_path / "d.tsv").read_text() == dy.render_tsv(want)
