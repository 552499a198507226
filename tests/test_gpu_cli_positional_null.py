"""peng_motif --positional-null: seed 1 of the gradient scenario (2 000 sequences whose G+C share falls from 65 % at the
centre to 35 % at the ends, TGACTCA laid into 5 % at the centre) as a FASTA file through the CLI.  The TSV under
`composition` against the model's line for line; under `flat` and without the flag byte for byte what it was; the main
outputs unchanged by the flag; two ranks against one process; and beside --mask-low-complexity and --holdout the masked
training share."""
import re

import pytest

import peng_motif_amd as pk
import motif_dust_model as md
import motif_holdout_model as mh
import motif_positional_model as mp
import positional_null_model as pn
from test_gpu_multirank import run_plain, run_ranks

pytestmark = pytest.mark.gpu

W = 8
SHAPE = ["--positional-bins", "10"]     # anchor centre, K 6, S 10 by default
COMPOSITION = ["--positional-null", "composition"]


@pytest.fixture(scope="module")
def scenario(tmp_path_factory):
    d = tmp_path_factory.mktemp("positional_null")
    seqs = pn.gradient(1, 0.05)
    fa = str(d / "input.fa")
    with open(fa, "w") as f:
        f.write(mp.fasta_text(seqs))
    return dict(fa=fa, seqs=seqs, args=[fa, "-w", str(W)])


@pytest.fixture(scope="module")
def runs(scenario, tmp_path_factory):
    d = tmp_path_factory.mktemp("runs")
    out = {}
    for tag, extra in (("none", []), ("flat", ["--positional-null", "flat"]), ("composition", COMPOSITION)):
        tsv = d / (tag + ".tsv")
        out[tag] = run_plain(scenario["args"] + ["--positional", str(tsv)] + SHAPE + extra, d, tag=tag) + (tsv,)
    out["plain"] = run_plain(scenario["args"], d, tag="plain")
    return out


def model_tsv(seqs, K=6, anchor=mp.CENTER, S=10, B=10, both=True, min_count=5, E=0.01):
    counts = mp.tables(seqs, K, anchor, S, B, both)
    pairs = pn.pair_tables(seqs, K, anchor, S, B, both)
    return pn.render_tsv(pk.position_summary(counts, K, both, min_count, E, pairs=pairs), counts, K)


def test_the_tsv_under_composition_is_the_model_line_by_line(scenario, runs):
    rc, so, se, _, _, tsv = runs["composition"]
    assert rc == 0, se.decode()[-2000:]
    want = model_tsv(scenario["seqs"])
    got = tsv.read_text()
    for n, (g, w) in enumerate(zip(got.splitlines(), want.splitlines())):
        assert g == w, "line %d" % n
    assert got == want
    counts = mp.tables(scenario["seqs"], 6, mp.CENTER, 10, 10, True)
    pairs = pn.pair_tables(scenario["seqs"], 6, mp.CENTER, 10, 10, True)
    assert got == pn.render_tsv(pn.summary(counts, pairs, 6, True, pk.binomial_log10_sf), counts, 6)
    lines = got.splitlines()
    assert lines[0].split("\t") == pn.COLUMNS and lines[0].split("\t")[6:8] == ["expected", "flat_expected"]
    r = [dict(zip(pn.COLUMNS, l.split("\t"))) for l in lines[1:]]
    assert 3 <= len(r) <= 10 and r[0]["word"] == "GACTCA" and r[0]["bin"] == "0"
    assert (r[0]["expected"], r[0]["flat_expected"]) == ("23.53", "24.81")      # (GACTCA in the G+C-rich centre: the flat null asks less)
    m = re.search(rb"^positional \(width 6, 10 bins of 10 from the center, both strands, (\d+) words, composition null\): (\d+) at "
                  rb"E-value <= 0.01 in (\d+) famil(?:y|ies); the first: GACTCA in bin 0, (\d+) times$", so, re.M)
    assert m, so[:1500]
    assert int(m.group(1)) == int(counts.sum()) and int(m.group(2)) == len(r) and m.group(4).decode() == r[0]["count"]


def test_flat_and_no_flag_write_what_they_wrote(scenario, runs):
    (rc0, so0, se0, meme0, js0, tsv0), (rc1, so1, se1, meme1, js1, tsv1) = runs["none"], runs["flat"]
    assert rc0 == 0 and rc1 == 0, (se0.decode()[-1000:], se1.decode()[-1000:])
    counts = mp.tables(scenario["seqs"], 6, mp.CENTER, 10, 10, True)
    want = mp.render_tsv(mp.summary(counts, 6, True, pk.binomial_log10_sf), counts, 6)
    assert tsv0.read_bytes() == tsv1.read_bytes() == want.encode()
    assert len(want.splitlines()) > 200        # the list of composition that the flat null makes of this input
    assert (so0, meme0, js0) == (so1, meme1, js1) and b"composition" not in so0


def test_the_main_outputs_are_unchanged_by_the_flag(runs):
    rc, so, se, meme, js = runs["plain"]
    assert rc == 0 and meme is not None
    for tag in ("none", "flat", "composition"):
        rc1, so1, se1, meme1, js1, _ = runs[tag]
        assert rc1 == 0 and (meme1, js1) == (meme, js)
        line = [l for l in so1.splitlines(True) if l.startswith(b"positional (")]
        assert len(line) == 1 and so1.replace(line[0], b"") == so and b"positional" not in so


def test_two_ranks_write_what_one_process_writes(scenario, runs, tmp_path):
    rc, so, se, meme, js, tsv = runs["composition"]
    res = run_ranks(scenario["args"] + ["--positional", str(tmp_path / "p.tsv")] + SHAPE + COMPOSITION, 2, tmp_path)
    for rank, (rrc, rso, rse, rmeme, rjs) in enumerate(res):
        assert rrc == 0, (rank, rse.decode()[-2000:])
    assert (res[0][1], res[0][3], res[0][4]) == (so, meme, js) and res[1][1] == b""
    assert (tmp_path / "p.tsv").read_bytes() == tsv.read_bytes()


def test_behind_the_mask_and_beside_a_holdout_share_the_masked_training_share_is_counted(scenario, tmp_path):
    args = scenario["args"] + ["--mask-low-complexity", "--holdout", str(tmp_path / "holdout.tsv"), "--positional", str(tmp_path / "p.tsv")]
    rc, so, se, _, _ = run_plain(args + SHAPE + COMPOSITION + ["--positional-evalue", "100"], tmp_path)
    assert rc == 0, se.decode()[-2000:]
    seqs = scenario["seqs"]
    masked, bits, _ = md.mask_codes(seqs, 20)
    train, hold = mh.split(1, 0, len(seqs), mh.threshold_of(0.1))
    assert bits > 0 and 100 < len(hold) < 300
    want = model_tsv([masked[i] for i in train], E=100.0)
    assert (tmp_path / "p.tsv").read_text() == want
    # ... and it is neither the whole input's, nor the unmasked share's, nor the masked whole's
    assert len({want, model_tsv(seqs, E=100.0), model_tsv([seqs[i] for i in train], E=100.0), model_tsv(masked, E=100.0)}) == 4
