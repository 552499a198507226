"""peng_motif --score-negatives control: the scenario of tests/motif_match_model.py (an input at 60 % GC, a control that is
half AT-rich and half three times as long, a GC-rich word that is planted nowhere) as two FASTA files through the CLI with
--score-motifs and --enrich.  The JSON's zoops_score, the enrichment table, the match report, the dumped counts, quotas
and kept indices against the models; --control-match none against the default; two ranks against one process; and the
control flags doing nothing while the negatives are sampled."""
import json
import math

import numpy as np
import pytest

import motif_compare_model as mc
import motif_enrich_model as me
import motif_match_model as mm
import motif_score_model as ms
from oracle import oracle as po
from test_gpu_motif_enrich import assert_same_tsv
from test_gpu_multirank import run_plain, run_ranks

pytestmark = pytest.mark.gpu

NAMES = ["GCRICH", "ATRICH", "MIXED"]
WORDS = [mm.GC_RICH_8MER, "ATTATAAT", "ACGTTGCA"]


def write_fasta(path, seqs, tag):
    with open(path, "wb") as f:
        for i, c in enumerate(seqs):
            f.write(b">%s%d\n" % (tag, i) + np.frombuffer(b"NACGT", np.uint8)[c].tobytes() + b"\n")


@pytest.fixture(scope="module")
def scenario(tmp_path_factory):
    d = tmp_path_factory.mktemp("control")
    pos, ctrl = mm.scenario(1)
    fa, cfa, db = str(d / "input.fa"), str(d / "control.fa"), str(d / "db.meme")
    write_fasta(fa, pos, b"in")
    write_fasta(cfa, ctrl, b"ctl")
    rows = [mm.word_pwm(w) for w in WORDS]
    mc.write_meme(db, NAMES, rows)
    codes, offs = ms.flatten(ctrl)  # the background model is the control's (order 2, the CLI's default)
    bg0 = np.asarray(po.bg_V(po.bg_counts(codes, offs, 2), 2), np.float32)[0:4]
    return dict(dir=d, pos=pos, ctrl=ctrl, rows=rows, db=db, bg0=bg0, args=[fa, "-w", "8", "--background-sequences", cfa])


def control_args(sc, d, tag, extra=()):
    return sc["args"] + ["--score-motifs", "--enrich", str(d / (tag + ".enrich.tsv")), "--enrich-db", sc["db"], "--score-negatives",
                         "control", "--control-match-report", str(d / (tag + ".match.tsv"))] + list(extra)


@pytest.fixture(scope="module")
def runs(scenario, tmp_path_factory):
    """the default match (which also leaves its tables) and --control-match none"""
    d = tmp_path_factory.mktemp("runs")
    dump = d / "tables"
    dump.mkdir()
    matched = run_plain(control_args(scenario, d, "m"), d, tag="m", extra_env={"PENGK_DUMP_TABLES": str(dump)})
    whole = run_plain(control_args(scenario, d, "w", ["--control-match", "none"]), d, tag="w")
    return d, dump, matched, whole


@pytest.fixture(scope="module")
def model(scenario):
    pos, ctrl = scenario["pos"], scenario["ctrl"]
    _, h_in = mm.strata(pos)
    s_ctrl, h_ctrl = mm.strata(ctrl)
    quota, short = mm.quotas(h_in, h_ctrl, 1)
    kept = mm.select(s_ctrl, h_ctrl, quota)
    return dict(h_in=h_in, h_ctrl=h_ctrl, quota=quota, short=short, kept=kept, matched=[ctrl[i] for i in kept])


def check_scores(js, pos, negs, bg0):
    """the JSON's zoops_score / occur against the model's from the written PWMs (to the digits the PWMs are written with,
    as tests/test_gpu_motif_score.py compares them)"""
    pats = json.loads(js)["patterns"]
    assert pats
    for p in pats:
        S = ms.log_odds(np.array(p["pwm"], np.float32), bg0)
        lo, hi = ms.score_range(S)
        P = ms.histogram(ms.best_scores(pos, S, True), lo, hi)
        N = ms.histogram(ms.best_scores(negs, S, True), lo, hi)
        assert int(N.sum()) == len(negs)
        assert abs(ms.auc(P, N) - p["zoops_score"]) < 1e-3, p["iupac_motif"]
        assert abs(ms.occur(P, N) - p["occur"]) < 1e-3, p["iupac_motif"]
    return pats


def test_the_matched_run_equals_the_models(scenario, runs, model):
    d, dump, (rc, so, se, meme, js), _ = runs
    assert rc == 0, se.decode()[-2000:]
    # the match: counts, quotas, kept indices, the report, the line on stdout
    for name, want in (("match_input", model["h_in"]), ("match_control", model["h_ctrl"]), ("match_quota", model["quota"]),
                       ("match_kept", model["kept"].astype(np.uint64))):
        assert np.array_equal(np.fromfile(str(dump / (name + ".u64")), np.uint64), want), name
    assert (d / "m.match.tsv").read_text() == mm.report(model["h_in"], model["h_ctrl"], model["quota"], 10, True)
    line = [l for l in so.decode().splitlines() if l.startswith("control negatives:")]
    assert line == ["control negatives: matched by gc,length (10 GC bins, ratio 1): %d strata in use, kept %d of 6000 control "
                    "sequences, shortfall %d" % (int((model["h_in"] > 0).sum()), len(model["kept"]), model["short"])]
    # the scores and the enrichment table against the matched control
    check_scores(js, scenario["pos"], model["matched"], scenario["bg0"])
    res = me.analyse(me.Packed(scenario["pos"]), me.Packed(model["matched"]), scenario["rows"], scenario["bg0"], 1e-3, True)
    assert_same_tsv((d / "m.enrich.tsv").read_text(), me.render(NAMES, [""] * 3, res))


def test_the_whole_control_calls_the_gc_rich_word_enriched_and_the_matched_one_does_not(scenario, runs, model):
    d, _, (rc0, so0, _, _, js0), (rc1, so1, se1, _, js1) = runs
    assert rc0 == 0 and rc1 == 0, se1.decode()[-2000:]
    assert b"control negatives: matched by none: kept 6000 of 6000 control sequences\n" in so1 and not (d / "w.match.tsv").exists()
    check_scores(js1, scenario["pos"], scenario["ctrl"], scenario["bg0"])
    res = me.analyse(me.Packed(scenario["pos"]), me.Packed(scenario["ctrl"]), scenario["rows"], scenario["bg0"], 1e-3, True)
    assert_same_tsv((d / "w.enrich.tsv").read_text(), me.render(NAMES, [""] * 3, res))
    row = {}
    for tag in "mw":
        lines = [l.split("\t") for l in (d / (tag + ".enrich.tsv")).read_text().splitlines()[1:]]
        row[tag] = next(l for l in lines if l[1] == "GCRICH")
        print(tag, "\t".join(row[tag]))
    assert int(row["w"][9]) == 6000 and int(row["m"][9]) == len(model["kept"])  # neg_scored
    assert float(row["w"][12]) < math.log10(0.05) < float(row["m"][12])  # log10_adj_pvalue


def test_two_ranks_write_what_one_process_writes(scenario, runs):
    d, _, (rc, so, se, meme, js), _ = runs
    assert rc == 0
    res = run_ranks(control_args(scenario, d, "r"), 2, d, tag="r")
    assert [r[0] for r in res] == [0, 0], res[0][2].decode()[-2000:] + res[1][2].decode()[-2000:]
    assert (res[0][1], res[0][3], res[0][4]) == (so, meme, js) and res[1][1] == b""
    assert (d / "r.enrich.tsv").read_bytes() == (d / "m.enrich.tsv").read_bytes()
    assert (d / "r.match.tsv").read_bytes() == (d / "m.match.tsv").read_bytes()


def test_the_control_flags_do_nothing_while_the_negatives_are_sampled(scenario, tmp_path):
    rc, so0, se, meme0, js0 = run_plain(scenario["args"] + ["--score-motifs"], tmp_path, tag="a")
    assert rc == 0, se.decode()[-2000:]
    rc, so1, se, meme1, js1 = run_plain(scenario["args"] + ["--score-motifs", "--control-match", "gc", "--control-match-gc-bins", "4",
                                                           "--control-ratio", "3"], tmp_path, tag="b")
    assert rc == 0, se.decode()[-2000:]
    assert (so1, meme1, js1) == (so0, meme0, js0) and b"control negatives" not in so0


def test_no_control_sequence_left_ends_the_run(scenario, tmp_path):
    """a control whose every sequence is far longer than the input's: no stratum in common"""
    cfa = str(tmp_path / "long.fa")
    write_fasta(cfa, mm.draw(np.random.default_rng(2), 20, 5000, 0.6), b"long")
    rc, so, se, meme, js = run_plain([scenario["args"][0], "-w", "8", "--background-sequences", cfa, "--score-motifs",
                                      "--score-negatives", "control"], tmp_path, tag="none")
    assert rc == 4 and b"no control sequence matches the input" in se.splitlines()[-2] and js is None
