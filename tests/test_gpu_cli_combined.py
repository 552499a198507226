"""Every report beside the flags that change what the search sees.

--mask-low-complexity, --holdout, --erase and --dyads change what round 1 of the search is run on, through process-wide state
that host/main.cpp attaches and detaches (override_packed_input, override_control_input, override_sequence_count,
set_dump_subdir).  The other half of the promise -- the background model and ALL reports scan the unmasked, whole input
("a site that overlaps a masked tract is still a site") -- is what this module runs: the scenario of
tests/cli_combined_model.py (certified by tests/test_cli_combined_cpu.py) through the CLI at W = 8 on both strands, with every
report on the command line, once per flag and once with all of them, on one, two and three ranks.

Each report file is held to the numpy model of that report over the WHOLE FASTA file through the comparer of its own
module, and each comparer is shown to fail against the model of the DUST-masked input and of the training sequences
alone.  The identities that need no model are byte comparisons."""
import functools
import json
import re

import numpy as np
import pytest

import peng_motif_amd as pk
import cli_combined_model as cc
import motif_compare_model as mcm
import motif_dust_model as md
import motif_dyads_model as dy
import motif_enrich_model as men
import motif_erase_model as me
import motif_qvalue_model as mq
import motif_score_model as ms
import test_gpu_motif_centrality as t_cen
import test_gpu_motif_spacing as t_sp
from oracle import oracle as po
from test_gpu_cli_erase import dumped_mask, meta
from test_gpu_motif_dinuc import assert_files_equal_the_model, mafk_model_inputs
from test_gpu_motif_enrich import assert_same_tsv as assert_same_enrich_tsv
from test_gpu_motif_qvalue import cli_model_inputs, drop_q
from test_gpu_motif_refine import assert_refined_file_equals_model
from test_gpu_motif_sites import assert_cli_equals_model
from test_gpu_multirank import run_plain, run_ranks

pytestmark = pytest.mark.gpu

W = 8
SITES_P = 1e-3
REPORT_FILES = ("sites.tsv", "centrality.tsv", "refined.meme", "spacing.tsv", "dinuc.tsv", "dinuc.models", "enrich.tsv", "compare.tsv")
FLAG_FILES = {"mask": ("mask.bed",), "holdout": ("holdout.tsv",), "erase": ("erase.tsv",), "dyads": ("dyads.tsv", "heads.meme")}
# name -> (the flags of the run, its ranks)
CASES = {
    "plain": ((), 1),
    "masked": (("mask",), 1),
    "held": (("holdout",), 1),
    "held_unscored": (("holdout", "unscored"), 1),
    "train": (("train",), 1),
    "erased": (("erase",), 1),
    "dyads": (("dyads",), 1),
    "all": (("mask", "holdout", "erase", "dyads"), 1),
    "all2": (("mask", "holdout", "erase", "dyads"), 2),
    "all3": (("mask", "holdout", "erase", "dyads"), 3),
    "disc": (("control",), 1),
    "disc_all": (("control", "discriminative", "mask", "holdout"), 1),
}


class Run:
    """one CLI run: every rank's (rc, stdout, stderr, MEME, JSON) and the directory its other files are in"""

    def __init__(self, name, d, res):
        self.name, self.d, self.res = name, d, res
        self.flags = CASES[name][0]
        self.rc, self.so, self.se, self.meme, self.js = res[0]
        self.dump = d / "tables"
        self.scores = d / "scores.txt"

    def file(self, name):
        return self.d / name

    def text(self, name):
        return (self.d / name).read_text()

    def patterns(self):
        return json.loads(self.js)["patterns"]


def command(scn, name, d):
    """the command line of a run whose files go to d"""
    flags = CASES[name][0]
    f = lambda x: str(d / x)  # noqa: E731
    if "train" in flags:  # the run of 7p's relation: the training sequences alone, the whole input as the background set
        return [scn["train_fa"], "-w", str(W), "--background-sequences", scn["fa"]]
    args = [scn["fa"], "-w", str(W)]
    if "control" in flags:
        args += ["--background-sequences", scn["bg"]]
    args += [] if "unscored" in flags else ["--score-motifs"]
    args += ["--sites", f("sites.tsv"), "--sites-pvalue", "1e-3", "--sites-qvalue", "--centrality", f("centrality.tsv"),
             "--refine", f("refined.meme"), "--spacing", f("spacing.tsv"), "--dinuc", f("dinuc.tsv"), "--dinuc-models", f("dinuc.models"),
             "--enrich", f("enrich.tsv"), "--enrich-db", scn["db"], "--compare", f("compare.tsv"), "--compare-db", scn["db"]]
    if "discriminative" in flags:
        args += ["--discriminative"]
    if "mask" in flags:
        args += ["--mask-low-complexity", "--mask-report", f("mask.bed")]
    if "holdout" in flags:
        args += ["--holdout", f("holdout.tsv")]
    if "erase" in flags:
        args += ["--erase", f("erase.tsv"), "--max-optimized-patterns", "5"]
    if "dyads" in flags:
        args += ["--dyads", f("dyads.tsv"), "--dyads-motifs", f("heads.meme")]
    return args


def launch(scn, name, d):
    """one CLI process per rank; the tables (PENGK_DUMP_TABLES) and the integer matrices --sites scanned with
    (PENGK_SITES_SCORES) are left beside the run's files"""
    (d / "tables").mkdir()
    env = {"PENGK_DUMP_TABLES": str(d / "tables"), "PENGK_SITES_SCORES": str(d / "scores.txt")}
    world = CASES[name][1]
    args = command(scn, name, d)
    res = [run_plain(args, d, tag="out", extra_env=env)] if world == 1 else run_ranks(args, world, d, tag="out", extra_env=env)
    for rank, r in enumerate(res):
        assert r[0] == 0, (name, rank, r[2].decode()[-2000:])
    return Run(name, d, res)


@pytest.fixture(scope="module")
def scn(tmp_path_factory):
    return build_scenario(tmp_path_factory.mktemp("combined"))


def build_scenario(d):
    """the scenario's files in d -- the input, its DUST-masked codes and its training sequences as FASTA files of their own,
    the control set, the database -- and what the tests know about them"""
    seqs, sites = cc.tracts_behind_the_word(cc.SEED)
    masked, bits, _ = md.mask_codes(seqs, cc.T)
    i0, i1 = cc.split(len(seqs))
    names = cc.names_of(len(seqs))
    control = cc.control()
    db_names, db_rows = cc.database()
    texts = {"input.fa": cc.fasta_text(seqs), "masked.fa": cc.fasta_text(masked),
             "train.fa": cc.fasta_text([seqs[i] for i in i0], [names[i] for i in i0]), "control.fa": cc.fasta_text(control)}
    for k, v in texts.items():
        (d / k).write_text(v)
    mcm.write_meme(d / "db.meme", db_names, db_rows)
    return dict(fa=str(d / "input.fa"), masked_fa=str(d / "masked.fa"), train_fa=str(d / "train.fa"), bg=str(d / "control.fa"),
                db=str(d / "db.meme"), db_names=db_names, db_rows=db_rows, seqs=seqs, sites=sites, masked=masked, bits=bits,
                taken=cc.gone(seqs, masked), i0=i0, i1=i1, control=control)


def _run_fixture(case, name):
    @pytest.fixture(scope="module", name=name)
    def fixture(scn, tmp_path_factory):
        return launch(scn, case, tmp_path_factory.mktemp(case))
    return fixture


# one module-scoped fixture per case, under the case's name (CASES["all"] as all_flags: `all` is a builtin)
FIXTURE_OF = {n: (n if n != "all" else "all_flags") for n in CASES}
for _case, _name in FIXTURE_OF.items():
    globals()[_name] = _run_fixture(_case, _name)


# ---- a. the reports scan the whole input -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model_inputs(fa):
    """(sequences, sampled negatives of --score-motifs at its defaults, V of orders 0..2) of a FASTA file that is its own
    background set: the same for every run, so built once per file"""
    return mafk_model_inputs(fa)


def check_sites(run, fa, scn):
    assert_cli_equals_model(fa, run.js, drop_q(run.text("sites.tsv")), SITES_P, True)


def sites_model_text(run, fa):
    """the --sites --sites-qvalue file of the model, from the integer matrices the run itself scanned with"""
    seqs, names, ids, Ss, bg = cli_model_inputs(fa, run.js, run.scores)
    return mq.render(seqs, names, ids, Ss, bg, SITES_P, True)


def check_qvalues(run, fa, scn):
    text = run.text("sites.tsv")
    same = text == sites_model_text(run, fa)  # (a bool: no diff of two long texts when it fails)
    assert text.count("\n") > 100 and same


def check_centrality(run, fa, scn):
    t_cen.assert_tsv_near_model(run.text("centrality.tsv"), t_cen.model_tsv(fa, run.js, 1e-4, True))


def check_refine(run, fa, scn):
    assert_refined_file_equals_model(fa, run.js, run.text("refined.meme"), True)


def check_spacing(run, fa, scn):
    t_sp.assert_tsv_near_model(run.text("spacing.tsv"), t_sp.model_tsv(fa, run.js, 1e-4, True))


def check_dinuc(run, fa, scn):
    assert_files_equal_the_model(model_inputs(fa), run.js, run.text("dinuc.tsv"), run.text("dinuc.models"), True)


def check_score(run, fa, scn):
    """zoops_score and occur of the JSON against the model, as tests/test_gpu_motif_score.py holds them: from the written
    PWMs, the input's background model and its sampled negatives, to 1e-3"""
    seqs, negs, V = model_inputs(fa)
    pats = run.patterns()
    assert pats
    for p in pats:
        S = ms.log_odds(np.array(p["pwm"], np.float32), V[0])
        lo, hi = ms.score_range(S)
        P = ms.histogram(ms.best_scores(seqs, S, True), lo, hi)
        N = ms.histogram(ms.best_scores(negs, S, True), lo, hi)
        assert abs(ms.auc(P, N) - p["zoops_score"]) < 1e-3, p["iupac_motif"]
        assert abs(ms.occur(P, N) - p["occur"]) < 1e-3, p["iupac_motif"]


@functools.lru_cache(maxsize=None)
def enrich_model_text(fa, db):
    seqs, negs, V = model_inputs(fa)
    names, rows = cc.database()
    res = men.analyse(men.Packed(seqs), men.Packed(negs), rows, V[0], 1e-3, True)
    return men.render(names, [""] * len(names), res)


def check_enrich(run, fa, scn):
    got = run.text("enrich.tsv")
    assert got.count("\n") > 2
    assert_same_enrich_tsv(got, enrich_model_text(fa, scn["db"]))


CHECKS = {"sites": check_sites, "qvalues": check_qvalues, "centrality": check_centrality, "refine": check_refine,
          "spacing": check_spacing, "dinuc": check_dinuc, "score": check_score, "enrich": check_enrich}


@pytest.mark.parametrize("report", list(CHECKS))
@pytest.mark.parametrize("name", ["masked", "held", "erased", "all"])
def test_the_report_is_the_model_of_the_whole_input_and_of_nothing_less(request, scn, tmp_path, name, report):
    """the report file of the run against the model fed the whole FASTA file and the run's own JSON -- and the same comparer
    against the model of (i) the DUST-masked codes, (ii) the training sequences alone and (iii) the codes behind the first
    erase mask, each of which must fail where the run had that transform on: a report that picked up the mask's validity
    words, the training ScanSubset, the overridden sequence count or a later round's validity words would print the lines
    of one of those models"""
    run = request.getfixturevalue(FIXTURE_OF[name])
    check = CHECKS[report]
    check(run, scn["fa"], scn)
    if "mask" in run.flags:
        with pytest.raises(AssertionError):
            check(run, scn["masked_fa"], scn)
    if "holdout" in run.flags:
        with pytest.raises(AssertionError):
            check(run, scn["train_fa"], scn)
    if "erase" in run.flags:  # (iii) what round 2 was searched behind: the sites of round 1's motifs erased as well
        behind = me.mask(scn["masked"] if "mask" in run.flags else scn["seqs"], *dumped_mask(run.dump, 2), True)[0]
        fa = tmp_path / "erased.fa"
        fa.write_text(cc.fasta_text(behind))
        with pytest.raises(AssertionError):
            check(run, str(fa), scn)


@pytest.mark.parametrize("name", ["masked", "held", "all"])
def test_sites_over_masked_bases_and_in_held_out_sequences_are_written(request, scn, name):
    """reach, computed from the model: among the model's --sites lines for the found motifs at least 20 overlap a base the
    mask took and at least 20 lie in held-out sequences, and every one of them is a line of the CLI's file"""
    run = request.getfixturevalue(FIXTURE_OF[name])
    got = set(run.text("sites.tsv").splitlines())
    held_out = set(int(i) for i in scn["i1"])
    over_mask, in_held = [], []
    for line in sites_model_text(run, scn["fa"]).splitlines()[1:]:
        f = line.split("\t")
        i, a, b = int(f[2][1:]), int(f[3]) - 1, int(f[4])
        if scn["taken"][i][a:b].any():
            over_mask.append(line)
        if i in held_out:
            in_held.append(line)
    print("%s: %d model sites overlap a masked base, %d lie in held-out sequences" % (name, len(over_mask), len(in_held)))
    assert len(over_mask) >= 20 and len(in_held) >= 20
    assert all(l in got for l in over_mask) and all(l in got for l in in_held)


# ---- b. exact identities -----------------------------------------------------------------------------------------------------
def test_dyads_change_nothing_but_their_own_line_and_files(plain, dyads):
    assert (dyads.meme, dyads.js) == (plain.meme, plain.js) and plain.meme is not None
    line = [l for l in dyads.so.splitlines(True) if l.startswith(b"dyads (")]
    assert len(line) == 1 and dyads.so.replace(line[0], b"") == plain.so and b"dyads" not in plain.so
    for name in REPORT_FILES:
        assert dyads.file(name).read_bytes() == plain.file(name).read_bytes(), name
    assert dyads.text("dyads.tsv").count("\n") >= 1 and not plain.file("dyads.tsv").exists()


def test_the_enrich_file_depends_on_the_database_the_whole_input_and_the_negatives_only(plain, masked, held, erased, dyads, all_flags,
                                                                                          disc, disc_all):
    want = plain.file("enrich.tsv").read_bytes()
    assert want.count(b"\n") > 2
    for run in (masked, held, erased, dyads, all_flags):
        assert run.file("enrich.tsv").read_bytes() == want, run.name
    assert disc_all.file("enrich.tsv").read_bytes() == disc.file("enrich.tsv").read_bytes()
    assert disc.file("enrich.tsv").read_bytes() != want  # (another background model: other log-odds, other negatives)


def test_the_compare_file_follows_the_meme_file(request):
    runs = [request.getfixturevalue(FIXTURE_OF[n]) for n in CASES if n not in ("train", "all2", "all3")]
    pairs = 0
    for k, a in enumerate(runs):
        assert a.file("compare.tsv").read_bytes().count(b"\n") >= 1
        for b in runs[k + 1:]:
            if a.meme == b.meme:
                pairs += 1
                assert a.file("compare.tsv").read_bytes() == b.file("compare.tsv").read_bytes(), (a.name, b.name)
    assert pairs >= 1  # (plain and dyads at the least)


def test_the_background_model_is_the_whole_background_sets(request, scn):
    V_input = po.bg_V(po.bg_counts(*ms.flatten(scn["seqs"]), 2), 2).tobytes()
    V_control = po.bg_V(po.bg_counts(*ms.flatten(scn["control"]), 2), 2).tobytes()
    assert V_input != V_control
    for n in CASES:
        run = request.getfixturevalue(FIXTURE_OF[n])
        V = np.fromfile(str(run.dump / "V.f32"), np.float32)
        assert V.tobytes() == (V_control if "control" in run.flags else V_input), n
    r2 = request.getfixturevalue("all_flags").dump / "round2" / "V.f32"
    assert np.fromfile(str(r2), np.float32).tobytes() == V_input


# ---- c. the hold-out identity, with reports present --------------------------------------------------------------------------
def test_the_holdout_motifs_are_those_of_the_training_sequences_alone(held, held_unscored, train):
    """7p's relation with every report on the command line.  Byte for byte where --score-motifs is not among them; with it
    the MEME and JSON files hold two more fields per motif and are in another order (and log(Pval) and bg_prob are printed
    with the stream's state at their place, tests/test_gpu_motif_score.py): the same motifs, every other field equal"""
    assert held_unscored.meme is not None and (held_unscored.meme, held_unscored.js) == (train.meme, train.js)
    key = lambda p: (p["iupac_motif"], p["sites"], p["pattern_length"])  # noqa: E731
    want = {key(p): p for p in train.patterns()}
    assert len(want) == len(train.patterns()) >= 1 and sorted(want) == sorted(key(p) for p in held.patterns())
    for p in held.patterns():
        q = {k: v for k, v in p.items() if k not in ("zoops_score", "occur")}
        r = want[key(p)]
        assert list(q) == list(r)
        for f in q:
            if f in ("log(Pval)", "bg_prob"):
                assert abs(q[f] - r[f]) <= 1e-5 * abs(r[f]) + 1e-6, (f, q[f], r[f])
            else:
                assert q[f] == r[f], f
    # the reports do not depend on --score-motifs beyond the motifs' order: the same set of lines
    assert sorted(drop_motif_index(held.text("sites.tsv"))) == sorted(drop_motif_index(held_unscored.text("sites.tsv")))
    assert held.file("holdout.tsv").read_text().split("\n")[0] == held_unscored.file("holdout.tsv").read_text().split("\n")[0]


def drop_motif_index(text):
    return [l.split("\t", 1)[1] for l in text.splitlines()[1:]]


# ---- d. later erase rounds under mask + holdout --------------------------------------------------------------------------------
def test_the_erase_rounds_mask_and_count_the_training_share_behind_the_mask(scn, all_flags):
    """Round 1 counts the training share behind the low-complexity mask; round 2 counts what the erase mask, made from the
    dumped matrices, leaves of exactly that; the report's site counts are the training share's (7p).

    erase_valid.u32 spans the whole input's validity words.  The words of the TRAINING sequences are the model's; the words
    of the HELD-OUT sequences are zero: run_erase_rounds clears both of its buffers before the first mask, because
    pengk_mask_sites writes only the words of the pair of offs / lens it is given.  They are not whatever the buffer held
    before, and not the sequences' own validity either: a held-out sequence is not searched in any round."""
    run, dump = all_flags, all_flags.dump
    seqs, i0, i1 = scn["seqs"], scn["i0"], scn["i1"]
    train = set(int(i) for i in i0)
    once = [scn["masked"][i] for i in i0]
    counts, ltot = po.count(*ms.flatten(once), W, True)
    m1, m2 = meta(dump / "meta.txt"), meta(dump / "round2" / "meta.txt")
    assert int(m1["ltot"]) == ltot and int(m1["N"]) == len(i0)
    assert np.array_equal(np.fromfile(str(dump / "counts.u32"), np.uint32).astype(np.uint64), counts)
    assert b"erase round 2:" in run.so and b"erase round 1: the input behind the low-complexity mask\n" in run.so
    # round 2
    Ss, thr = dumped_mask(dump, 2)
    twice, n2, erased = me.mask(once, Ss, thr, True)
    assert erased > 0 and ("erase round 2: %d bases" % erased).encode() in run.so
    it = iter(twice)
    whole = [next(it) if i in train else np.zeros(len(c), np.uint8) for i, c in enumerate(seqs)]
    want = me.valid_words(whole)
    got = np.fromfile(str(dump / "round2" / "erase_valid.u32"), np.uint32)
    words = np.cumsum([0] + [(len(c) + 31) // 32 for c in seqs])
    for i in (int(i1[0]), int(i1[-1])):
        assert not want[words[i]:words[i + 1]].any() and me.valid_words([seqs[i]]).any()
    assert len(got) >= len(want) and np.array_equal(got[:len(want)], want)
    counts2, ltot2 = po.count(*ms.flatten(twice), W, True)
    assert int(m2["ltot"]) == ltot2 and int(m2["N"]) == len(i0)
    assert np.array_equal(np.fromfile(str(dump / "round2" / "counts.u32"), np.uint32).astype(np.uint64), counts2)
    # the report: the sites of every round's motifs on what that round searched -- of the training share
    Ss3, thr3 = dumped_mask(dump, 3)
    n3 = me.mask(twice, Ss3, thr3, True)[1]
    lines = [l.split("\t") for l in run.text("erase.tsv").splitlines()[1:]]
    ids = [[l[1] for l in lines if l[0] == str(r)] for r in (1, 2)]
    assert len(ids[0]) == len(Ss) and len(ids[1]) == len(Ss3) and len(lines) == len(Ss) + len(Ss3)
    seeds = [int(next(l[5] for l in lines if l[0] == str(r))) for r in (1, 2)]
    rounds = [dict(seeds=seeds[0], windows=ltot, bases_erased=0, motifs=[(i, len(S), t, int(n)) for i, S, t, n in zip(ids[0], Ss, thr, n2)]),
              dict(seeds=seeds[1], windows=ltot2, bases_erased=erased,
                   motifs=[(i, len(S), t, int(n)) for i, S, t, n in zip(ids[1], Ss3, thr3, n3)])]
    assert run.text("erase.tsv") == me.render_report(rounds)
    # ... and not the whole input's, behind the mask or as it is: the hold-out share has sites of its own
    for other in (scn["masked"], seqs):
        assert me.mask(other, Ss, thr, True)[1].tolist() != n2.tolist()
    assert sorted(ids[0] + ids[1]) == sorted(p["iupac_motif"] for p in run.patterns())


# ---- e. dyads count what round 1 counts ----------------------------------------------------------------------------------------
def test_the_dyads_are_those_of_the_training_share_behind_the_mask(scn, all_flags):
    tsv = all_flags.text("dyads.tsv")
    once = [scn["masked"][i] for i in scn["i0"]]
    counts, mono = dy.tables(once, 20, True)
    assert tsv == dy.render_tsv(pk.dyad_summary(counts, mono, True))
    assert tsv == dy.render_tsv(dy.summary(counts, mono, True, pk.binomial_log10_sf))
    for other in (scn["seqs"], scn["masked"], [scn["seqs"][i] for i in scn["i0"]]):  # neither flag alone, nor neither
        assert tsv != dy.render_tsv(pk.dyad_summary(*dy.tables(other, 20, True), True))


# ---- f. ranks --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["all2", "all3"])
def test_ranks_write_what_one_process_writes(request, all_flags, name):
    many = request.getfixturevalue(name)
    assert (many.so, many.meme, many.js) == (all_flags.so, all_flags.meme, all_flags.js) and all_flags.meme is not None
    for rank in range(1, len(many.res)):
        assert many.res[rank][1] == b"", rank
    for name_ in REPORT_FILES + sum((FLAG_FILES[f] for f in many.flags), ()):
        assert many.file(name_).read_bytes() == all_flags.file(name_).read_bytes(), name_
    for name_ in ("counts.u32", "meta.txt", "round2/counts.u32", "round2/meta.txt", "round2/erase_thr.i32", "holdout_thr.i32", "mask_counts.u64"):
        assert (many.dump / name_).read_bytes() == (all_flags.dump / name_).read_bytes(), name_
    assert re.search(rb"holdout \(fraction 0\.1, seed 1\): \d+ of 2000 input sequences set aside", many.so)
