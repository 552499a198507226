"""peng_motif --score-negatives control beyond the one configuration of tests/test_gpu_cli_control.py: every match mode of
tests/motif_match_model.py (MODES, on mode_scenario(1): negatives larger and smaller than the input, one GC bin, no length
matching, the first and the last length bin) against the models; --dinuc as a consumer of the control, alone and beside
--score-motifs and --enrich; two and three ranks, ranks that keep nothing and ranks that hold no control sequence at
all, against one process; and the control beside --discriminative and --erase.  tests/test_control_modes_cpu.py holds the
scenarios to their point on the CPU."""
import json

import numpy as np
import pytest

import motif_compare_model as mc
import motif_enrich_model as me
import motif_match_model as mm
import motif_score_model as ms
from oracle import oracle as po
from test_gpu_cli_control import NAMES, WORDS, check_scores, write_fasta
from test_gpu_motif_dinuc import assert_files_equal_the_model
from test_gpu_motif_enrich import assert_same_tsv
from test_gpu_multirank import run_plain, run_ranks

pytestmark = pytest.mark.gpu

MODE = {m[0]: m for m in mm.MODES}
MATCH_NAME = {(True, True): "gc,length", (True, False): "gc", (False, True): "length"}
DUMPS = ("match_input", "match_control", "match_quota", "match_kept")
CAP = ["--max-optimized-patterns", "5"]  # (the --dinuc model runs once per motif and ambiguous log-odds entry)


def background(ctrl):
    """the background model of the control file (order 2, the CLI's default): V of orders 0, 1, 2"""
    codes, offs = ms.flatten(ctrl)
    Vc = np.asarray(po.bg_V(po.bg_counts(codes, offs, 2), 2), np.float32)
    return [Vc[0:4], Vc[4:20], Vc[20:84]]


def fasta_pair(d, pos, ctrl):
    fa, cfa = str(d / "input.fa"), str(d / "control.fa")
    write_fasta(fa, pos, b"in")
    write_fasta(cfa, ctrl, b"ctl")
    return [fa, "-w", "8", "--background-sequences", cfa, "--score-negatives", "control"]


def consumers(d, tag, db, score=True, enrich=True, dinuc=False, report=True):
    """the flags of the consumers of the negatives, their files named d / tag.*"""
    out = ["--control-match-report", str(d / (tag + ".match.tsv"))] if report else []
    if score:
        out += ["--score-motifs"]
    if enrich:
        out += ["--enrich", str(d / (tag + ".enrich.tsv")), "--enrich-db", db]
    if dinuc:
        out += ["--dinuc", str(d / (tag + ".dinuc.tsv")), "--dinuc-models", str(d / (tag + ".dinuc.models"))]
    return out


def files(d, tag, kinds=("match.tsv", "enrich.tsv", "dinuc.tsv", "dinuc.models")):
    return {k: (d / (tag + "." + k)).read_bytes() if (d / (tag + "." + k)).exists() else None for k in kinds}


def dumped(dump):
    return {name: (dump / (name + ".u64")).read_bytes() for name in DUMPS}


def run_ok(args, d, tag, dump=None):
    """run_plain of a run that must end well (a fixture goes no further after one that did not)"""
    r = run_plain(args, d, tag=tag, extra_env={"PENGK_DUMP_TABLES": str(dump)} if dump else None)
    assert r[0] == 0, (tag, r[0], r[2].decode()[-2000:])
    return r


def control_line(so):
    line = [l for l in so.decode().splitlines() if l.startswith("control negatives:")]
    assert len(line) == 1, so.decode()[-2000:]
    return line[0]


def model_of(pos, ctrl, name):
    _, _, gc, length, G, ratio = MODE[name]
    m = mm.match(pos, ctrl, gc, length, G, ratio)
    m["negs"] = [ctrl[i] for i in m["kept"]]
    m["line"] = mm.stdout_line(MATCH_NAME[(gc, length)], m, len(ctrl))
    m["report"] = mm.report(m["h_in"], m["h_ctrl"], m["quota"], m["G"], length)
    return m


def assert_match_equals_the_model(m, dump, report, so):
    """the dumped counts, quotas and kept indices, the report and the line on stdout"""
    for name, want in zip(DUMPS, (m["h_in"], m["h_ctrl"], m["quota"], m["kept"].astype(np.uint64))):
        assert np.array_equal(np.fromfile(str(dump / (name + ".u64")), np.uint64), want), name
    assert report.decode() == m["report"]
    assert control_line(so) == m["line"]


def assert_scores_and_enrichment(js, enrich_tsv, pos, negs, rows, bg0):
    check_scores(js, pos, negs, bg0)
    res = me.analyse(me.Packed(pos), me.Packed(negs), rows, bg0, 1e-3, True)
    assert_same_tsv(enrich_tsv.decode(), me.render(NAMES, [""] * 3, res))
    scored = {int(l.split("\t")[9]) for l in enrich_tsv.decode().splitlines()[1:]}  # neg_scored
    assert scored == {len(negs)}


def assert_ranks_equal_one_process(res, one, d, tag, one_tag, kinds):
    """every rank ends as the one process did; rank 0 wrote its stdout, MEME and JSON, the others nothing on stdout; the
    files named by the flags hold the same bytes"""
    rc, so, se, meme, js = one
    assert [r[0] for r in res] == [rc] * len(res), [r[2].decode()[-1000:] for r in res]
    assert (res[0][1], res[0][3], res[0][4]) == (so, meme, js)
    assert all(r[1] == b"" for r in res[1:])
    assert files(d, tag, kinds) == files(d, one_tag, kinds)


# ---- the scenarios -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def db(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("db") / "db.meme")
    rows = [mm.word_pwm(w) for w in WORDS]
    mc.write_meme(path, NAMES, rows)
    return path, rows


@pytest.fixture(scope="module")
def edges(tmp_path_factory):
    """mode_scenario(1): the scenario with the sequences at the length bins' edges"""
    d = tmp_path_factory.mktemp("edges")
    pos, ctrl = mm.mode_scenario(1)
    return dict(dir=d, pos=pos, ctrl=ctrl, V=background(ctrl), args=fasta_pair(d, pos, ctrl))


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    """scenario(1), as tests/test_gpu_cli_control.py runs it"""
    d = tmp_path_factory.mktemp("plain")
    pos, ctrl = mm.scenario(1)
    return dict(dir=d, pos=pos, ctrl=ctrl, V=background(ctrl), args=fasta_pair(d, pos, ctrl))


# ---- every mode equals the models ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mode_runs(edges, db):
    out = {}
    for name, flags, *_ in mm.MODES:
        dump = edges["dir"] / ("tables_" + name)
        dump.mkdir()
        out[name] = (dump, run_ok(edges["args"] + flags + consumers(edges["dir"], name, db[0]), edges["dir"], name, dump))
    return out


@pytest.mark.parametrize("name", list(MODE))
def test_every_mode_equals_the_models(edges, db, mode_runs, name):
    dump, (rc, so, se, meme, js) = mode_runs[name]
    assert rc == 0, se.decode()[-2000:]
    m = model_of(edges["pos"], edges["ctrl"], name)
    print(name, m["line"])
    f = files(edges["dir"], name)
    assert_match_equals_the_model(m, dump, f["match.tsv"], so)
    assert_scores_and_enrichment(js, f["enrich.tsv"], edges["pos"], m["negs"], db[1], edges["V"][0])


def test_the_modes_differ_where_they_should(edges, mode_runs):
    """the singular forms, and negatives on both sides of the input's size (the conditions of the scenario, seen on stdout)"""
    lines = {name: control_line(r[1]) for name, (_, r) in mode_runs.items()}
    assert "(1 GC bin, ratio 1): 1 stratum in use, kept 2018 of 6012" in lines["gc1"]
    assert "(1 GC bin, ratio 2)" in lines["length_r2"] and "(16 GC bins, ratio 3)" in lines["both16_r3"]
    kept = {name: int(l.split("kept ")[1].split()[0]) for name, l in lines.items()}
    assert kept["default"] < len(edges["pos"]) < kept["gc4_r3"]
    assert len({r[4] for _, r in mode_runs.values()}) > 1  # (the scores are not those of one set of negatives)


# ---- --dinuc consumes the control ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dinuc_runs(plain, db):
    """default (fewer negatives than the input) and gc4_r3 (more): --dinuc alone, beside --score-motifs and --enrich,
    those two without it, and --dinuc beside --enrich only; and the run that builds no negatives at all"""
    d = plain["dir"]
    out = {}
    for name in ("default", "gc4_r3"):
        flags = MODE[name][1] + CAP
        for tag, kw in (("alone", dict(score=False, enrich=False, dinuc=True)), ("all", dict(dinuc=True)), ("two", dict()),
                        ("enrich", dict(score=False, dinuc=True))):
            dump = d / ("tables_%s_%s" % (name, tag))
            dump.mkdir()
            out[name, tag] = (dump, run_ok(plain["args"] + flags + consumers(d, name + "_" + tag, db[0], **kw), d, name + "_" + tag, dump))
    out["none"] = (None, run_ok(plain["args"] + CAP, d, "none"))
    return out


@pytest.mark.parametrize("tag", ["alone", "all"])
@pytest.mark.parametrize("name", ["default", "gc4_r3"])
def test_dinuc_scores_against_the_kept_control(plain, db, dinuc_runs, name, tag):
    dump, (rc, so, se, meme, js) = dinuc_runs[name, tag]
    assert rc == 0, se.decode()[-2000:]
    m = model_of(plain["pos"], plain["ctrl"], name)
    f = files(plain["dir"], name + "_" + tag)
    assert_match_equals_the_model(m, dump, f["match.tsv"], so)
    assert (len(m["negs"]) > len(plain["pos"])) == (name == "gc4_r3") and len(m["negs"]) != len(plain["pos"])
    mixed = len({len(c) for c in m["negs"]}) > 1  # (100 and 300 bp: the model's per-sequence path)
    assert mixed == (name == "gc4_r3")
    assert json.loads(js)["patterns"]
    assert_files_equal_the_model((plain["pos"], m["negs"], plain["V"]), js, f["dinuc.tsv"].decode(), f["dinuc.models"].decode(), True,
                                 batch=not mixed)
    if tag == "all":
        assert_scores_and_enrichment(js, f["enrich.tsv"], plain["pos"], m["negs"], db[1], plain["V"][0])
    else:
        assert f["enrich.tsv"] is None and "zoops_score" not in json.loads(js)["patterns"][0]


@pytest.mark.parametrize("name", ["default", "gc4_r3"])
def test_dinuc_leaves_everything_else_alone(plain, dinuc_runs, name):
    d = plain["dir"]
    alone, both, two, none = (dinuc_runs[k][1] for k in ((name, "alone"), (name, "all"), (name, "two"), "none"))
    assert [r[0] for r in (alone, both, two, none)] == [0] * 4
    # beside the other two: their outputs are those of the run without --dinuc
    assert both[1:2] + both[3:] == two[1:2] + two[3:]
    assert files(d, name + "_all", ("match.tsv", "enrich.tsv")) == files(d, name + "_two", ("match.tsv", "enrich.tsv"))
    assert dumped(dinuc_runs[name, "all"][0]) == dumped(dinuc_runs[name, "two"][0]) == dumped(dinuc_runs[name, "alone"][0])
    # alone: the run without --dinuc builds no negatives, so its stdout lacks their line and nothing else
    line = control_line(alone[1]).encode() + b"\n"
    assert b"control negatives" not in none[1] and alone[1].replace(line, b"") == none[1]
    assert alone[3:] == none[3:]
    assert files(d, name + "_alone", ("match.tsv",)) == files(d, name + "_two", ("match.tsv",))
    # the first-order models do not depend on who else reads the negatives.  --score-motifs re-ranks the motifs, and a
    # motif's index keys the choice among its equally good sites (tests/motif_centrality_model.py, best_sites): a motif
    # that keeps its index keeps its line and its block byte for byte, every other one what no such choice touches
    got, want = files(d, name + "_all", ("dinuc.tsv", "dinuc.models")), files(d, name + "_alone", ("dinuc.tsv", "dinuc.models"))
    assert files(d, name + "_enrich", ("dinuc.tsv", "dinuc.models")) == want  # (beside --enrich alone nothing is re-ranked)
    assert dinuc_runs[name, "enrich"][1][3:] == alone[3:]
    assert files(d, name + "_enrich", ("enrich.tsv",)) == files(d, name + "_two", ("enrich.tsv",))
    pwms = [[json.dumps(p["pwm"]) for p in json.loads(r[4])["patterns"]] for r in (both, alone)]
    assert sorted(pwms[0]) == sorted(pwms[1]) and len(set(pwms[0])) == len(pwms[0]) > 1
    if pwms[0] == pwms[1]:
        assert got == want
    rows = [f["dinuc.tsv"].splitlines(True) for f in (got, want)]
    blocks = [f["dinuc.models"].split(b"MOTIF ") for f in (got, want)]
    assert rows[0][0] == rows[1][0] and blocks[0][0] == blocks[1][0] and len(rows[0]) == len(blocks[0]) == 1 + len(pwms[0])
    same = 0
    for i, pwm in enumerate(pwms[0]):
        j = pwms[1].index(pwm)
        a, b = rows[0][1 + i].split(b"\t"), rows[1][1 + j].split(b"\t")
        assert (a[0], a[2:5]) == (b[0], b[2:5]) and (int(a[1]), int(b[1])) == (i + 1, j + 1)  # motif | width, flank, sites
        assert blocks[0][1 + i].split(b"\n")[0] == blocks[1][1 + j].split(b"\n")[0]
        if i == j:
            assert rows[0][1 + i] == rows[1][1 + j] and blocks[0][1 + i] == blocks[1][1 + j]
            same += 1
    print(name, "motifs at the same index in both runs:", same, "of", len(pwms[0]))


# ---- ranks ---------------------------------------------------------------------------------------------------------------------
ALL_KINDS = ("match.tsv", "enrich.tsv", "dinuc.tsv", "dinuc.models")


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_write_what_one_process_writes(plain, db, dinuc_runs, world):
    """gc4_r3 with all three consumers: more negatives than input sequences on every rank, and the ranks before a shard
    counted over more than one earlier rank"""
    d = plain["dir"]
    tag = "ranks%d" % world
    res = run_ranks(plain["args"] + MODE["gc4_r3"][1] + CAP + consumers(d, tag, db[0], dinuc=True), world, d, tag=tag)
    assert_ranks_equal_one_process(res, dinuc_runs["gc4_r3", "all"][1], d, tag, "gc4_r3_all", ALL_KINDS)


def test_ranks_that_keep_nothing(plain, db, tmp_path):
    """the control with every sequence of a stratum the input uses in the first quarter of the file: of three ranks the
    second and the third select nothing and scan no negative"""
    m = model_of(plain["pos"], plain["ctrl"], "default")
    front, n = mm.front_loaded(plain["ctrl"], m["h_in"])
    cfa = tmp_path / "front.fa"
    write_fasta(str(cfa), front, b"ctl")
    head = tmp_path / "head.fa"
    write_fasta(str(head), front[:n], b"ctl")
    assert 4 * head.stat().st_size < cfa.stat().st_size  # (three ranks cut the file into thirds, at record starts)
    args = [plain["args"][0], "-w", "8", "--background-sequences", str(cfa), "--score-negatives", "control"] + CAP
    dump = tmp_path / "tables"
    dump.mkdir()
    one = run_ok(args + consumers(tmp_path, "one", db[0], dinuc=True), tmp_path, "one", dump)
    mf = model_of(plain["pos"], front, "default")
    assert int(mf["kept"].max()) < n and len(mf["kept"]) == len(m["kept"])
    assert_match_equals_the_model(mf, dump, files(tmp_path, "one")["match.tsv"], one[1])
    res = run_ranks(args + consumers(tmp_path, "many", db[0], dinuc=True), 3, tmp_path, tag="many")
    assert_ranks_equal_one_process(res, one, tmp_path, "many", "one", ALL_KINDS)


def test_ranks_without_a_control_sequence(plain, db, tmp_path):
    """a control of two sequences, both of a stratum of the input, read by three ranks: at least one of them holds none"""
    m = model_of(plain["pos"], plain["ctrl"], "default")
    two = [plain["ctrl"][i] for i in m["kept"][:2]]
    cfa = tmp_path / "two.fa"
    write_fasta(str(cfa), two, b"ctl")
    args = [plain["args"][0], "-w", "8", "--background-sequences", str(cfa), "--score-negatives", "control"] + CAP
    dump = tmp_path / "tables"
    dump.mkdir()
    one = run_ok(args + consumers(tmp_path, "one", db[0], dinuc=True), tmp_path, "one", dump)
    mt = model_of(plain["pos"], two, "default")
    assert len(mt["kept"]) == 2
    assert_match_equals_the_model(mt, dump, files(tmp_path, "one")["match.tsv"], one[1])
    res = run_ranks(args + consumers(tmp_path, "many", db[0], dinuc=True), 3, tmp_path, tag="many")
    assert_ranks_equal_one_process(res, one, tmp_path, "many", "one", ALL_KINDS)


# ---- beside the other users of the control file and of the scan layout ---------------------------------------------------------
@pytest.mark.parametrize("which", ["discriminative", "erase"])
def test_the_control_beside(plain, db, dinuc_runs, tmp_path, which):
    """--discriminative reads the same file for its counts; --erase extends the motif list before it is scored.  The scores
    and the enrichment follow from the PWMs the JSON holds; the match depends on the sequences only."""
    dump = tmp_path / "tables"
    dump.mkdir()
    if which == "discriminative":
        extra = ["--discriminative"] + consumers(tmp_path, "x", db[0], enrich=False)
    else:
        extra = ["--erase", str(tmp_path / "erase.tsv")] + consumers(tmp_path, "x", db[0])
    rc, so, se, meme, js = run_plain(plain["args"] + CAP + extra, tmp_path, tag="x", extra_env={"PENGK_DUMP_TABLES": str(dump)})
    assert rc == 0, se.decode()[-2000:]
    m = model_of(plain["pos"], plain["ctrl"], "default")
    f = files(tmp_path, "x")
    assert_match_equals_the_model(m, dump, f["match.tsv"], so)
    ref_dump, ref = dinuc_runs["default", "two"]
    assert ref[0] == 0
    assert dumped(dump) == dumped(ref_dump) and f["match.tsv"] == files(plain["dir"], "default_two")["match.tsv"]
    if which == "discriminative":
        check_scores(js, plain["pos"], m["negs"], plain["V"][0])
        assert b"discriminative mode: k-mer enrichment is held to the control set's counts" in so
    else:
        assert_scores_and_enrichment(js, f["enrich.tsv"], plain["pos"], m["negs"], db[1], plain["V"][0])
        assert (tmp_path / "erase.tsv").exists() and b"erase round" in so
