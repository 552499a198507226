"""The scenarios of tests/test_gpu_cli_control_modes.py, from the models alone (tests/motif_match_model.py): what every
match mode keeps of mode_scenario(1), and that the set still holds what the device tests are for -- negatives both larger
and smaller than the input, a shortfall and none, one stratum with one GC bin, the first and the last length bin in every
report by length and 1 .. inf in every other -- and a control whose matching sequences all lie in the first quarter of its
file.  No device compute here."""
import numpy as np
import pytest

import motif_match_model as mm
from test_gpu_cli_control import write_fasta

# mode: (strata in use, kept, control, input, shortfall, report lines)
FIGURES = {
    "default": (14, 1485, 6012, 2018, 533, 24),
    "gc4_r3": (3, 3023, 6012, 2018, 3031, 4),
    "length_r2": (5, 3038, 6012, 2018, 998, 6),
    "both16_r3": (15, 1502, 6012, 2018, 4552, 29),
    "gc1": (1, 2018, 6012, 2018, 0, 1),
}


@pytest.fixture(scope="module")
def matches():
    pos, ctrl = mm.mode_scenario(1)
    out = {}
    for name, _, gc, length, G, ratio in mm.MODES:
        m = mm.match(pos, ctrl, gc, length, G, ratio)
        m["rows"] = [l.split("\t") for l in mm.report(m["h_in"], m["h_ctrl"], m["quota"], m["G"], length).splitlines()[1:]]
        m["n_in"], m["n_ctrl"] = len(pos), len(ctrl)
        out[name] = m
    return out


def test_the_modes_are_the_flags_they_say():
    assert [m[0] for m in mm.MODES] == list(FIGURES)
    for name, flags, gc, length, G, ratio in mm.MODES:
        f = dict(zip(flags[0::2], flags[1::2]))
        assert len(flags) == 2 * len(f)
        assert {"gc,length": (True, True), "gc": (True, False), "length": (False, True)}[f.get("--control-match", "gc,length")] == (gc, length)
        assert int(f.get("--control-ratio", 1)) == ratio
        assert (int(f.get("--control-match-gc-bins", 10)) if gc else 1) == G  # (without GC matching: one bin)


def test_the_edge_sequences_are_behind_the_scenario():
    pos, ctrl = mm.mode_scenario(1)
    pos0, ctrl0 = mm.scenario(1)
    assert all(np.array_equal(a, b) for a, b in zip(pos, pos0)) and all(np.array_equal(a, b) for a, b in zip(ctrl, ctrl0))
    assert [len(c) for c in pos[len(pos0):]] == [L for L in mm.EDGE_LENGTHS for _ in range(3)]
    assert [len(c) for c in ctrl[len(ctrl0):]] == [L for L in mm.EDGE_LENGTHS for _ in range(2)]
    assert [mm.length_bin(L) for L in mm.EDGE_LENGTHS] == [0, 0, 1, 14, 15, 15]


@pytest.mark.parametrize("name", list(FIGURES))
def test_the_figures_of_every_mode(matches, name):
    m = matches[name]
    got = (m["in_use"], len(m["kept"]), m["n_ctrl"], m["n_in"], m["short"], len(m["rows"]))
    print(name, got)
    assert got == FIGURES[name]
    assert sum(int(r[6]) for r in m["rows"]) == len(m["kept"]) and sum(int(r[4]) for r in m["rows"]) == m["n_in"]
    assert m["ratio"] * m["n_in"] - len(m["kept"]) == m["short"]


def test_the_scenario_keeps_its_point(matches):
    kept = {k: len(m["kept"]) for k, m in matches.items()}
    n_in = matches["default"]["n_in"]
    assert any(k > n_in for k in kept.values()) and any(k < n_in for k in kept.values())
    assert any(m["short"] == 0 for m in matches.values()) and any(m["short"] > 0 for m in matches.values())
    assert sum(1 for m in matches.values() if m["in_use"] == 1 and m["G"] == 1) == 1
    for name, m in matches.items():
        ends = [(r[0], r[1]) for r in m["rows"]]
        if m["use_length"]:
            assert any(lo == "1" and hi != "inf" for lo, hi in ends) and any(hi == "inf" and lo != "1" for lo, hi in ends), name
        else:
            assert set(ends) == {("1", "inf")}, name
        if m["G"] not in (1, 10):  # GC bounds that are no multiples of a tenth
            assert any(r[2] not in ("%.3f" % (k / 10) for k in range(10)) for r in m["rows"]), name
    # the singular forms of the line on stdout
    assert mm.stdout_line("gc", matches["gc1"], 6012) == ("control negatives: matched by gc (1 GC bin, ratio 1): 1 stratum in use, "
                                                          "kept 2018 of 6012 control sequences, shortfall 0")
    assert "(10 GC bins, ratio 1): 14 strata in use" in mm.stdout_line("gc,length", matches["default"], 6012)


def test_the_front_loaded_control_ends_in_the_first_quarter_of_its_file(tmp_path):
    pos, ctrl = mm.scenario(1)
    m = mm.match(pos, ctrl)
    front, n = mm.front_loaded(ctrl, m["h_in"])
    assert n == 1510 and len(front) == len(ctrl)
    # the same sequences, the same match: only the order differs
    assert sorted(c.tobytes() for c in front) == sorted(c.tobytes() for c in ctrl)
    m2 = mm.match(pos, front)
    assert np.array_equal(m2["h_ctrl"], m["h_ctrl"]) and np.array_equal(m2["quota"], m["quota"])
    assert len(m2["kept"]) == len(m["kept"]) and int(m2["kept"].max()) < n
    # as test_gpu_cli_control.py writes it: three ranks cut it into thirds at record starts
    whole, head = tmp_path / "front.fa", tmp_path / "head.fa"
    write_fasta(str(whole), front, b"ctl")
    write_fasta(str(head), front[:n], b"ctl")
    size, end = whole.stat().st_size, head.stat().st_size
    print(n, end, size)
    assert (end, size) == (164990, 1253690) and 4 * end < size
    assert whole.read_bytes()[:end] == head.read_bytes()
