"""Certifies the scenario of tests/cli_combined_model.py without a GPU: the conditions tests/test_gpu_cli_combined.py relies on
when it tells a report that scanned the whole input from one that scanned the masked input or the training share.  They
are conditions, not measurements: a seed that misses one is replaced, the bar stays."""
import numpy as np
import pytest

import cli_combined_model as cc
import motif_dust_model as md
import motif_score_model as ms


@pytest.fixture(scope="module")
def scenario():
    seqs, sites = cc.tracts_behind_the_word(cc.SEED)
    masked, bits, touched = md.mask_codes(seqs, cc.T)
    return dict(seqs=seqs, sites=sites, masked=masked, bits=bits, touched=touched)


def test_the_planted_words_are_where_the_list_says(scenario):
    seqs, sites = scenario["seqs"], scenario["sites"]
    assert len(seqs) == 2000 and all(len(c) == 100 for c in seqs)
    assert 500 <= len(sites) <= 700 and len({i for i, _ in sites}) == len(sites)  # about 30 %, one word per sequence
    w = md.codes_of(cc.WORD)
    kept = np.array([(seqs[i][q:q + len(w)] == w).sum() for i, q in sites])
    assert (kept >= 0).all() and 0.8 < kept.mean() / len(w) < 0.9  # every letter kept with probability 0.85


def test_the_mask_reaches_into_planted_sites(scenario):
    taken = cc.gone(scenario["seqs"], scenario["masked"])
    hit = cc.sites_with_a_masked_base(scenario["sites"], taken)
    print("%d planted sites, %d with a masked base (%.2f on average), %d bases masked in %d sequences" % (
        len(scenario["sites"]), len(hit), np.mean([k for _, _, k in hit]), scenario["bits"], scenario["touched"]))
    assert len(hit) >= 50
    assert scenario["bits"] > 2000
    assert scenario["bits"] == int(sum(t.sum() for t in taken))


def test_planted_sites_lie_in_held_out_sequences(scenario):
    i0, i1 = cc.split(len(scenario["seqs"]))
    held = cc.sites_in(scenario["sites"], i1)
    print("%d of %d sequences held out, %d planted sites among them" % (len(i1), len(scenario["seqs"]), len(held)))
    assert len(i0) + len(i1) == len(scenario["seqs"]) and 100 < len(i1) < 300
    assert len(held) >= 30
    # and some of the sites the mask reaches are in the training share, some are not: the two transforms do not coincide
    hit = cc.sites_with_a_masked_base(scenario["sites"], cc.gone(scenario["seqs"], scenario["masked"]))
    assert cc.sites_in(hit, i0) and cc.sites_in(hit, i1)


def test_the_fasta_text_round_trips(scenario, tmp_path):
    seqs, masked = scenario["seqs"], scenario["masked"]
    i0, _ = cc.split(len(seqs))
    names = cc.names_of(len(seqs))
    for tag, s, nm in (("whole", seqs, None), ("masked", masked, None), ("train", [seqs[i] for i in i0], [names[i] for i in i0])):
        fa = tmp_path / (tag + ".fa")
        fa.write_text(cc.fasta_text(s, nm))
        back = ms.read_fasta_codes(str(fa))
        assert len(back) == len(s) and all(np.array_equal(a, b) for a, b in zip(back, s)), tag
    assert cc.fasta_text(seqs) == md.fasta_text(seqs)


def test_the_control_set_and_the_database():
    ctl = cc.control()
    assert len(ctl) == 2000 and md.mask_codes(ctl, cc.T)[1] > 2000  # (its tracts are masked by the same rule)
    names, rows = cc.database()
    assert len(names) == len(rows) == 25 and "MARE" in names
    assert all(r.shape[1] == 4 and np.all(r > 0) for r in rows)
