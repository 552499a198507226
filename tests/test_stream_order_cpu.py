"""The inputs of tests/test_gpu_stream_order.py, certified on the CPU: a call that ran ahead of the gate read POISON, so for
every output the GPU test compares, the model's value on the poison must differ from its value on the real input -- in a
table, in a sizeable share of the entries that either holds -- or reading poison could pass by accident.  The few outputs
that cannot differ (they follow from the sizes, which the poison shares by construction) are named here; they are covered
by the other half of the gate: the production overwrites every output buffer, so what was written early is gone.

Also the lanes arithmetic that chain (a) relies on, restated: 16 PWMs give the serial EM two lanes under em_overlap = 2.
"""
import os
import re

import numpy as np
import pytest

import stream_gate as sg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# these follow from the sizes alone: the visited windows (the run structure is shared), the iteration count (fixed by
# max_iterations at threshold 0) and the synthetic set (a generator without a device input)
SAME_BY_CONSTRUCTION = {"ltot", "state", "synth_words", "synth_valid", "synth_offs", "synth_lens"}
TABLE_ENTRIES = 256  # from this size on an output counts as a table
# Real input and poison are independent draws, so an entry that either holds differs unless two independent values
# collide: small counts collide often (two Poisson(0.2) bins of the W = 10 table are both 1 in one of six bins that
# hold anything), float entries practically never.  A quarter of the support is far above what a read of poison could
# leave intact and below what the sparsest table here shows.
MIN_SHARE = 0.25


def differing(real, poison):
    """(entries that differ, entries that either array holds: not all bits zero), floats by their bits"""
    r, p = np.asarray(real).reshape(-1), np.asarray(poison).reshape(-1)
    assert r.shape == p.shape and r.dtype == p.dtype
    if r.dtype.kind == "f":
        r, p = r.view(np.uint32), p.view(np.uint32)
    return int((r != p).sum()), int(((r != 0) | (p != 0)).sum())


def certify(real, poison):
    assert real.keys() == poison.keys()
    for name in real:
        d, held = differing(real[name], poison[name])
        if name in SAME_BY_CONSTRUCTION:
            assert d == 0, name  # (if this ever differs, it moves to the certified ones)
            continue
        assert d > 0, "%s: the poison gives the real value" % name
        if np.asarray(real[name]).size >= TABLE_ENTRIES:
            assert d >= MIN_SHARE * held, "%s: only %d of %d held entries differ under poison" % (name, d, held)


@pytest.mark.parametrize("whole", [False, True], ids=["invalid_bases", "whole"])
@pytest.mark.parametrize("W,both", sg.A_CONFIGS)
def test_chain_a_outputs_differ_under_poison(W, both, whole):
    real, poison = sg.chain_a_case(W, both, whole, False), sg.chain_a_case(W, both, whole, True)
    certify(real["want"], poison["want"])
    # the inputs themselves: the same sizes, other bits
    pr, pp = real["packed"], poison["packed"]
    assert (len(pr.words), len(pr.items), pr.n_windows, pr.max_bin_bound, pr.all_whole) == \
           (len(pp.words), len(pp.items), pp.n_windows, pp.max_bin_bound, pp.all_whole)
    assert pr.all_whole == int(whole) and pr.n_sequences == sg.A_N_SEQ
    assert differing(pr.words, pp.words)[0] > 0.9 * len(pr.words) and np.array_equal(pr.items, pp.items)
    assert differing(real["pwms"], poison["pwms"])[0] > 0
    if not whole:  # a run shorter than W behind the last invalid base is not visited
        assert pr.n_windows < sg.A_N_SEQ * (sg.A_LEN - W + 1) - len(sg.A_INVALID)


def test_chain_b_outputs_differ_under_poison():
    real, poison = sg.chain_b_want(False), sg.chain_b_want(True)
    certify(real, poison)
    assert real["masked"][0] > 500 and real["masked"][1] > 20  # the mask really takes bases: the later calls see another validity
    lens = [len(c) for c in sg.scan_seqs(False)]
    assert lens == [len(c) for c in sg.scan_seqs(True)] and set(sg.B_LENGTHS) <= set(lens) and len(lens) == sg.B_N_SEQ


def test_strata_of_words_is_the_models_stratum_where_invalid_letters_are_stored_as_A():
    """chain (b) hands pengk_seq_strata the mask's validity over words that keep the masked letters: n follows the validity,
    gc the stored letters (include/pengk.h).  Where both describe the same bases this is tests/motif_match_model.py."""
    import motif_dust_model as md
    import motif_match_model as mm
    for poison in (False, True):
        seqs = sg.scan_seqs(poison)
        s, h = sg.strata_of_words(seqs, seqs)
        ws, wh = mm.strata(seqs)
        assert s.tobytes() == ws.tobytes() and h.tobytes() == wh.tobytes()
    seqs = sg.scan_seqs(False)
    masked, _, _ = md.mask_codes(seqs, sg.B_DUST_T)
    s, _ = sg.strata_of_words(seqs, masked)
    assert 0 < int((s != mm.strata(masked)[0]).sum()) < len(seqs)  # (a masked C or G still counts: another stratum for some)
    assert int((s != mm.strata(seqs)[0]).sum()) > 0  # (... and the mask's validity is read: n is smaller)


def test_chain_c_outputs_differ_under_poison():
    real, poison = sg.chain_c_want(False), sg.chain_c_want(True)
    certify(real, poison)
    # every call has work to show: sites found and bases erased, sequences above the centrality thresholds
    assert real["site_counts"].sum(axis=1).min() > 20 and real["erase_sites"].min() > 5 and real["erased"][0] > 50
    assert real["central_lengths"].sum(axis=1).min() > 50
    # ... and host parameters of its own: no two calls share a motif width
    widths = [w for ws in sg.C_WIDTHS.values() for w in ws]
    assert len(set(widths)) == len(widths)


def test_sixteen_pwms_take_two_lanes():
    assert sg.em_lanes(sg.A_N_PWM, 2) == 2 and sg.em_lanes(sg.A_N_PWM, 1) == 1
    assert sg.em_lanes(15, 2) == 1 and sg.em_lanes(16, 4) == 2 and sg.em_lanes(32, 4) == 4 and sg.em_lanes(1000, 9) == 4
    # the restated formula is the library's: csrc/em.hip, launch_serial_ahead
    with open(os.path.join(ROOT, "peng-motif_amd", "csrc", "em.hip")) as fh:
        src = fh.read()
    assert "int lanes = ctx->em_overlap < 1 ? 1 : ctx->em_overlap > MAX_EM_LANES ? MAX_EM_LANES : ctx->em_overlap;" in src
    assert "while (lanes > 1 && n_pwm < 8 * (int64_t)lanes) --lanes;" in src
    with open(os.path.join(ROOT, "peng-motif_amd", "csrc", "pengk_internal.h")) as fh:
        assert re.search(r"constexpr int MAX_EM_LANES = 4;", fh.read())
    with open(os.path.join(ROOT, "peng-motif_amd", "csrc", "pengk_internal.h")) as fh:
        assert re.search(r"int em_overlap = 2;", fh.read())  # the default the GPU test's first runs rely on


def test_gate_length_rule():
    assert sg.Gate.length_ms(0.5) == 50.0 and sg.Gate.length_ms(5.0) == 100.0 and sg.Gate.length_ms(100.0) == 400.0
