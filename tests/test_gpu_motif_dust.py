"""--mask-low-complexity on the device (include/pengk.h, "masking low-complexity stretches"): pengk_mask_low_complexity
against the numpy model of tests/motif_dust_model.py -- the output validity words bit for bit, both counters exact -- on the
constructed cases that tests/test_motif_dust_cpu.py holds to their classes, across the tile and workgroup seams, without
input validity, in two calls, and then the count of a masked, device-packed set against the oracle's count of the masked
codes."""
import numpy as np
import pytest

import peng_motif_amd as pk
import motif_dust_model as md
import motif_erase_model as me
import motif_score_model as ms
from oracle import oracle as po

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = pk.Context(0)
    yield c
    c.close()


def check_mask(ctx, seqs, T=20, all_valid=False, want=None):
    """the device's mask of the sequences against the model's (want: the model's (masked, bits, touched), if at hand);
    all_valid: the input validity is not given (the sequences must then hold no invalid base)"""
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    out, masked = ctx.mask_low_complexity(scan, T, all_valid=all_valid)
    m, bits, touched = want if want is not None else md.mask_codes(seqs, T)
    words = me.valid_words(m)
    got = out.to_host()[:len(words)]
    bad = np.flatnonzero(got != words)
    assert len(bad) == 0, "first differing validity word %d of %d: %08x, the model %08x" % (bad[0], len(words), got[bad[0]], words[bad[0]])
    assert masked.to_host().tolist() == [bits, touched]
    return bits


def test_symbol():
    assert hasattr(pk.lib(), "pengk_mask_low_complexity")


@pytest.mark.parametrize("case", md.cases(), ids=lambda c: c["name"])
def test_constructed_cases(ctx, case):
    check_mask(ctx, case["seqs"], case["T"])
    if all((np.asarray(c) >= 1).all() for c in case["seqs"]):
        check_mask(ctx, case["seqs"], case["T"], all_valid=True)


def test_threshold_311_masks_nothing_anywhere(ctx):
    seqs = [md.codes_of("A" * 300), md.codes_of("CA" * 150), md.seam_sequence(3000)] + md.random_sequences(4, 60)
    assert check_mask(ctx, seqs, 309) > 0  # (62 equal triplets: 10 * 1891 = 310 * 61 -- at 310 the one top score is not above)
    assert check_mask(ctx, seqs, 310) == 0
    assert check_mask(ctx, seqs, 311) == 0
    assert check_mask(ctx, seqs, 1000) == 0


def test_random_sequences(ctx):
    for T in (1, 10, 20, 45):
        assert check_mask(ctx, md.random_sequences(10 + T, 400, 300), T) > 0


def test_one_sequence_of_70000_bases(ctx):
    """a repeat of 20 .. 66 bases across every multiple of 64 bases: whatever the kernel's tiles are, their seams lie on
    some of them"""
    c = md.seam_sequence()
    assert check_mask(ctx, [c], 20) > 20000
    assert check_mask(ctx, [np.maximum(c, 1)[:50001], c[:257], c[:385], c[:384], c[:513]], 20, all_valid=False) > 10000
    check_mask(ctx, [np.maximum(c, 1)[:30000]], 20, all_valid=True)


@pytest.fixture(scope="module")
def many():
    seqs, idx, pool = md.many_sequences()
    pm, _, _ = md.mask_codes(pool, 20)
    masked = [pm[i] for i in idx]
    lost = np.array([int((np.asarray(a) != np.asarray(b)).sum()) for a, b in zip(pool, pm)])
    return seqs, masked, int(lost[idx].sum()), int((lost[idx] > 0).sum()), lost[idx]


def test_100000_sequences(ctx, many):
    seqs, masked, bits, touched, _ = many
    assert touched > 10000
    check_mask(ctx, seqs, 20, want=(masked, bits, touched))


@pytest.mark.parametrize("cut", [1, 255, 256, 257, 50001])
def test_two_calls_give_the_bits_of_one(ctx, many, cut):
    """the offset arrays split at a sequence: each call writes its own sequences' words, the counters add up"""
    seqs, masked, bits, touched, lost = many
    n = 60000
    lay = pk.ScanLayout(*ms.flatten(seqs[:n]))
    words, valid = ctx.to_device(lay.words), ctx.to_device(lay.valid)
    out = ctx.to_device(np.zeros(len(lay.valid), np.uint32))
    cnt = ctx.to_device(np.zeros(2, np.uint64))
    for a, b in ((0, cut), (cut, n)):
        part = (words, valid, ctx.to_device(lay.offs[a:b]), ctx.to_device(lay.lens[a:b]), b - a)
        ctx.mask_low_complexity(part, 20, out_valid=out, masked=cnt)
    want = me.valid_words(masked[:n])
    assert np.array_equal(out.to_host()[:len(want)], want)
    assert cnt.to_host().tolist() == [int(lost[:n].sum()), int((lost[:n] > 0).sum())]


def test_no_sequence_and_argument_errors(ctx):
    seqs = [md.codes_of("A" * 40)]
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    cnt = ctx.to_device(np.array([5, 7], np.uint64))
    out = ctx.to_device(np.full(2, 0xDEADBEEF, np.uint32))
    ctx.mask_low_complexity(scan, 20, out_valid=out, masked=cnt, n_seq=0)
    assert cnt.to_host().tolist() == [5, 7] and out.to_host().tolist() == [0xDEADBEEF] * 2
    ctx.mask_low_complexity(scan, 20, out_valid=out, masked=cnt)   # added to, not written
    assert cnt.to_host().tolist() == [45, 8]
    for T in (0, -1, 1001):
        with pytest.raises(pk.PengkError) as e:
            ctx.mask_low_complexity(scan, T)
        assert e.value.code == pk.ERR_ARG
    with pytest.raises(pk.PengkError) as e:
        ctx.mask_low_complexity(scan, 20, out_valid=scan[1])
    assert e.value.code == pk.ERR_ARG
    with pytest.raises(pk.PengkError) as e:
        ctx.mask_low_complexity(scan, 20, n_seq=1 << 32)
    assert e.value.code == pk.ERR_ARG
    ctx.mask_low_complexity(scan, 1000)
    ctx.mask_low_complexity(scan, 1)


def test_count_after_mask_and_pack(ctx):
    """mask, pack on the device, count at W = 8: the oracle's count of the masked codes"""
    W = 8
    seqs = md.tracts(1, n=600)
    seqs[5][50] = 0
    masked, bits, touched = md.mask_codes(seqs, 20)
    assert bits > 2000 and touched > 100
    scan = ctx.upload_scan(pk.ScanLayout(*ms.flatten(seqs)))
    out, cnt = ctx.mask_low_complexity(scan, 20)
    assert cnt.to_host().tolist() == [bits, touched]
    _, _, st = ctx.pack_scan(scan, W, valid=out, attach=True)
    for both in (False, True):
        counts, ltot = ctx.count(both)
        if both:
            ctx.mirror(W, counts)
        want, lt = po.count(*ms.flatten(masked), W, both)
        assert int(ltot.to_host()[0]) == lt == st.n_windows
        assert np.array_equal(counts.to_host().astype(np.uint64), want)
