"""numpy restatement of the hold-out split and test (--holdout; include/pengk.h, "a hold-out share"): the
class of every sequence (one hash of its global index against a threshold), the two compacted shares,
pengk_holdout_summary on top of motif_enrich_model's summary and Fisher tail, and the TSV the CLI writes.  Up to the
histograms everything is integer, so the device must agree with it bit for bit."""
import math

import numpy as np

import motif_enrich_model as me
import motif_score_model as ms
import motif_sites_model as mst

GOLDEN = ms.GOLDEN
COLUMNS = ("motif\tconsensus\tthreshold_bits\ttrain_pos_hits\ttrain_neg_hits\ttrain_log10_adj_p\thold_pos_hits\thold_pos_scored\t"
           "hold_neg_hits\thold_neg_scored\thold_log10_p\thold_log10_E\thold_enrichment\n")


# ---- the split --------------------------------------------------------------------------------------------------------------
def threshold_of(fraction):
    """the CLI's threshold: (uint64_t)(F * 4294967296.0)"""
    return int(fraction * 4294967296.0)


def classes(seed, seq0, n_seq, threshold, index=None):
    """uint8[n_seq]: 1 (hold-out) iff mix64(seed + GOLDEN * (g + 1)) >> 32 < threshold, g = seq0 + (index[i] or i)"""
    i = np.arange(n_seq, dtype=np.uint64) if index is None else np.asarray(index, np.uint64)
    with np.errstate(over="ignore"):
        g = np.uint64(seq0) + i
        r = ms.mix64(np.uint64(seed & ms.M64) + np.uint64(GOLDEN) * (g + np.uint64(1))) >> np.uint64(32)
    if threshold >= 1 << 32:  # (r < 2^32 always)
        return np.ones(n_seq, np.uint8)
    return (r < np.uint64(threshold)).astype(np.uint8)


def split(seed, seq0, n_seq, threshold, index=None):
    """(index0, index1): the local indices of the training and of the hold-out share, in file order"""
    c = classes(seed, seq0, n_seq, threshold, index)
    return np.flatnonzero(c == 0).astype(np.uint32), np.flatnonzero(c == 1).astype(np.uint32)


# ---- the summary ------------------------------------------------------------------------------------------------------------
def summary(train_pos, train_neg, hold_pos, hold_neg, thr, n_train_pos, n_train_neg, n_hold_pos, n_hold_neg):
    """pengk_holdout_summary: a dict with the fields of pengk_holdout"""
    tr = me.summary(train_pos, train_neg, thr, n_train_pos, n_train_neg)
    out = dict(threshold=tr["threshold"], n_thresholds=tr["n_thresholds"], train_pos_hits=tr["pos_hits"],
               train_neg_hits=tr["neg_hits"], train_log10_adj_pvalue=tr["log10_adj_pvalue"], hold_pos_hits=0, hold_neg_hits=0,
               hold_log10_pvalue=0.0)
    if tr["n_thresholds"]:
        k = tr["threshold"] - thr
        a, b = sum(int(x) for x in hold_pos[k:]), sum(int(x) for x in hold_neg[k:])
        out.update(hold_pos_hits=a, hold_neg_hits=b, hold_log10_pvalue=me.log10_sf(n_hold_pos + n_hold_neg, a + b, n_hold_pos, a))
    out["hold_enrichment"] = me.enrichment(out["hold_pos_hits"], out["hold_neg_hits"], n_hold_pos, n_hold_neg)
    return out


# ---- found motifs on the four sets ------------------------------------------------------------------------------------------
def analyse(sets, Ss, bg0, P, both):
    """per motif (its integer log-odds S, w x 4): dict(thr, hi, hists, scored, summary); sets: the four sequence lists
    (training input, training negatives, hold-out input, hold-out negatives) as byte codes"""
    packed = [me.Packed(s) for s in sets]
    out = []
    for S in Ss:
        lo, tail = mst.tail_pvalues(S, bg0)
        thr, hi = mst.threshold(lo, tail, P), me.score_hi(S)
        hs = [me.histogram(me.best_scores(p, S, both), thr, hi) for p in packed]
        out.append(dict(thr=thr, hi=hi, hists=[h for h, _ in hs], scored=[n for _, n in hs],
                        summary=summary(*[h for h, _ in hs], thr, *[n for _, n in hs])))
    return out


def log10_evalue(s, n_motifs):
    return min(0.0, s["hold_log10_pvalue"] + math.log10(n_motifs)) if n_motifs else 0.0


def consensus(S):
    return "".join("ACGT"[int(np.argmax(row))] for row in np.asarray(S))


def header(fraction, seed, sizes):
    """sizes: the four sets' sequence counts (training input, training negatives, hold-out input, hold-out negatives)"""
    return "# holdout fraction %.6g seed %d train_pos %d train_neg %d hold_pos %d hold_neg %d\n" % ((fraction, seed) + tuple(sizes))


def render(ids, Ss, results, fraction, seed, sizes):
    """the --holdout TSV (str): one line per motif in the order given"""
    lines = [header(fraction, seed, sizes), COLUMNS]
    n = len(results)
    for mid, S, r in zip(ids, Ss, results):
        s = r["summary"]
        lines.append("%s\t%s\t%s\t%d\t%d\t%.3f\t%d\t%d\t%d\t%d\t%.3f\t%.3f\t%.3f\n" % (
            mid, consensus(S), mst.fmt_score(s["threshold"]), s["train_pos_hits"], s["train_neg_hits"], s["train_log10_adj_pvalue"],
            s["hold_pos_hits"], r["scored"][2], s["hold_neg_hits"], r["scored"][3], s["hold_log10_pvalue"], log10_evalue(s, n),
            s["hold_enrichment"]))
    return "".join(lines)
