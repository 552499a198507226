"""numpy restatement of the motif sites (--sites; include/pengk.h, "motif sites"): the exact tail
p-values of an integer log-odds matrix, the per-motif threshold, the enumeration of every window strand at or above it
and the TSV the CLI writes.  After the threshold everything is integer, so the device must agree with it bit for bit."""
import re

import numpy as np

from motif_score_model import revcomp_S

HEADER = "#motif_index\tmotif_id\tsequence_name\tstart\tstop\tstrand\tscore\tp_value\tmatched_sequence\n"


def tail_pvalues(S, bg):
    """(lo, tail): tail[t - lo] = P(score >= t) for one window strand with bases drawn from bg (float32 taken as double).
    q_0 = delta(0); q_{j+1}[t] = sum over a = 0..3 in order of q_j[t - S[j][a]] * bg[a], each from 0.0; the tail summed
    sequentially from the highest score down."""
    S = np.asarray(S, np.int64)
    b = np.asarray(bg, np.float32).astype(np.float64)
    q, clo = np.ones(1), 0
    for j in range(S.shape[0]):
        mn, mx = int(S[j].min()), int(S[j].max())
        nq = np.zeros(len(q) + mx - mn)
        for a in range(4):
            s = int(S[j, a]) - mn  # (terms outside q's range would add +0.0: the same bits)
            nq[s:s + len(q)] += q * b[a]
        q, clo = nq, clo + mn
    tail = np.zeros(len(q))
    acc = 0.0
    for t in range(len(q) - 1, -1, -1):
        acc += q[t]
        tail[t] = acc
    return clo, tail


def threshold(lo, tail, p):
    """the smallest integer t with P(score >= t) <= p; lo + len(tail) (= hi + 1) when none qualifies"""
    ok = np.nonzero(tail <= p)[0]
    return lo + int(ok[0]) if len(ok) else lo + len(tail)


def sites(seqs, S, t, both):
    """the sites of one motif, in order (sequence, position, + before -): a list of (seq, pos, strand, score);
    seqs: byte codes (1..4 = A,C,G,T, else invalid)"""
    S = np.asarray(S, np.int64)
    w = S.shape[0]
    mats = [S, revcomp_S(S)] if both else [S]
    out = []
    for i, c in enumerate(seqs):
        c = np.asarray(c, np.int64)
        L = len(c)
        if L < w:
            continue
        ok = (c >= 1) & (c <= 4)
        bad = np.concatenate([[0], np.cumsum(~ok)])
        starts = np.arange(L - w + 1)
        good = (bad[starts + w] - bad[starts]) == 0
        b = np.where(ok, c - 1, 0)
        cols = b[starts[:, None] + np.arange(w)[None, :]]
        sc = [M[np.arange(w)[None, :], cols].sum(axis=1) for M in mats]
        hit = np.zeros((len(starts), len(mats)), bool)
        for k in range(len(mats)):
            hit[:, k] = good & (sc[k] >= t)
        for p, k in zip(*np.nonzero(hit)):  # (row-major: position, then + before -)
            out.append((i, int(p), int(k), int(sc[k][p])))
    return out


def all_sites(seqs, Ss, ts, both):
    """every motif's sites in the --sites order, as the structured array Context.motif_sites returns"""
    rows = [(m,) + s for m, (S, t) in enumerate(zip(Ss, ts)) for s in sites(seqs, S, t, both)]
    out = np.zeros(len(rows), [("motif", np.int64), ("seq", np.uint64), ("pos", np.uint32), ("strand", np.uint8), ("score", np.int32)])
    for k, (m, i, p, st, sc) in enumerate(rows):
        out[k] = (m, i, p, st, sc)
    return out


def fmt_score(s):
    """s / 100 with exactly two decimals, from the integer"""
    s = int(s)
    return "%s%d.%02d" % ("-" if s < 0 else "", abs(s) // 100, abs(s) % 100)


def render(seqs, names, motif_ids, Ss, bg, P, both, header=True, first_index=1):
    """the --sites TSV (str) of motifs Ss (in the MEME file's order) over seqs (byte codes) named names"""
    lines = [HEADER] if header else []
    for m, S in enumerate(Ss):
        lo, tail = tail_pvalues(S, bg)
        t = threshold(lo, tail, P)
        w = len(S)
        for i, p, st, sc in sites(seqs, S, t, both):
            bases = "".join("ACGT"[x - 1] for x in seqs[i][p:p + w])
            if st:
                bases = bases[::-1].translate(str.maketrans("ACGT", "TGCA"))
            lines.append("%d\t%s\t%s\t%d\t%d\t%s\t%s\t%.3g\t%s\n" % (m + first_index, motif_ids[m], names[i], p + 1, p + w, "+-"[st],
                                                                    fmt_score(sc), tail[sc - lo], bases))
    return "".join(lines)


def read_fasta_names(path):
    """the record names the CLI writes: the header without '>', cut at the first whitespace, of the records the reader
    keeps (an empty header: the record's 1-based index among them)"""
    names, cur, has = [], None, False
    with open(path, "rb") as fh:
        for line in fh:
            line = line.rstrip(b"\r\n")
            if line.startswith(b">"):
                if cur is not None and has:
                    names.append(cur)
                cur, has = line[1:].decode(), False
            elif line and cur is not None:
                has = True
    if cur is not None and has:
        names.append(cur)
    out = []
    for k, n in enumerate(names):
        out.append(re.split(r"[ \t\v\f\r]", n)[0] if n else str(k + 1))
    return out
