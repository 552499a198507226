"""numpy restatement of the motif scoring (include/pengk.h, "motif scoring"): log-odds quantization,
the background sampler's counter-based draws, the integer ZOOPS scan, histograms, AUC (zoops_score) and occur.
Everything after the quantization is integer arithmetic, so the device must agree with it bit for bit."""
import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
SENTINEL = -2 ** 31


def mix64(x):
    """splitmix64 finalizer on uint64 arrays (wraps mod 2^64)"""
    x = np.asarray(x, np.uint64)
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint64(30))
        x = x * np.uint64(0xBF58476D1CE4E5B9)
        x = x ^ (x >> np.uint64(27))
        x = x * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return x


def log_odds(pwm, bg):
    """S[j][a] = clamp(lround(100 * log2(pwm / bg)), -2000, 2000) in double (a zero probability: -2000)"""
    p = np.asarray(pwm, np.float32).astype(np.float64)
    b = np.asarray(bg, np.float32).astype(np.float64)
    with np.errstate(divide="ignore"):
        v = 100.0 * np.log2(p / b)
    v = np.clip(v, -2000.0, 2000.0)
    # lround: halves away from zero
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int32)


def revcomp_S(S):
    """S_rc[j][a] = S[w-1-j][3-a]"""
    return np.ascontiguousarray(np.asarray(S)[::-1, ::-1])


def thresholds(V, K):
    """uint32 triples for the contexts of orders 0..K (V: the background model's V[0..2] as lists of float32)"""
    out = []
    for k in range(K + 1):
        v = np.asarray(V[k], np.float32).astype(np.float64).reshape(-1, 4)
        for ctx in range(4 ** k):
            c = 0.0
            for b in range(3):
                c += float(v[ctx, b])
                out.append(min(int(np.floor(c * 2.0 ** 32)), 2 ** 32 - 1))
    return np.array(out, np.uint32)


def sample(lens, seed, seq0, K, th):
    """negatives: list of uint8 arrays of bases 0..3, one per length, for global indices seq0, seq0+1, ..."""
    lens = np.asarray(lens, np.int64)
    n = len(lens)
    Lmax = int(lens.max()) if n else 0
    th = np.asarray(th, np.uint64).reshape(-1, 3)
    out = np.zeros((n, max(Lmax, 1)), np.uint8)
    hist = np.zeros(n, np.int64)
    idx = (np.arange(n, dtype=np.uint64) + np.uint64(seq0)) << np.uint64(32)
    for p in range(Lmax):
        with np.errstate(over="ignore"):
            r = mix64(np.uint64(seed) + np.uint64(GOLDEN) * (idx + np.uint64(p + 1))) >> np.uint64(32)
        kk = min(p, K)
        row = 0 if kk == 0 else (1 + (hist & 3) if kk == 1 else 5 + (hist & 15))
        T = th[row] if kk else np.broadcast_to(th[0], (n, 3))
        b = (r >= T[:, 0]).astype(np.int64) + (r >= T[:, 1]) + (r >= T[:, 2])
        hist = ((hist << 2) | b) & 15
        out[:, p] = b
    return [out[i, :lens[i]] for i in range(n)]


def best_scores(seqs, S, both):
    """best window score of every sequence; seqs: byte codes (1..4 = A,C,G,T, else invalid)"""
    S = np.asarray(S, np.int64)
    w = S.shape[0]
    mats = [S, revcomp_S(S)] if both else [S]
    out = np.full(len(seqs), SENTINEL, np.int64)
    for i, c in enumerate(seqs):
        c = np.asarray(c, np.int64)
        L = len(c)
        if L < w:
            continue
        ok = (c >= 1) & (c <= 4)
        bad = np.concatenate([[0], np.cumsum(~ok)])
        starts = np.arange(L - w + 1)
        good = (bad[starts + w] - bad[starts]) == 0
        if not good.any():
            continue
        b = np.where(ok, c - 1, 0)
        cols = b[starts[:, None] + np.arange(w)[None, :]]
        best = None
        for M in mats:
            sc = M[np.arange(w)[None, :], cols].sum(axis=1)[good].max()
            best = sc if best is None else max(best, sc)
        out[i] = best
    return out


def score_range(S):
    S = np.asarray(S, np.int64)
    return int(S.min(axis=1).sum()), int(S.max(axis=1).sum())


def histogram(best, lo, hi):
    best = np.asarray(best, np.int64)
    b = np.where(best == SENTINEL, 0, 1 + np.clip(best, lo, hi) - lo)
    return np.bincount(b, minlength=hi - lo + 2).astype(np.uint64)


def auc(P, N):
    """zoops_score: sum_s P[s] (2 Nneg_below(s) + N[s]) / (2 Npos Nneg), exact integer numerator"""
    P = [int(x) for x in P]
    N = [int(x) for x in N]
    npos, nneg = sum(P), sum(N)
    if npos == 0 or nneg == 0:
        return 0.5
    num, below = 0, 0
    for p, n in zip(P, N):
        num += p * (2 * below + n)
        below += n
    assert num <= 2 ** 62
    return float(num) / (2.0 * npos * nneg)


def occur(P, N):
    P = [int(x) for x in P]
    N = [int(x) for x in N]
    npos, nneg = sum(P), sum(N)
    if npos == 0 or nneg == 0:
        return 0.0
    neg_ge, pos_ge = nneg, npos
    for t in range(len(N)):
        if 100 * neg_ge <= nneg:
            break
        neg_ge -= N[t]
        pos_ge -= P[t]
    fpr, tpr = neg_ge / nneg, pos_ge / npos
    if fpr == 1.0:
        return 0.0
    return min(max((tpr - fpr) / (1.0 - fpr), 0.0), 1.0)


def read_fasta_codes(path):
    """byte codes of a FASTA file as the host reader keeps them (A,C,G,T = 1..4 in either case, else 0; a header
    without sequence is dropped)"""
    seqs, cur = [], None
    lut = np.zeros(256, np.uint8)
    for i, ch in enumerate("ACGT"):
        lut[ord(ch)] = lut[ord(ch.lower())] = i + 1
    with open(path, "rb") as fh:
        for line in fh:
            line = line.rstrip(b"\r\n")
            if line.startswith(b">"):
                if cur is not None:
                    seqs.append(np.concatenate(cur) if cur else np.zeros(0, np.uint8))
                cur = []
            elif line and cur is not None:
                cur.append(lut[np.frombuffer(line, np.uint8)])
    if cur is not None:
        seqs.append(np.concatenate(cur) if cur else np.zeros(0, np.uint8))
    return [x for x in seqs if len(x)]


def flatten(seqs):
    offs = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    codes = np.concatenate(seqs).astype(np.uint8) if seqs else np.zeros(0, np.uint8)
    return codes, offs
