"""numpy restatement of --mask-low-complexity (include/pengk.h, "masking low-complexity stretches"): this
project's own statement of the symmetric DUST criterion of Morgulis et al. 2006.  Integer throughout, so the device must
agree with it bit for bit.  The numbers are NOT promised to be those of NCBI's dustmasker or of sdust.

Per sequence, letters s[0..L) in 0..3 and validity bits v:
  triplet   stands at p (0 <= p <= L-3) iff v[p] & v[p+1] & v[p+2]; t[p] = 16 s[p] + 4 s[p+1] + s[p+2]
  interval  (i, l) = the triplets i .. i+l-1, all standing, 2 <= l <= MAX_L = 62 (at most WINDOW = 64 bases)
  score     num(i, l) / (l - 1), num = sum over triplet values x of c_x (c_x - 1) / 2; compared by cross-multiplication
  high      10 num > T (l - 1)
  perfect   high, and no interval inside it (l' >= 2) has a strictly larger score
  cover     the bases [i, i+l+2) of every perfect interval; the output validity is v & ~cover

mask_bruteforce   the definition read literally: every interval against every interval inside it
mask              the recurrence, vectorised over the starts:
                    c(i, l) = #{p in [i, i+l-1): t[p] = t[i+l-1]} = c(i+1, l-1) + [t[i] == t[i+l-1]]
                    num(i, l) = num(i, l-1) + c(i, l)
                    M(i, l) = the largest score inside (i, l) = max(S(i, l), M(i, l-1), M(i+1, l-1)), M(., 1) = 0/1
                    (i, l) perfect iff high and S(i, l) >= M(i, l-1) and S(i, l) >= M(i+1, l-1)
                  per start only the longest perfect l counts: base b is covered iff max over i <= b of
                  (i + lmax(i) + 2) > b (a start further than 63 bases to the left ends at or before b)."""
import numpy as np

WINDOW = 64
MAX_L = WINDOW - 2
DEFAULT_T = 20


def codes_of(s):
    return np.array(["NACGT".index(x) for x in s], np.uint8)


def letters(codes):
    """(seq, valid) of byte codes (0 = other, A,C,G,T = 1..4): letters 0..3 (0 where invalid) and the validity bits"""
    c = np.asarray(codes, np.uint8)
    ok = (c >= 1) & (c <= 4)
    return np.where(ok, c - 1, 0).astype(np.int64), ok


def triplets(seq, valid):
    s = np.asarray(seq, np.int64)
    v = np.asarray(valid, bool)
    if len(s) < 3:
        return np.zeros(0, np.int64), np.zeros(0, bool)
    return 16 * s[:-2] + 4 * s[1:-1] + s[2:], v[:-2] & v[1:-1] & v[2:]


# ---- the definition, literally ----------------------------------------------------------------------------------------------
def interval_nums(t, stand):
    """N[i, l] = num(i, l) for 1 <= l <= MAX_L where the interval stands, else -1 (column 0 unused)"""
    nt = len(t)
    N = np.full((nt, MAX_L + 1), -1, np.int64)
    for i in range(nt):
        n = min(MAX_L, nt - i)
        bad = np.flatnonzero(~stand[i:i + n])
        if len(bad):
            n = int(bad[0])
        if n == 0:
            continue
        onehot = np.zeros((n, 64), np.int64)
        onehot[np.arange(n), t[i:i + n]] = 1
        c = np.cumsum(onehot, axis=0)  # c[l-1, x]: occurrences of x among the triplets i .. i+l-1
        N[i, 1:n + 1] = (c * (c - 1) // 2).sum(axis=1)
    return N


def perfect_intervals(seq, valid, T=DEFAULT_T):
    """[(i, l)] of every perfect interval, by the definition"""
    t, stand = triplets(seq, valid)
    N = interval_nums(t, stand)
    out = []
    ii = np.arange(MAX_L)[:, None]
    ll = np.arange(MAX_L + 1)[None, :]
    for i in range(len(t)):
        for l in range(2, MAX_L + 1):
            num = N[i, l]
            if num < 0:
                break
            if not 10 * num > T * (l - 1):
                continue
            sub = N[i:i + l - 1, :l + 1]  # the starts i .. i+l-2, the lengths 0 .. l
            inside = (ll[:, :l + 1] >= 2) & (ii[:sub.shape[0]] + ll[:, :l + 1] <= l)
            assert (sub[inside] >= 0).all()  # (an interval inside a standing one stands)
            larger = inside & (sub * (l - 1) > num * (ll[:, :l + 1] - 1))
            if not larger.any():
                out.append((i, l))
    return out


def mask_bruteforce(seq, valid, T=DEFAULT_T):
    """the output validity bits of one sequence, by the definition"""
    v = np.asarray(valid, bool).copy()
    for i, l in perfect_intervals(seq, valid, T):
        v[i:i + l + 2] = False
    return v


# ---- the recurrence ------------------------------------------------------------------------------------------------------------
def longest_perfect(t, stand, T=DEFAULT_T):
    """lmax[i]: the longest l at which (i, l) is perfect, 0 if none.  One array over any number of sequences: a triplet
    that does not stand ends every interval, so sequences laid behind one another with an invalid base between them do
    not see each other."""
    nt = len(t)
    lmax = np.zeros(nt, np.int32)
    if nt == 0:
        return lmax
    t = np.asarray(t, np.int32)
    pos = np.arange(nt)
    bad = np.where(~stand, pos, nt)
    nxt = np.minimum.accumulate(bad[::-1])[::-1]  # the first triplet >= i that does not stand
    run = np.minimum(nxt - pos, MAX_L).astype(np.int32)
    c = np.zeros(nt + 1, np.int32)
    num = np.zeros(nt, np.int32)
    Mn = np.zeros(nt + 1, np.int32)
    Md = np.ones(nt + 1, np.int32)
    tpad = np.concatenate([t, np.full(MAX_L, -1, np.int32)])
    for l in range(2, MAX_L + 1):
        d = l - 1
        cn = c[1:] + (t == tpad[d:d + nt])
        num = num + cn
        on, od, nn, nd = Mn[:-1], Md[:-1], Mn[1:], Md[1:]
        perfect = (10 * num > T * d) & (num * od >= on * d) & (num * nd >= nn * d) & (run >= l)
        lmax[perfect] = l
        nb = nn * od > on * nd  # the neighbour's M is the larger of the two
        bn, bd = np.where(nb, nn, on), np.where(nb, nd, od)
        s = num * bd >= bn * d
        c[:-1] = cn
        Mn[:-1] = np.where(s, num, bn)
        Md[:-1] = np.where(s, d, bd)
    return lmax


def cover_of(lmax, L):
    """bool per base: covered by [i, i + lmax[i] + 2) of some start with lmax[i] > 0 (a running maximum)"""
    end = np.zeros(L, np.int64)
    n = len(lmax)
    end[:n] = np.where(lmax > 0, np.arange(n) + lmax + 2, 0)
    return np.maximum.accumulate(end) > np.arange(L) if L else np.zeros(0, bool)


def mask(seq, valid, T=DEFAULT_T):
    """the output validity bits of one sequence, by the recurrence"""
    v = np.asarray(valid, bool)
    t, stand = triplets(seq, v)
    return v & ~cover_of(longest_perfect(t, stand, T), len(v))


def mask_codes(seqs, T=DEFAULT_T):
    """(masked, bits, touched): the sequences (byte codes) with every covered base set to code 0, the valid bases that were
    covered and the sequences with at least one.  All sequences in one pass of the recurrence."""
    seqs = [np.asarray(c, np.uint8) for c in seqs]
    if not seqs:
        return [], 0, 0
    cat = np.zeros(sum(len(c) + 1 for c in seqs), np.uint8)  # (one invalid base behind every sequence)
    starts, g = [], 0
    for c in seqs:
        starts.append(g)
        cat[g:g + len(c)] = c
        g += len(c) + 1
    s, v = letters(cat)
    out = mask(s, v, T)
    masked, bits, touched = [], 0, 0
    for c, g in zip(seqs, starts):
        gone = v[g:g + len(c)] & ~out[g:g + len(c)]
        n = int(gone.sum())
        bits += n
        touched += n > 0
        masked.append(np.where(gone, 0, c).astype(np.uint8))
    return masked, bits, touched


def masked_runs(seqs, masked):
    """[(sequence index, start, end)] of every maximal run of bases that the mask took, in order (--mask-report)"""
    out = []
    for k, (c, m) in enumerate(zip(seqs, masked)):
        gone = np.concatenate([[False], np.asarray(c) != np.asarray(m), [False]])
        edge = np.flatnonzero(gone[1:] != gone[:-1])
        out += [(k, int(a), int(b)) for a, b in zip(edge[::2], edge[1::2])]
    return out


def render_report(runs):
    return "".join("%d\t%d\t%d\n" % r for r in runs)


# ---- helpers of the scenarios -------------------------------------------------------------------------------------------------
def period(word):
    """the smallest p with word[k] == word[k + p] for every k"""
    return next(p for p in range(1, len(word) + 1) if all(word[k] == word[k + p] for k in range(len(word) - p)))


def de_bruijn_flank():
    """a string over ACGT in which no triplet occurs twice and no letter three times in a row: the order-3 de Bruijn
    sequence (66 letters, every triplet once) minus its four homopolymer triplets"""
    k, n = 4, 3
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    s = "".join("ACGT"[x] for x in seq + seq[:2])
    for x in "ACGT":
        s = s.replace(x * 3, x * 2)
    return s


def tracts(seed, n=2000, L=100, word="TGACTCAGCA", f_word=0.3, f_tract=0.2, p=0.85):
    """the scenario of the mask's purpose: n uniform sequences of L bases, `word` planted in a share f_word of them (every
    letter kept with probability p, else uniform among the others), a poly-A or (CA)n tract of 20-40 bases in a share f_tract"""
    rng = np.random.default_rng(seed)
    seqs = [rng.integers(1, 5, L).astype(np.uint8) for _ in range(n)]
    w = codes_of(word)
    for i in np.flatnonzero(rng.random(n) < f_tract).tolist():
        m = int(rng.integers(20, 41))
        q = int(rng.integers(0, L - m + 1))
        seqs[i][q:q + m] = 1 if rng.random() < 0.5 else np.tile(codes_of("CA"), 20)[:m]
    for i in np.flatnonzero(rng.random(n) < f_word).tolist():
        q = int(rng.integers(0, L - len(w) + 1))
        c = w.copy()
        for j in np.flatnonzero(rng.random(len(w)) >= p).tolist():
            c[j] = (c[j] - 1 + rng.integers(1, 4)) % 4 + 1
        seqs[i][q:q + len(w)] = c
    return seqs


def fasta_text(seqs):
    return "".join(">s%d\n%s\n" % (k, "".join("NACGT"[x] for x in c)) for k, c in enumerate(seqs))


# ---- constructed cases (tests/test_motif_dust_cpu.py certifies their classes, tests/test_gpu_motif_dust.py runs them) -------
def unit(p):
    """a repeat unit of period exactly p"""
    return {1: "A", 2: "CA", 3: "CAG", 4: "GATA", 7: "GGAATCT"}[p]


def cases():
    """[dict(name, cls, seqs, T, ...)]: one constructed input per class of the mask.  cls names what the CPU test holds the
    case to: 'run' / 'runs_exact' (the runs (sequence, first, last + 1) are masked exactly and nothing else), 'runs' (every run
    is masked from its first to its last base, in one piece), 'nothing' (no base masked), 'ties' (the named interval is
    perfect and holds an interval of exactly its score), 'overlap' (two perfect intervals overlap, neither inside the other),
    'model' (the two restatements agree, no class of its own)."""
    F = de_bruijn_flank()
    h = len(F) // 2
    out = []

    def case(name, cls, strs, T=DEFAULT_T, **kw):
        out.append(dict(name=name, cls=cls, seqs=[codes_of(s) if isinstance(s, str) else np.asarray(s, np.uint8) for s in strs],
                        T=T, **kw))

    def flanked(x, n):
        """x^n in the middle of the flank, where x does not continue on either side; (string, first, last + 1)"""
        a, b = F[:h], F[h:]
        while a[-1] == x:
            a = a[:-1]
        while b[0] == x:
            b = b[1:]
        return a + x * n + b, len(a), len(a) + n

    rng = np.random.default_rng(123)
    case("lengths", "model", [rng.integers(1, 3, L).astype(np.uint8) for L in (0, 1, 2, 3, 4, 31, 32, 33, 63, 64, 65, 66, 67)])
    case("lengths_homopolymer", "model", ["A" * L for L in (0, 1, 2, 3, 4, 31, 32, 33, 63, 64, 65, 66, 67)])
    # a homopolymer of n bases is n - 2 equal triplets: num = (n-2)(n-3)/2 over l - 1 = n - 3, the score (n - 2) / 2
    for T, stays, goes in ((20, 6, 7), (10, 4, 5), (30, 8, 9)):
        for x in "AG":
            s, a, b = flanked(x, stays)
            case("homopolymer_%s%d_T%d_at_equality" % (x, stays, T), "nothing", [s], T)
            s, a, b = flanked(x, goes)
            case("homopolymer_%s%d_T%d" % (x, goes, T), "run", [s], T, run=(0, a, b))
    s7 = flanked("A", 7)[0]
    case("T1", "model", [s7, F, "ACACACAC" + F], 1)
    # 62 equal triplets score 1891 / 61 = 31, the largest score there is: 10 * 1891 = 310 * 61, so T = 310 already masks nothing
    case("T309", "model", ["A" * 64, "A" * 200, s7], 309)
    case("T310", "nothing", ["A" * 64, "A" * 200, s7, "CA" * 100], 310)
    case("T311", "nothing", ["A" * 64, "A" * 200, s7, "CA" * 100], 311)
    for p in (1, 2, 3, 4, 7):
        for n in (61, 62, 63, 64, 65, 66, 67, 200):
            strs, runs = [], []
            for k, al in enumerate(range(32)):
                pre = F[:al]
                while pre and pre[-1] == unit(p)[-1]:  # (the run must not begin earlier than it says)
                    pre = pre[:-1] + ("T" if pre[-1] != "T" else "C")
                post = "T" if (unit(p) * n)[n % p] != "T" else "C"
                strs.append(pre + (unit(p) * n)[:n] + post + F[al:al + 9])
                runs.append((k, len(pre), len(pre) + n))
            # (the flank holds every triplet once, so a repeat of period > 2 may take a few flank bases with it)
            case("period%d_%dbases_every_alignment" % (p, n), "runs_exact" if p <= 2 else "runs", strs, runs=runs)
    run = "A" * 30
    for k in range(3):  # one invalid base at each position of a triplet inside a run: two runs, each judged alone
        q = 12 + k
        case("invalid_base_in_run_%d" % k, "model", [F[:20] + run[:q] + "N" + run[q + 1:] + F[20:], run[:q] + "N" + run[q + 1:]])
    case("invalid_base_leaves_a_short_half", "model", ["A" * 7 + "N" + "A" * 6 + "C", "A" * 6 + "N" + "A" * 7])
    case("invalid_first_and_last_base", "model", ["N" + "A" * 20, "A" * 20 + "N", "N" + "A" * 20 + "N", "N", "NN", "NNN", "ANA"])
    # a perfect interval (sequence, i, l) with an interval inside it (i2, l2) of exactly its score: equality keeps it perfect
    case("equal_scores_inside", "ties", ["AACAAACCCCCCCCCCCAACCCCCAAC", "CCACACCCCACACACACACCCACACAAA", "CACACACCCCCCAACCCCCCCCAA"],
         ties=[(0, 9, 13, 9, 6), (1, 3, 21, 8, 16), (2, 7, 13, 14, 6)])
    case("two_overlapping_perfect_intervals", "overlap", [F[:10] + "A" * 12 + "CACACACACACACACACACACACA" + F[10:],
                                                         "A" * 10 + "T" + "A" * 10, "A" * 40 + "CA" * 20 + "CAG" * 12])
    return out


def seam_sequence(L=70000, seed=5):
    """one sequence of L bases with a repeat of 20 .. 66 bases laid across every multiple of 64 bases"""
    rng = np.random.default_rng(seed)
    c = rng.integers(1, 5, L).astype(np.uint8)
    for k, g in enumerate(range(64, L - 70, 64)):
        n = 20 + k % 47
        u = codes_of(unit((1, 2, 3, 4, 7)[k % 5]))
        a = g - int(rng.integers(1, n))  # (the run straddles g)
        c[a:a + n] = np.tile(u, n)[:n]
    c[rng.integers(0, L, 40)] = 0
    return c


def many_sequences(n=100000, pool=3000, seed=6):
    """(sequences, index into the pool, the pool): n sequences of 1 .. 300 bases drawn from a pool of distinct ones, so
    that the model runs once per distinct sequence; skewed compositions, tracts and invalid bases"""
    rng = np.random.default_rng(seed)
    P = []
    for k in range(pool):
        L = k % 300 + 1
        w = rng.dirichlet(np.full(4, 0.7))
        c = (rng.choice(4, L, p=w) + 1).astype(np.uint8)
        if k % 3 == 0 and L > 12:
            m = int(rng.integers(6, min(L, 70)))
            q = int(rng.integers(0, L - m + 1))
            c[q:q + m] = np.tile(codes_of(unit((1, 2, 3, 4, 7)[k % 5])), m)[:m]
        if k % 7 == 0:
            c[rng.integers(0, L)] = 0
        P.append(c)
    idx = rng.integers(0, pool, n)
    idx[:pool] = np.arange(pool)
    return [P[i] for i in idx], idx, P


def random_sequences(seed, n, max_len=140):
    """skewed compositions and invalid bases, lengths 0 .. max_len"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        L = k if k < 8 else int(rng.integers(0, max_len + 1))  # (the shortest lengths are always among them)
        w = rng.dirichlet(np.full(4, (0.15, 0.4, 1.0)[k % 3]))
        c = (rng.choice(4, L, p=w) + 1).astype(np.uint8)
        if k % 2 and L:
            c[rng.integers(0, L, 1 + k % 3)] = 0
        out.append(c)
    return out
