"""numpy restatement of --erase (include/pengk.h, "erasing sites and packing on the device"): the mask
that the sites of a set of motifs leave of a sequence set, the count layout the host packer writes for what is left,
and the report's TSV.  Integer throughout, so the device must agree with it bit for bit.

mask   built on motif_sites_model.sites: a site of motif m at p covers the bases [p, p + w_m); every motif is judged
       against the input's validity; a covered base becomes code 0 (invalid).
pack   the scan rule of the reference, resolved as csrc/pack.cpp does: a sequence is cut into runs of >= W valid bases;
       behind a run that an invalid base at q ended the scan resumes at q + 2, behind a stretch too short at q + 1.
       Only run bases are stored, behind FRONT_PAD zero bases, 32 per word, (pad + bases + 31) / 32 + 4 words; a run of n
       windows becomes ceil(n / M) items (stream offset | windows << 40 | continues << 56)."""
import numpy as np

import motif_sites_model as mst

FRONT_PAD = 64
DEFAULT_ITEM_WINDOWS = 256
REPORT_HEADER = "#round\tmotif_id\twidth\tthreshold\tsites\tround_seeds\tround_windows\tround_bases_erased\n"


# ---- mask ------------------------------------------------------------------------------------------------------------
def cover(seqs, Ss, ts, both):
    """(cover, sites): cover[i] = bool per base of sequence i, True where a site of some motif lies over it;
    sites[m] = the site window strands of motif m"""
    cov = [np.zeros(len(c), bool) for c in seqs]
    n_sites = np.zeros(len(Ss), np.uint64)
    for m, (S, t) in enumerate(zip(Ss, ts)):
        w = len(S)
        for i, p, _, _ in mst.sites(seqs, S, t, both):
            cov[i][p:p + w] = True
            n_sites[m] += 1
    return cov, n_sites


def mask(seqs, Ss, ts, both):
    """(masked, sites, erased): the sequences with every covered base set to code 0, the site window strands per motif
    and the number of valid bases that were covered"""
    cov, n_sites = cover(seqs, Ss, ts, both)
    out, erased = [], 0
    for c, v in zip(seqs, cov):
        c = np.asarray(c, np.uint8)
        ok = (c >= 1) & (c <= 4)
        erased += int((ok & v).sum())
        out.append(np.where(v, 0, c).astype(np.uint8))
    return out, n_sites, erased


def valid_words(seqs):
    """the validity words of the scan layout: every sequence from a word boundary, bit k of word j = base 32 j + k is
    valid, the bits beyond the end 0"""
    out = []
    for c in seqs:
        c = np.asarray(c, np.uint8)
        ok = np.zeros((len(c) + 31) // 32 * 32, np.uint64)
        ok[:len(c)] = (c >= 1) & (c <= 4)
        out.append((ok.reshape(-1, 32) << np.arange(32, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint32))
    return np.concatenate(out) if out else np.zeros(0, np.uint32)


# ---- pack ------------------------------------------------------------------------------------------------------------
def runs(c, W):
    """the visited runs of one sequence: [(start, length)]"""
    c = np.asarray(c)
    L = len(c)
    bad = np.flatnonzero((c < 1) | (c > 4)).tolist() + [L]
    out, i, k = [], 0, 0
    while i < L:
        while bad[k] < i:
            k += 1
        j = bad[k]
        if j - i >= W:
            out.append((i, j - i))
            i = j + 2
        else:
            i = j + 1
    return out


def pack(seqs, W, item_windows=0):
    """dict(words, items, n_bases, n_windows, max_bin_bound, all_whole, max_len) of the sequences (byte codes)"""
    M = item_windows or DEFAULT_ITEM_WINDOWS
    stored, items = [np.zeros(FRONT_PAD, np.uint64)], []
    g, n_windows, bound, all_whole, max_len = FRONT_PAD, 0, 0, 1, 0
    for c in seqs:
        c = np.asarray(c, np.uint8)
        max_len = max(max_len, len(c))
        rr = runs(c, W)
        if not (len(rr) == 1 and rr[0] == (0, len(c))):
            all_whole = 0
        for start, n in rr:
            stored.append(c[start:start + n].astype(np.uint64) - np.uint64(1))
            nwin = n - W + 1
            n_windows += nwin
            bound += (nwin + W - 1) // W
            for f in range(0, nwin, M):
                items.append((g + f) | (min(M, nwin - f) << 40) | ((1 if f else 0) << 56))
            g += n
    n_words = (g + 31) // 32 + 4
    b = np.zeros(n_words * 32, np.uint64)
    b[:g] = np.concatenate(stored)
    words = (b.reshape(-1, 32) << (np.uint64(2) * np.arange(32, dtype=np.uint64))[None, :]).sum(axis=1).astype(np.uint64)
    return dict(words=words, items=np.array(items, np.uint64), n_bases=g - FRONT_PAD, n_windows=n_windows, max_bin_bound=bound,
                all_whole=all_whole, max_len=max_len)


# ---- report ------------------------------------------------------------------------------------------------------------
def render_report(rounds):
    """the --erase TSV.  rounds: [dict(seeds, windows, bases_erased, motifs=[(motif_id, width, threshold, sites)])] in
    round order; a round that ran and reported nothing has no motifs and gets one line with motif_id '-'"""
    lines = [REPORT_HEADER]
    for r, rd in enumerate(rounds):
        tail = "%d\t%d\t%d\n" % (rd["seeds"], rd["windows"], rd["bases_erased"])
        if not rd["motifs"]:
            lines.append("%d\t-\t0\t-\t0\t%s" % (r + 1, tail))
        for mid, w, thr, n in rd["motifs"]:
            lines.append("%d\t%s\t%d\t%s\t%d\t%s" % (r + 1, mid, w, mst.fmt_score(thr), n, tail))
    return "".join(lines)


# ---- helpers of the scenarios -------------------------------------------------------------------------------------------
def codes_of(s):
    return np.array(["NACGT".index(x) for x in s], np.uint8)


def consensus_pwm(word, p=0.85):
    """w x 4 float64: p on the consensus letter (IUPAC S: C and G share it), the rest spread evenly"""
    sets = {"A": "A", "C": "C", "G": "G", "T": "T", "S": "CG", "W": "AT", "R": "AG", "Y": "CT", "K": "GT", "M": "AC", "N": "ACGT"}
    out = np.zeros((len(word), 4))
    for j, x in enumerate(word):
        on = ["ACGT".index(a) for a in sets[x]]
        off = [a for a in range(4) if a not in on]
        out[j, on] = p / len(on) if off else 0.25
        out[j, off] = (1.0 - p) / max(len(off), 1)
    return out


def shares_kmer(a, b, k=6):
    """a and b (strings over ACGT) share a k-mer on either strand"""
    rc = b[::-1].translate(str.maketrans("ACGT", "TGCA"))
    ks = {b[i:i + k] for i in range(len(b) - k + 1)} | {rc[i:i + k] for i in range(len(rc) - k + 1)}
    return any(a[i:i + k] in ks for i in range(len(a) - k + 1))


def planted(seed, n=2000, L=100, A="TGACTCAGCA", fa=0.5, B="GGCTGGAGTG", fb=0.03):
    """n uniform sequences of L bases; B planted in a share fb of them, then A in a share fa, each at a uniform position"""
    rng = np.random.default_rng(seed)
    seqs = [rng.integers(1, 5, L).astype(np.uint8) for _ in range(n)]
    for word, f in ((B, fb), (A, fa)):
        c = codes_of(word)
        for i in np.flatnonzero(rng.random(n) < f).tolist():
            p = int(rng.integers(0, L - len(c) + 1))
            seqs[i][p:p + len(c)] = c
    return seqs


# ---- constructed cases (tests/test_motif_erase_cpu.py certifies their classes, tests/test_gpu_motif_erase.py runs them) ---
SCAN_TABLES = 40  # csrc/scan_walk.h: 4-mer chunk tables of one motif group in LDS


def groups(lens, both):
    """the LDS group of every motif: greedy in motif order, ceil(w / 4) tables per strand, SCAN_TABLES per group"""
    out, g, used = [], -1, SCAN_TABLES + 1
    for w in lens:
        need = (w + 3) // 4 * (2 if both else 1)
        if g < 0 or used + need > SCAN_TABLES:
            g, used = g + 1, 0
        used += need
        out.append(g)
    return out


def word_S(word, on=100, off=-100):
    """the matrix that scores len(word) * on on the word alone"""
    S = np.full((len(word), 4), off, np.int32)
    S[np.arange(len(word)), ["ACGT".index(x) for x in word]] = on
    return S


def score_range(S):
    S = np.asarray(S, np.int64)
    return int(S.min(axis=1).sum()), int(S.max(axis=1).sum())


def mask_cases():
    """[dict(name, seqs, Ss, ts, both)]: one constructed input per class of the mask"""
    rng = np.random.default_rng(77)
    C = "C" * 40
    out = []

    def case(name, strs, Ss, ts, both=True):
        seqs = [codes_of(s) if isinstance(s, str) else np.asarray(s, np.uint8) for s in strs]
        out.append(dict(name=name, seqs=seqs, Ss=[np.asarray(S, np.int32) for S in Ss], ts=list(ts), both=both))

    acgg = word_S("ACGG")  # (its reverse complement CCGT is another word)
    case("first_and_last_window", ["ACGG" + C + "ACGG"], [acgg], [400])
    case("overlapping_sites", ["C" * 5 + "AAAAAA" + "C" * 30], [word_S("AAAA")], [400], both=False)
    case("minus_strand_only", ["T" * 7 + "CCGT" + "T" * 30], [acgg], [400])
    case("cover_ends_at_bit_31_and_32", ["C" * 28 + "ACGG" + C, "C" * 29 + "ACGG" + C], [acgg], [400])
    case("window_across_invalid_base", ["ACNGG" + "C" * 10 + "ACGG", "ACGN" + C], [acgg], [400])
    S5 = rng.integers(-300, 301, (5, 4)).astype(np.int32)
    lo, hi = score_range(S5)
    body = [rng.integers(1, 5, 70).astype(np.uint8) for _ in range(3)]
    body[1][20] = body[1][23] = body[1][50] = 0  # (bases 21 and 22 are valid and lie in no window of valid bases)
    case("threshold_above_every_score", body, [S5], [hi + 1])
    case("threshold_below_every_score", body, [S5], [lo])
    wide = [rng.integers(-300, 301, (64, 4)).astype(np.int32) for _ in range(3)]
    long_ = [rng.integers(1, 5, n).astype(np.uint8) for n in (64, 65, 100, 130)]
    long_[3][10] = 0
    case("three_groups_cover_one_base", long_, wide, [score_range(S)[0] for S in wide])
    return out


def pack_cases(W):
    """[(name, sequences, item_windows)]: the constructed inputs of tests/count_edges_model.py -- every stream alignment,
    runs cut by invalid bases, every legal cut of a run into items -- under their own item_windows, 64 and the default;
    a 70 000-base sequence (more windows than an item's 16-bit field holds); sequences that leave nothing; no sequence"""
    import count_edges_model as cem

    rng = np.random.default_rng(900 + W)
    out = []
    for cls in ("alignment", "runs_and_N", "item_lengths"):
        for part in cem.CLASSES[cls](W):
            seqs = [part["codes"][a:b] for a, b in zip(part["offs"][:-1], part["offs"][1:])]
            for M in sorted({part["M"], 64, 0}):
                out.append(("%s/%s/M=%d" % (cls, part["name"], M), seqs, M))
    long_ = rng.integers(1, 5, 70000).astype(np.uint8)
    cut = long_.copy()
    cut[[5, 6, 40000, 40002, 69999]] = 0
    for M in (64, 0, 65535):
        out.append(("long/M=%d" % M, [long_, cut, long_[:100]], M))
    nothing = [np.zeros(50, np.uint8), rng.integers(1, 5, W - 1).astype(np.uint8), np.zeros(0, np.uint8)]
    out.append(("nothing_stored", nothing, 0))
    out.append(("nothing_between", [long_[:40]] + nothing + [long_[:33]], 64))
    out.append(("no_sequence", [], 0))
    return out
