"""Constructed inputs for the count kernels of csrc/count.hip at their item, repeat and offset edges, and the plain
references they are compared with (tests/test_count_edges_cpu.py, tests/test_gpu_count_edges.py).  No device here.

References
  sparse_count     the reference's count rule on byte codes and offsets without a 4^W table: per visited run, left to
                   right, a window is counted iff its (canonical) id was not counted at a start position less than W
                   back.  {id: count} over canonical ids only, and ltot.
  deferral_model   which continuing items the scan hands to the exact fallback, from the packed stream and the items
                   alone: the rule of DESIGN.md 2 ("replay a prologue of ceil16(3W-3) bases with an empty ring; if none
                   of its windows is suppressed the ring is the true one, otherwise the item goes on a defer list", as
                   does an item closer to the head of its run than the replay reaches).
  fixup_model      where the fallback's backward search ends for one item: "certified once 2(W-1) consecutive windows
                   were not suppressed, or the replay started at the head of the run; otherwise quadruple `back`".
  resplit          other legal item lists for the same stream.

Codes are the oracle's: 0 invalid, 1..4 = A C G T; ids are little-endian base 4 (first base in the low digits).

What the classes hold, as sequences / packer's items / items deferral_model predicts deferred (plus strand + both):
  W   item_lengths  alignment     periods       prologue_edge     long_fixup         runs_and_N
  2   62/86/20+20   832/960/72+72 22/73/6+6     52/364/29+29      3/939/936+936      32/43/1+1
  4   62/86/12+14   832/960/10+28 28/94/30+45   104/728/58+61     6/1878/1872+1872   32/43/1+1
  6   62/86/12+13   832/960/1+6   32/108/50+55  104/728/46+46     6/1878/1872+1872   32/43/0+0
  8   62/86/12+13   832/960/0+3   36/122/60+67  168/1176/78+79    6/1878/1872+1872   32/43/0+0
  10  62/86/12+12   832/960/0+0   40/136/70+76  168/1176/78+78    6/1878/1872+1872   32/43/0+0
  12  62/86/12+12   832/960/0+0   44/150/80+87  232/1624/150+150  6/1878/1872+1872   32/43/0+0
  14  62/86/12+12   832/960/0+0   48/164/90+95  232/1624/148+148  6/1878/1872+1872   32/43/0+0
"""
import functools

import numpy as np

import peng_motif_amd as pk

WS_MASK = (1 << 40) - 1
NW_MAX = 65535
WS = (2, 4, 6, 8, 10, 12)


def prologue_bases(W):
    return ((3 * W - 3 + 15) // 16) * 16


# ---- sequences ---------------------------------------------------------------------------------------------------------
def seq(s):
    return np.array(["NACGT".index(c) for c in s], np.uint8)


def rand(rng, n):
    return rng.integers(1, 5, size=n).astype(np.uint8)


def revcomp_codes(s):
    return (5 - s[::-1]).astype(np.uint8)


def tile(unit, n):
    return np.resize(unit, n).astype(np.uint8)


def join(seqs):
    offs = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    codes = np.concatenate(seqs).astype(np.uint8) if seqs else np.zeros(0, np.uint8)
    return codes, offs


def window_ids(b2, W):
    """(plus, canonical) ids of the windows starting at 0 .. len - W of an array of 2-bit bases"""
    n = len(b2) - W + 1
    if n <= 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    b2 = b2.astype(np.int64)
    plus = np.zeros(n, np.int64)
    rc = np.zeros(n, np.int64)
    for q in range(W):
        plus |= b2[q:q + n] << (2 * q)
        rc |= (3 - b2[q:q + n]) << (2 * (W - 1 - q))
    return plus, np.minimum(plus, rc)


def primitive(unit):
    p = len(unit)
    return not any(p % q == 0 and np.array_equal(tile(unit[:q], p), unit) for q in range(1, p))


def clean_random(rng, n, W):
    """n random bases in which no window equals, on either strand, one of the W - 1 windows in front of it: nothing is
    suppressed in such a stretch in either strand mode"""
    out, plus, canon = [], [], []
    mask = (1 << (2 * W)) - 1
    x = r = 0
    for i in range(n):
        for c in rng.permutation(4).tolist():
            nx, nr = (x >> 2) | (c << (2 * (W - 1))), ((r << 2) & mask) | (3 - c)
            if i < W - 1 or (nx not in plus[-(W - 1):] and min(nx, nr) not in canon[-(W - 1):]):
                break
        else:
            raise ValueError("no clean continuation")
        x, r = nx, nr
        out.append(c + 1)
        if i >= W - 1:
            plus.append(x)
            canon.append(min(x, r))
    return np.array(out, np.uint8)


# ---- the count rule ------------------------------------------------------------------------------------------------------
def visited_runs(codes, offs, W):
    """the reference's scan rule (src/base_pattern.cpp:347-381): at i, W valid bases in a row start a run, which is
    visited window by window until the base to the right of the window is invalid (index q) or the sequence ends, and
    the scan resumes at q + 2; a shorter stretch is left at the invalid base and the scan resumes right behind it.
    -> (start, windows) arrays, starts absolute in codes"""
    starts, wins = [], []
    bad = np.flatnonzero(np.asarray(codes) == 0)
    for s in range(len(offs) - 1):
        a, e = int(offs[s]), int(offs[s + 1])
        k = int(np.searchsorted(bad, a))
        i = a
        while i < e:
            while k < len(bad) and bad[k] < i:
                k += 1
            stop = int(bad[k]) if k < len(bad) and bad[k] < e else e
            if stop - i >= W:
                starts.append(i)
                wins.append(stop - i - W + 1)
                i = stop + 2
            else:
                i = stop + 1
    return np.array(starts, np.int64), np.array(wins, np.int64)


def _ranges(starts, lens):
    """concatenated aranges start .. start + len - 1, and the index of the range each element comes from"""
    lens = np.asarray(lens, np.int64)
    tot = int(lens.sum())
    which = np.repeat(np.arange(len(lens)), lens)
    first = np.repeat(np.cumsum(lens) - lens, lens)
    return np.repeat(np.asarray(starts, np.int64), lens) + (np.arange(tot) - first), which


def kept_mask(ids, W, run=None):
    """the non-overlap rule: window t is counted iff none of the windows t-1 .. t-(W-1) of its run that were counted has
    its id.  ids: window ids in scan order; run: the run every window belongs to (None = one run)."""
    n = len(ids)
    kept = np.ones(n, bool)
    if run is None:
        run = np.zeros(n, np.int64)
    cand = np.zeros(n, bool)
    for d in range(1, min(W, n)):
        cand[d:] |= (ids[d:] == ids[:-d]) & (run[d:] == run[:-d])
    todo = np.flatnonzero(cand)
    if todo.size:
        idl, runl, k = ids.tolist(), run.tolist(), kept.tolist()
        for t in todo.tolist():
            x, r = idl[t], runl[t]
            for j in range(t - 1, max(t - W, -1), -1):
                if runl[j] != r:
                    break
                if k[j] and idl[j] == x:
                    k[t] = False
                    break
        kept = np.array(k, bool)
    return kept


def sparse_count_arrays(codes, offs, W, both):
    """-> (ids ascending, their counts, ltot, kept mask, window starts, run of every window)"""
    starts, wins = visited_runs(codes, offs, W)
    pos, run = _ranges(starts, wins)
    plus, canon = window_ids(np.clip(np.asarray(codes).astype(np.int64) - 1, 0, 3), W)
    ids = (canon if both else plus)[pos] if pos.size else np.zeros(0, np.int64)
    kept = kept_mask(ids, W, run)
    u, c = np.unique(ids[kept], return_counts=True)
    return u, c.astype(np.int64), int(wins.sum()), kept, pos, run


def sparse_count(codes, offs, W, both):
    """{id: count} (canonical ids only under both strands) and ltot"""
    u, c, ltot = sparse_count_arrays(codes, offs, W, both)[:3]
    return dict(zip(u.tolist(), c.tolist())), ltot


def revcomp_ids(x, W):
    x = np.asarray(x, np.int64)
    r = np.zeros_like(x)
    for q in range(W):
        r |= (3 - ((x >> (2 * q)) & 3)) << (2 * (W - 1 - q))
    return r


def dense(sparse, W, mirrored):
    """a sparse count as the 4^W table (W <= 12), mirrored on the host like pengk_mirror_counts does on the device"""
    out = np.zeros(4 ** W, np.uint64)
    x = np.fromiter(sparse.keys(), np.int64, len(sparse))
    c = np.fromiter(sparse.values(), np.uint64, len(sparse))
    out[x] = c
    if mirrored:
        out[revcomp_ids(x, W)] = c
    return out


# ---- the packed stream ---------------------------------------------------------------------------------------------------
def item_fields(items):
    it = np.asarray(items, np.uint64)
    return ((it & np.uint64(WS_MASK)).astype(np.int64), ((it >> np.uint64(40)) & np.uint64(0xFFFF)).astype(np.int64),
            ((it >> np.uint64(56)) & np.uint64(1)).astype(np.int64))


def make_items(ws, nw, cont):
    return (np.asarray(ws, np.uint64) | (np.asarray(nw, np.uint64) << np.uint64(40)) | (np.asarray(cont, np.uint64) << np.uint64(56)))


def stream_bases(words):
    w = np.asarray(words, np.uint64)
    return ((w[:, None] >> (np.uint64(2) * np.arange(32, dtype=np.uint64))[None, :]) & np.uint64(3)).astype(np.int64).reshape(-1)


def item_runs(items):
    """(stream offset of the first window, windows) of every run of an item list"""
    ws, nw, cont = item_fields(items)
    heads = np.flatnonzero(cont == 0)
    if not heads.size:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return ws[heads], np.add.reduceat(nw, heads)


def replay_windows(items):
    """the stream offset and the run of every window an item list visits, in order; an item that continues a run must
    begin where the item in front of it ended"""
    ws, nw, cont = item_fields(items)
    assert not len(ws) or cont[0] == 0
    assert np.all((nw >= 1) & (nw <= NW_MAX))
    c = np.flatnonzero(cont == 1)
    assert np.array_equal(ws[c], ws[c - 1] + nw[c - 1]), "a continuing item does not continue"
    pos, which = _ranges(ws, nw)
    return pos, (np.cumsum(cont == 0) - 1)[which]


def replay_count(words, items, W, both):
    """the count the items stand for: {id: count}, ltot"""
    pos, run = replay_windows(items)
    plus, canon = window_ids(stream_bases(words), W)
    ids = (canon if both else plus)[pos] if pos.size else np.zeros(0, np.int64)
    u, c = np.unique(ids[kept_mask(ids, W, run)], return_counts=True)
    return dict(zip(u.tolist(), c.tolist())), len(pos)


def deferral_model(words, items, W, both):
    """bool per item: the scan cannot certify its ring.  A continuing item replays, from an empty ring, the P - W + 1
    windows that end on the P - W + 1 bases in front of its first window's last base (they start at ws - (P - W + 1) ..
    ws - 1, whatever the stream holds there); a replayed window is kept unless one of the kept replayed windows of the
    W - 1 positions in front of it has its id.  The item defers iff a replayed window is not kept -- or if its run has
    fewer than P - W + 1 windows in front of it: the replay would reach in front of the run."""
    ws, nw, cont = item_fields(items)
    out = np.zeros(len(ws), bool)
    idx = np.flatnonzero(cont == 1)
    if not idx.size:
        return out
    n = prologue_bases(W) - W + 1
    plus, canon = window_ids(stream_bases(words), W)
    ids = (canon if both else plus)[ws[idx][:, None] - n + np.arange(n)[None, :]]
    kept = np.ones(ids.shape, bool)
    for t in range(1, n):
        hit = np.zeros(len(idx), bool)
        for d in range(1, min(W - 1, t) + 1):
            hit |= kept[:, t - d] & (ids[:, t - d] == ids[:, t])
        kept[:, t] = ~hit
    head_ws = ws[np.flatnonzero(cont == 0)][np.cumsum(cont == 0) - 1]  # first window of every item's run
    out[idx] = ~kept.all(axis=1) | (ws[idx] - head_ws[idx] < n)
    return out


def fixup_model(words, items, it, W, both):
    """the fallback's search for item `it`: replay from `back` windows in front of it with an empty ring, back = 8(W-1),
    then four times as far each time; the start is good once 2(W-1) windows in a row were not suppressed in front of the
    item, or when it is the head of the run.  -> dict(back, at_head, max_clean: the longest such row of the last replay,
    levels: (back, max_clean) of every replay)"""
    ws, nw, cont = item_fields(items)
    j = it
    while cont[j]:
        j -= 1
    head = int(ws[j])
    plus, canon = window_ids(stream_bases(words), W)
    ids = canon if both else plus
    back, levels = 8 * (W - 1), []
    while True:
        p0 = int(ws[it]) - back if int(ws[it]) - head > back else head
        kept = kept_mask(ids[p0:int(ws[it])], W)
        best = cur = 0
        for k in kept.tolist():
            cur = cur + 1 if k else 0
            best = max(best, cur)
        levels.append((back, best))
        if p0 == head or best >= 2 * (W - 1):
            return dict(back=back, at_head=p0 == head, max_clean=best, levels=levels)
        back *= 4


def resplit(items, cut=None, seed=None):
    """another legal item list for the same runs: pieces of `cut` windows (None, no seed: every run whole, in pieces of
    65535 where it is longer), or cut at seeded random positions"""
    rws, rnw = item_runs(items)
    rng = np.random.default_rng(seed) if seed is not None else None
    ws_out, nw_out, cont_out = [], [], []
    for w0, n in zip(rws.tolist(), rnw.tolist()):
        if rng is not None:
            k = int(rng.integers(0, min(n - 1, 6) + 1))
            cuts = np.unique(rng.integers(1, n, size=k)) if k else np.zeros(0, np.int64)
            edges = np.concatenate([[0], cuts, [n]]).astype(np.int64)
            edges = np.unique(np.concatenate([edges] + [np.arange(a, b, NW_MAX) for a, b in zip(edges[:-1], edges[1:])]))
        else:
            edges = np.append(np.arange(0, n, cut or NW_MAX), n).astype(np.int64)
        ws_out.append(w0 + edges[:-1])
        nw_out.append(np.diff(edges))
        c = np.ones(len(edges) - 1, np.int64)
        c[0] = 0
        cont_out.append(c)
    if not ws_out:
        return np.zeros(0, np.uint64)
    return make_items(np.concatenate(ws_out), np.concatenate(nw_out), np.concatenate(cont_out))


def resplits(items):
    """(name, items) of every re-split the tests attach"""
    out = [("whole", resplit(items))] + [("every %d" % c, resplit(items, cut=c)) for c in (1, 15, 16, 17)]
    return out + [("random %d" % s, resplit(items, seed=s)) for s in (1, 2)]


# ---- case classes --------------------------------------------------------------------------------------------------------
# A class is a list of parts; a part is a dict: name, codes, offs, M (the packer's item_windows) and what the CPU test
# needs to certify it.
LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33)


def _part(name, seqs, M, **meta):
    codes, offs = join(seqs)
    return dict(name=name, codes=codes, offs=offs, M=M, **meta)


def _with_repeat_on_cuts(s, W, M):
    """a copy of s with a short tandem repeat laid across every item boundary (window k M starts at base k M)"""
    s = s.copy()
    unit = seq("A") if W == 2 else seq("AC")
    n = len(s) - W + 1
    cuts = list(range(M, n, M)) or [len(s) // 2]
    for c in cuts:
        a, e = max(c - 2 * W, 0), min(c + 2 * W, len(s))
        s[a:e] = tile(unit, e - a)
    return s


@functools.lru_cache(None)
def item_lengths(W):
    rng = np.random.default_rng(1000 + W)
    parts = []
    for M in (64, 256):
        want = LENGTHS + (M - 1, M, M + 1, 2 * M, 2 * M + 1)
        seqs = [rand(rng, n + W - 1) for n in want]
        seqs += [_with_repeat_on_cuts(s, W, M) for s in seqs]
        parts.append(_part("item_lengths M=%d" % M, seqs, M, windows=want * 2))
    want = (65534, 65535, 65536, 65537, 140000)
    seqs = [rand(rng, n + W - 1) for n in want]
    seqs += [_with_repeat_on_cuts(s, W, NW_MAX) for s in seqs]
    parts.append(_part("item_lengths M=65535", seqs, NW_MAX, windows=want * 2))
    return parts


@functools.lru_cache(None)
def alignment(W):
    """every run length at every residue of the stream word: in front of each target sequence goes the one prefix
    sequence of 10 .. 41 bases that puts its first base on the residue wanted (W .. W + 31 bases above W = 10: a
    sequence shorter than W leaves nothing in the stream)"""
    rng = np.random.default_rng(2000 + W)
    seqs, targets = [], []
    cur, lo = pk.FRONT_PAD_BASES, max(10, W)
    for n in LENGTHS + (63, 64, 65, 128, 129):
        for res in rng.permutation(32).tolist():  # (in random order, so that the prefixes take every length)
            p = lo + (res - cur - lo) % 32
            seqs.append(rand(rng, p))
            cur += p
            seqs.append(rand(rng, n + W - 1))
            targets.append((n, cur))  # windows, stream offset of the target's first base
            cur += n + W - 1
    return [_part("alignment", seqs, 64, targets=targets)]


def _selfrc(rng, n):
    """n bases whose even-length core equals its own reverse complement.  (No word of odd length does: its middle base
    would be its own complement.  For odd n the core has n - 1 bases and one random base follows.)"""
    h = rand(rng, n // 2)
    core = np.concatenate([h, revcomp_codes(h)])
    return core if n % 2 == 0 else np.concatenate([core, rand(rng, 1)])


def _suppressed_plus(s, W):
    return int((~sparse_count_arrays(s, np.array([0, len(s)], np.int64), W, False)[3]).sum())


@functools.lru_cache(None)
def periods(W):
    rng = np.random.default_rng(3000 + W)
    R = max(6 * W, 160)  # at M = 64 every copy spans several items
    seqs, alone = [], []

    def add(unit, kind, p):
        rep = tile(unit, R)
        seqs.append(np.concatenate([rand(rng, 40), rep, rand(rng, 40)]))
        alone.append((len(seqs), kind, p))
        seqs.append(rep)

    for p in range(1, W + 3):
        while True:  # a unit whose repeat behaves as its period says on the plus strand, by the reference
            unit = rand(rng, p)
            if primitive(unit) and (_suppressed_plus(tile(unit, R), W) > 0) == (p < W):
                break
        add(unit, "random", p)
    for u in ("AT", "CG", "ACGT", "AATT"):
        add(seq(u), "rc-periodic " + u, len(u))
    for n in (W - 1, W, W + 1):
        if n >= 2:
            while True:
                unit = _selfrc(rng, n)
                if primitive(unit):
                    break
            add(unit, "self-rc core, %d bases" % n, n)
    arm = rand(rng, 2 * W)
    hair = np.concatenate([arm, seq("ACGT"), revcomp_codes(arm)])  # (the loop is its own reverse complement)
    seqs.append(np.concatenate([rand(rng, 40), hair, rand(rng, 40)]))
    seqs.append(hair)
    return [_part("periods", seqs, 64, alone=alone)]


def _last_suppressed(s, W):
    bad = np.flatnonzero(~sparse_count_arrays(s, np.array([0, len(s)], np.int64), W, False)[3])
    return int(bad[-1]) if bad.size else -1


@functools.lru_cache(None)
def prologue_edge(W):
    """one clean 400-base sequence with a repeat of period < W laid over it, M = 64.  `exact`: (sequence, boundary
    window B, o): on the plus strand the last suppressed window of the sequence starts at F + o, F = B - (P - W + 1) the
    first window item B / 64 replays, o = -1 outside, 0 at, +1 inside.  `shifted`: the repeat moved base by base over
    2P + 2 positions, its last whole window from B - P - 1 to B + P."""
    rng = np.random.default_rng(4000 + W)
    L, P = 400, prologue_bases(W)
    base = clean_random(rng, L, W)
    RL = 3 * W
    units = [rand(rng, 1)]
    while W >= 4 and len(units) < 2:
        u = rand(rng, W - 1)
        if primitive(u):
            units.append(u)
    seqs, exact, shifted, spans = [], [], [], []
    for ui, unit in enumerate(units):
        first = len(seqs)
        rep = tile(unit, RL)

        def laid(a):
            s = base.copy()
            s[a:a + RL] = rep
            # the flanks must not prolong the repeat (nor, with the base put there instead, begin a run of their own)
            if a + RL < L and s[a + RL] == unit[RL % len(unit)]:
                s[a + RL] = next(c for c in (1, 2, 3, 4) if c != s[a + RL] and (a + RL + 1 >= L or c != s[a + RL + 1]))
            if a > 0 and s[a - 1] == unit[-1]:
                s[a - 1] = next(c for c in (1, 2, 3, 4) if c != s[a - 1] and (a < 2 or c != s[a - 2]))
            return s

        for B in range(64, L - W + 1, 64):
            F = B - (P - W + 1)
            for o in (-1, 0, 1):
                a, got = F + o - (RL - W), None
                for _ in range(8):
                    if not 0 <= a <= L - RL:
                        got = None
                        break
                    got = _last_suppressed(laid(a), W)
                    if got == F + o:
                        break
                    a += F + o - got
                if got != F + o:
                    raise ValueError("no placement puts the last suppressed window on %d" % (F + o))
                exact.append((len(seqs), B, o))
                seqs.append(laid(a))
        B = 128
        for j in range(2 * P + 2):
            a = B - P - 1 - (RL - W) + j
            if 0 <= a:
                shifted.append(len(seqs))
                seqs.append(laid(a))
        spans.append((first, len(seqs)))
    return [_part("prologue_edge", seqs, 64, exact=exact, shifted=shifted, repeats=spans)]


FIXUP_BOUNDARY = 64 * 32  # the item boundary (a window index) the clean stretch lies 100 windows in front of


def _cert_item(p):
    ws = item_fields(p.items)[0]
    return int(np.flatnonzero(ws == pk.FRONT_PAD_BASES + FIXUP_BOUNDARY)[0])


@functools.lru_cache(None)
def long_fixup(W):
    """20 000-base repeats at M = 64: every item behind the first is deferred and its fix-up walks back to the head.
    `cert`: (failing sequence, succeeding sequence) per repeat -- the same repeat with a clean stretch that ends 100
    windows in front of item 32: in the failing one the fix-up of item 32 never sees more than 2(W-1) - 1 clean windows
    in a row and walks on to the head, in the succeeding one it sees exactly 2(W-1) and stops (fixup_model, both strand
    modes).  `clean`: the two figures reached; a homopolymer at W = 2 and a period-3 repeat at W = 4 cannot hit them
    (one foreign base already makes three, respectively seven, clean windows) and get the nearest on either side.
    The pair pins the table at these two inputs, not where the kernel chooses to certify: the clean stretch empties the
    ring of every repeat window, so a fix-up that certifies there and one that walks on to the head count the same
    ids, and only fixup_model tells the two apart.  A fix-up that certifies too early shows on `periods`, where the
    clean windows in front of an item are not followed by 100 windows that rebuild the true ring."""
    rng = np.random.default_rng(5000 + W)
    L = 20000
    units = [rand(rng, 1)]
    while W >= 4 and len(units) < 2:
        u = rand(rng, 3)
        if primitive(u):
            units.append(u)
    seqs = [tile(u, L) for u in units]
    cert, clean = [], []
    e = FIXUP_BOUNDARY - 100
    for u in units:
        def verdicts(s):
            p = pk.Packed(s, np.array([0, L], np.int64), W, 64)
            return [fixup_model(p.words, p.items, _cert_item(p), W, both) for both in (False, True)]

        bar, bad, good = 2 * (W - 1), (-1, None), (1 << 30, None)
        for _ in range(300):  # the stretches that miss and reach the bar most narrowly, the same way on both strands
            stretch = clean_random(rng, 4 * W, W)
            for c in range(1, len(stretch) + 1):
                s = tile(u, L)
                s[e - c:e] = stretch[len(stretch) - c:]
                v = verdicts(s)
                if all(x["at_head"] for x in v):
                    k = {max(k for _, k in x["levels"][:-1]) for x in v}
                    if len(k) == 1 and bad[0] < min(k) < bar:
                        bad = (min(k), s)
                elif not any(x["at_head"] for x in v):
                    k = {x["max_clean"] for x in v}
                    if len(k) == 1 and bar <= min(k) < good[0]:
                        good = (min(k), s)
                    break
            if bad[0] == bar - 1 and good[0] == bar:
                break
        clean.append((bad[0], good[0]))
        bad, good = bad[1], good[1]
        cert.append((len(seqs), len(seqs) + 1))
        seqs += [bad, good]
    return [_part("long_fixup", seqs, 64, cert=cert, clean=clean)]


def expect_runs(raw, W):
    """visited run lengths of valid stretches of `raw` bases separated by one invalid base each: the base behind the
    invalid base that ended a visited run is skipped"""
    out, skip = [], False
    for r in raw:
        eff = max(r - skip, 0)
        skip = eff >= W
        if skip:
            out.append(eff)
    return out


@functools.lru_cache(None)
def runs_and_N(W):
    rng = np.random.default_rng(6000 + W)
    seqs, runs = [], []

    def add(effective):
        """stretches that leave visited runs of these lengths (0 = two invalid bases in a row)"""
        raw, skip = [], False
        for e in effective:
            raw.append(e + (1 if skip and e > 0 else 0))
            skip = e >= W
        parts = []
        for k, r in enumerate(raw):
            parts += [rand(rng, r)] + ([np.zeros(1, np.uint8)] if k + 1 < len(raw) else [])
        seqs.append(np.concatenate(parts))
        runs.append([e for e in effective if e >= W])
        assert expect_runs(raw, W) == runs[-1]

    for n in (W - 1, W, W + 1):
        add([n, 40])            # at the head
        add([40, n])            # at the end, behind a visited run (one base skipped)
        add([W - 2, n])         # at the end, behind a stretch too short to visit (nothing skipped)
        add([40, n, 40])        # in the middle
        add([n, n, n])
        add([0, n])             # the sequence begins with an invalid base
        add([n, 0])             # ... ends with one
        add([40, 0, n])         # two invalid bases in a row: the skipped base is the second of them
        add([n])                # whole sequences of W-1, W, W+1 bases
    add([150, 150])             # runs of several items
    none = [rand(rng, W - 1), np.zeros(20, np.uint8), np.concatenate([rand(rng, W - 1), np.zeros(1, np.uint8), rand(rng, W - 1)]),
            rand(rng, 1)]
    return [_part("runs_and_N", seqs, 64, runs=runs), _part("runs_and_N no window", none, 64, runs=[[] for _ in none])]


CLASSES = dict(item_lengths=item_lengths, alignment=alignment, periods=periods, prologue_edge=prologue_edge,
               long_fixup=long_fixup, runs_and_N=runs_and_N)


def case_tag(cls, part, W, both):
    """the unique name of a part under a strand mode (the key of its entry in tests/golden/edges_count_w*.npz)"""
    return "%s/%s/W%d/%s" % (cls, part["name"], W, "both" if both else "plus")


@functools.lru_cache(None)
def packed(cls, W):
    """the parts of a class as the host packer packs them"""
    return [pk.Packed(p["codes"], p["offs"], W, p["M"]) for p in CLASSES[cls](W)]


def everything(W):
    """all classes as one input (the W = 14 comparison)"""
    seqs = []
    for f in CLASSES.values():
        for part in f(W):
            seqs += [part["codes"][a:b] for a, b in zip(part["offs"][:-1], part["offs"][1:])]
    return join(seqs)
