"""Pure-Python / numpy restatement of the dinucleotide-preserving shuffle (include/pengk.h, pengk_shuffle_sequences;
DESIGN.md 16): the doublet counts over the letters 0..4 (4 = not A/C/G/T), the last-edge tree by Wilson's loop-erased
walk, the walk that draws every letter's outgoing edges without replacement, all from counter-based splitmix64 draws.
Integer arithmetic only, so the device must agree with it bit for bit.  pack / unpack go to and from the scan layout."""
import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def mix64(x):
    """splitmix64 finalizer on a Python int (mod 2^64)"""
    x &= M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def draw(seed, g, c):
    return mix64(seed + GOLDEN * ((g << 32) + c)) >> 32


def walk_draws(seed, g, L):
    """draw(p) for p = 0 .. L-1 at once (numpy uint64, wrapping)"""
    with np.errstate(over="ignore"):
        x = np.uint64(seed & M64) + np.uint64(GOLDEN) * (np.uint64((g << 32) & M64) + np.arange(L, dtype=np.uint64))
        x = x ^ (x >> np.uint64(30))
        x = x * np.uint64(0xBF58476D1CE4E5B9)
        x = x ^ (x >> np.uint64(27))
        x = x * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return (x >> np.uint64(32)).tolist()


def shuffle(s, seed, g, stats=None):
    """the shuffle of the letters s (0..4) of the sequence with global index g; stats (a dict), if given, receives
    the number of tree draws and the counters left at the end"""
    s = [int(x) for x in s]
    L = len(s)
    if L == 0:
        return []
    cnt = [[0] * 5 for _ in range(5)]
    for p in range(L - 1):
        cnt[s[p]][s[p + 1]] += 1
    out = [sum(r) for r in cnt]
    f = s[L - 1]

    def sel(u, k):
        for v in range(5):
            if k < cnt[u][v]:
                return v
            k -= cnt[u][v]
        raise AssertionError("sel beyond the row")

    in_tree = [False] * 5
    in_tree[f] = True
    nxt = [0] * 5
    t = 0
    for u0 in range(5):
        if out[u0] == 0 or in_tree[u0]:
            continue
        u = u0
        while not in_tree[u]:
            v = sel(u, (draw(seed, g, (1 << 31) + t) * out[u]) >> 32)
            t += 1
            nxt[u] = v
            u = v
        u = u0
        while not in_tree[u]:
            in_tree[u] = True
            u = nxt[u]
    rem = out[:]
    for u in range(5):
        if u != f and out[u] > 0:
            cnt[u][nxt[u]] -= 1
            rem[u] -= 1
    r = walk_draws(seed, g, L)
    o = [s[0]]
    u = s[0]
    for p in range(1, L):
        if rem[u] > 0:
            v = sel(u, (r[p] * rem[u]) >> 32)
            cnt[u][v] -= 1
            rem[u] -= 1
        else:
            v = nxt[u]
        o.append(v)
        u = v
    if stats is not None:
        stats["tree_draws"] = t
        stats["rem"] = rem
        stats["cnt"] = cnt
    return o


def doublets(s):
    """the 25 doublet counts of the letters s, as a 5 x 5 array"""
    s = np.asarray(s, np.int64)
    c = np.zeros((5, 5), np.int64)
    if len(s) > 1:
        np.add.at(c, (s[:-1], s[1:]), 1)
    return c


def pack(seqs):
    """letters 0..4 of every sequence -> (words, valid, offs, lens) of the scan layout: every sequence from a 32-base
    boundary, code 0 and validity 0 where the letter is 4, zero bits beyond a sequence's end"""
    lens = np.array([len(s) for s in seqs], np.uint32)
    nw = (lens.astype(np.int64) + 31) // 32
    w0 = np.concatenate([[0], np.cumsum(nw)]).astype(np.int64)
    words = np.zeros(max(int(w0[-1]), 1), np.uint64)
    valid = np.zeros(max(int(w0[-1]), 1), np.uint32)
    for i, s in enumerate(seqs):
        s = np.asarray(s, np.uint64)
        if len(s) == 0:
            continue
        p = np.arange(len(s))
        ok = s < 4
        j = int(w0[i]) + (p >> 5)
        np.bitwise_or.at(words, j, np.where(ok, s, 0).astype(np.uint64) << (2 * (p & 31)).astype(np.uint64))
        np.bitwise_or.at(valid, j, (ok.astype(np.uint32) << (p & 31).astype(np.uint32)).astype(np.uint32))
    offs = (w0[:-1] * 32).astype(np.int64)
    return words, valid, (offs if len(seqs) else np.zeros(1, np.int64)), (lens if len(seqs) else np.zeros(1, np.uint32))


def unpack(words, valid, offs, lens):
    """the letters 0..4 of every sequence of a scan layout (valid = None: every base valid)"""
    out = []
    for o, L in zip(offs, lens):
        g = int(o) + np.arange(int(L))
        b = ((words[g >> 5] >> (2 * (g & 31)).astype(np.uint64)) & np.uint64(3)).astype(np.uint8)
        if valid is not None:
            ok = (valid[g >> 5] >> (g & 31).astype(np.uint32)) & np.uint32(1)
            b = np.where(ok == 1, b, 4).astype(np.uint8)
        out.append(b)
    return out


def shuffle_layout(words, valid, offs, lens, n_seq, seed, seq0):
    """(words, valid) the device must write for the first n_seq sequences of a scan layout"""
    seqs = unpack(words, valid, offs[:n_seq], lens[:n_seq])
    w, v, _, _ = pack([shuffle(s, seed, seq0 + i) for i, s in enumerate(seqs)])
    return w, v
