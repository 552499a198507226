"""numpy restatement of the sequence-scan kernels, vectorised over sequences of one length, for sets too large for the
per-sequence models (motif_score_model, motif_sites_model, motif_centrality_model, motif_refine_model).  It adds no
semantics of its own: include/pengk.h is the specification, those four models are the restatement it must agree with
array for array (tests/test_scan_batch_model_cpu.py), and it exists so that a million sequences can be compared value by
value (tests/test_gpu_scan_scale.py).

Input: an (n, L) uint8 code array (0 = invalid, 1..4 = A, C, G, T) and one motif S (w x 4 integer log-odds).  From the
window scores of both strands and their validity mask come, without a Python loop over sequences: the best score, the
site counts and records, the best site under the keyed tie-break, and the site-profile counts.  A mixed-length set
(flat codes + offsets) is handled one length class at a time and scattered back to the set's order.

Memory: sequences are taken CHUNK_CELLS bases at a time (n_chunk = CHUNK_CELLS / L sequences).  A chunk holds the base
indices (8 bytes per base), the scores of both strands (2 x 4), one gathered column (4), the validity sums (4 + 1) and,
in the tie-break, the keys of both strands with a few temporaries (< 2 x 8 x 5): below 128 bytes per base, 256 MiB at
the default CHUNK_CELLS = 2^21, plus the outputs themselves (per sequence, and per record)."""
import numpy as np

from motif_score_model import GOLDEN, SENTINEL, mix64, revcomp_S

CHUNK_CELLS = 1 << 21
MAX_MOTIF_LEN = 64
SITES = np.dtype([("seq", np.int64), ("pos", np.uint32), ("strand", np.uint8), ("score", np.int32)])
ALL_SITES = np.dtype([("motif", np.int64), ("seq", np.uint64), ("pos", np.uint32), ("strand", np.uint8), ("score", np.int32)])


def window_scores(codes, S, both):
    """(sc, good): sc[k, i, p] (int32) the score of window p of sequence i on strand k (0 = +, 1 = - with `both`), whatever
    its bases; good[i, p]: every base of the window is A/C/G/T.  L - w + 1 windows, none when L < w."""
    codes = np.asarray(codes, np.uint8)
    n, L = codes.shape
    S = np.asarray(S, np.int32)
    w = S.shape[0]
    ns = 2 if both else 1
    nwin = max(L - w + 1, 0)
    sc = np.zeros((ns, n, nwin), np.int32)
    if nwin == 0 or n == 0:
        return sc, np.zeros((n, nwin), bool)
    ok = (codes >= 1) & (codes <= 4)
    bad = np.zeros((n, L + 1), np.int32)
    np.cumsum(~ok, axis=1, out=bad[:, 1:])
    good = (bad[:, w:] - bad[:, :nwin]) == 0
    b = np.where(ok, codes, 1).astype(np.intp) - 1
    for k, M in enumerate([S, revcomp_S(S)][:ns]):
        for j in range(w):
            sc[k] += np.take(M[j], b[:, j:j + nwin])
    return sc, good


def _best_site(sc, good, m, g):
    """(best int32, site uint64) of one chunk; g: the sequences' global indices (uint64)"""
    ns, n, nwin = sc.shape
    best = np.full(n, SENTINEL, np.int32)
    site = np.zeros(n, np.uint64)
    if nwin == 0 or n == 0:
        return best, site
    has = good.any(axis=1)
    top = np.where(good[None], sc, SENTINEL).max(axis=(0, 2))
    # the window strands in the order of 2p + s: (p, s) row-major
    tied = np.ascontiguousarray((good[None] & (sc == top[None, :, None])).transpose(1, 2, 0)).reshape(n, nwin * ns)
    cand = np.arange(nwin * ns, dtype=np.uint64) * np.uint64(1 if ns == 2 else 2)
    first = tied.argmax(axis=1)
    many = np.nonzero(tied.sum(axis=1) > 1)[0]
    if len(many):  # the largest key; an equal key: the smaller 2p + s (argmax takes the first)
        T = tied[many]
        with np.errstate(over="ignore"):
            h = mix64((np.uint64(GOLDEN) * (g[many] + np.uint64(1))) ^ np.uint64(m))
        key = mix64(h[:, None] ^ cand[None, :])
        key[~T] = 0
        first[many] = (T & (key == key.max(axis=1)[:, None])).argmax(axis=1)
    best[has] = top[has]
    site[has] = cand[first[has]]
    return best, site


def _sites(sc, good, t):
    """(counts, records) of one chunk; the records in the order sequence, position, + before -"""
    ns, n, nwin = sc.shape
    hit = np.empty((n, nwin, ns), bool)
    for k in range(ns):
        hit[:, :, k] = good & (sc[k] >= t)
    i, p, s = np.nonzero(hit)
    rec = np.zeros(len(i), SITES)
    rec["seq"], rec["pos"], rec["strand"], rec["score"] = i, p, s, sc[s, i, p]
    return hit.reshape(n, -1).sum(axis=1, dtype=np.int64), rec


def scan(codes, S, both, thr=None, m=None, seq0=0, index=None):
    """everything about one motif on one equal-length set in one pass over its window scores, a dict:
      best       int64 (n): the best window score (SENTINEL without a valid window), as motif_score_model.best_scores
      best_plus  the same on the + strand alone
      counts, sites   (thr given) int64 (n) and a SITES array: the window strands with score >= thr, as
                 motif_sites_model.sites (sequence, position, + before -); seq = the row of codes
      best_site, site (m given) int32 / uint64 (n), as motif_centrality_model.best_sites; sequence i has the global
                 index seq0 + index[i] (index: its place in the whole set, default i)"""
    codes = np.asarray(codes, np.uint8)
    n, L = codes.shape
    out = {"best": np.full(n, SENTINEL, np.int64), "best_plus": np.full(n, SENTINEL, np.int64)}
    if thr is not None:
        out["counts"] = np.zeros(n, np.int64)
        recs = []
    if m is not None:
        out["best_site"] = np.full(n, SENTINEL, np.int32)
        out["site"] = np.zeros(n, np.uint64)
        g = np.uint64(seq0) + (np.arange(n, dtype=np.uint64) if index is None else np.asarray(index, np.uint64))
    step = max(1, CHUNK_CELLS // max(L, 1))
    for a in range(0, n, step):
        e = min(n, a + step)
        sc, good = window_scores(codes[a:e], S, both)
        if sc.shape[2]:
            out["best"][a:e] = np.where(good[None], sc, SENTINEL).max(axis=(0, 2))
            out["best_plus"][a:e] = np.where(good, sc[0], SENTINEL).max(axis=1)
        if thr is not None:
            out["counts"][a:e], r = _sites(sc, good, thr)
            r["seq"] += a
            recs.append(r)
        if m is not None:
            out["best_site"][a:e], out["site"][a:e] = _best_site(sc, good, m, g[a:e])
    if thr is not None:
        out["sites"] = np.concatenate(recs) if recs else np.zeros(0, SITES)
    return out


def best_scores(codes, S, both):
    r = scan(codes, S, both)
    return r["best"] if both else r["best_plus"]


def site_counts(codes, S, t, both):
    return scan(codes, S, both, thr=t)["counts"]


def sites(codes, S, t, both):
    return scan(codes, S, both, thr=t)["sites"]


def all_sites(codes, Ss, ts, both):
    """every motif's sites in the --sites order, as motif_sites_model.all_sites"""
    parts = [sites(codes, S, t, both) for S, t in zip(Ss, ts)]
    out = np.zeros(sum(len(p) for p in parts), ALL_SITES)
    j = 0
    for m, p in enumerate(parts):
        o = out[j:j + len(p)]
        o["motif"], o["seq"], o["pos"], o["strand"], o["score"] = m, p["seq"], p["pos"], p["strand"], p["score"]
        j += len(p)
    return out


def best_sites(codes, S, both, m, seq0=0, index=None):
    r = scan(codes, S, both, m=m, seq0=seq0, index=index)
    return r["best_site"], r["site"]


def clamp_flank(w, flank):
    return min(int(flank), (MAX_MOTIF_LEN - int(w)) // 2)


def site_profile(codes, best, site, w, t, flank):
    """counts (MAX_MOTIF_LEN x 5 uint64) of one motif from its best sites, as motif_refine_model.site_profile"""
    codes = np.asarray(codes, np.uint8)
    n, L = codes.shape
    F = clamp_flank(w, flank)
    counts = np.zeros((MAX_MOTIF_LEN, 5), np.uint64)
    best = np.asarray(best, np.int64)
    p = (np.asarray(site, np.uint64) >> np.uint64(1)).astype(np.int64)
    s = (np.asarray(site, np.uint64) & np.uint64(1)).astype(np.int64)
    rows = np.nonzero((best != SENTINEL) & (best >= t) & (L >= w) & (p <= L - w))[0]
    if len(rows) == 0:
        return counts
    p, s = p[rows], s[rows]
    for col in range(-F, w + F):
        q = np.where(s == 0, p + col, p + w - 1 - col)
        inside = (q >= 0) & (q < L)
        c = codes[rows, np.clip(q, 0, L - 1)].astype(np.int64)
        ok = inside & (c >= 1) & (c <= 4)
        b = np.where(ok, np.where(s == 0, c - 1, 4 - c), 4)
        counts[col + F] += np.bincount(b, minlength=5).astype(np.uint64)
    return counts


# ---- a mixed-length set: flat codes + offsets, one length class at a time -------------------------------------------
def length_classes(offs):
    """[(L, idx)]: the sequences of every length that occurs, idx ascending"""
    lens = np.diff(np.asarray(offs, np.int64))
    return [(int(L), np.nonzero(lens == L)[0]) for L in np.unique(lens)]


def class_codes(codes, offs, idx, L):
    return np.asarray(codes, np.uint8)[np.asarray(offs, np.int64)[idx][:, None] + np.arange(L)[None, :]]


def scan_mixed(codes, offs, S, both, thr=None, m=None, seq0=0):
    """scan() of a mixed-length set: the same dict, every array in the set's order, the sites sorted by sequence (within
    one sequence they keep their order)"""
    n = len(offs) - 1
    out, recs = {}, []
    for L, idx in length_classes(offs):
        r = scan(class_codes(codes, offs, idx, L), S, both, thr=thr, m=m, seq0=seq0, index=idx)
        for k, v in r.items():
            if k == "sites":
                v["seq"] = idx[v["seq"]]
                recs.append(v)
            else:
                out.setdefault(k, np.zeros(n, v.dtype))[idx] = v
    if thr is not None:
        rec = np.concatenate(recs) if recs else np.zeros(0, SITES)
        out["sites"] = rec[np.argsort(rec["seq"], kind="stable")]
    return out


def site_profile_mixed(codes, offs, best, site, w, t, flank):
    counts = np.zeros((MAX_MOTIF_LEN, 5), np.uint64)
    for L, idx in length_classes(offs):
        if L:
            counts += site_profile(class_codes(codes, offs, idx, L), np.asarray(best)[idx], np.asarray(site)[idx], w, t, flank)
    return counts
