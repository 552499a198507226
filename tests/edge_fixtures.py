"""What tests/golden/make_edge_golden.py and the tests that read its fixtures (tests/golden/edges_*.npz) must agree on: the
tag and the input arrays of every case of em_edges_model, table_edges_model and count_edges_model, how arrays are hashed,
which indices of a large table a fixture keeps, and how a fixture file is read.  No GPU, no reference here.

A fixture holds, per case, the sha256 of every INPUT array (so that a change of a model or of numpy shows as "inputs
drifted, regenerate" and not as a parity failure) and what the compiled reference (oracle/_ref/ref_edges, ref_dump)
made of those inputs: small results in full, large tables as sha256 plus the values at SLICE indices.

Float tables are hashed in a canonical form: every NaN as 0x7FC00000.  x86 and gfx950 give 0 / 0 different sign bits
(tests/test_gpu_table_edges.py), so the device could never meet a hash of the raw bits; the stored slices and the EM PWMs
are the reference's raw bits, and the CPU tests compare those byte for byte."""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EM_WS = (2, 4, 6, 8, 10, 12)
TABLE_WS = (2, 4, 6, 8, 10, 12)   # W = 14 stays oracle-only: the reference's size_t counter table alone is 2 GiB there
COUNT_WS = (2, 4, 6, 8, 10, 12)
FULL_LIMIT = 4096                 # arrays up to this many entries can be stored in full
SEED_SELECTIONS = ((10.0, 3, 1), (3.0, 1, 0))  # (z threshold, count threshold, filter_neighbors): oracle/ref_dump.cpp's two


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def canonical(a):
    """float32 array -> its bits with every NaN as 0x7FC00000"""
    a = np.ascontiguousarray(a, np.float32)
    bits = a.view(np.uint32).copy()
    bits[np.isnan(a)] = 0x7FC00000
    return bits


def table_digest(a):
    a = np.asarray(a)
    return digest(canonical(a) if a.dtype == np.float32 else a)


def f32_bits(x):
    return int(np.float32(x).view(np.uint32))


_files = {}


def load(name):
    """a fixture file as a dict of arrays, with `index`: tag -> row"""
    if name not in _files:
        path = os.path.join(GOLDEN, name + ".npz")
        with np.load(path) as z:
            d = {k: z[k] for k in z.files}
        d["index"] = {str(t): i for i, t in enumerate(d["tags"])}
        _files[name] = d
    return _files[name]


def inputs_match(fix, tag, arrays):
    """-> None, or a sentence: the inputs of `tag` are not the ones the fixture was made from"""
    i = fix["index"].get(tag)
    if i is None:
        return "case %s has no fixture entry: regenerate with tests/golden/make_edge_golden.py" % tag
    for j, a in enumerate(arrays):
        if not np.array_equal(fix["sha_in"][i, j], digest(a)):
            return "inputs drifted: input %d of case %s is not what the fixture was made from; regenerate" % (j, tag)
    return None


# ---- EM ----------------------------------------------------------------------------------------------------------------
def em_file(W):
    return "edges_em_w%d" % W


def em_inputs(c):
    params = np.array([f32_bits(c["saturation"]), f32_bits(c["threshold"]), c["max_iter"]], np.uint32)
    return [c["counts"], c["bg"], c["pwms"], params]


def em_cases(W):
    import em_edges_model as em
    return [(cls, c) for cls in em.classes(W) for c in em.cases(W, cls)]


def em_reference(fix, c):
    """float32 [max_iter + 1, n PWMs, W, 4]: the reference's returned PWM at every iteration cap 0 .. max_iter"""
    i = fix["index"][c["tag"]]
    flat = fix["pwm_cat"][fix["pwm_off"][i]:fix["pwm_off"][i + 1]]
    return flat.view(np.float32).reshape(c["max_iter"] + 1, len(c["pwms"]), c["W"], 4)


def em_reference_iterations(ref, threshold):
    """per PWM: (m, identifiable) -- m the smallest cap whose PWM is the PWM at max_iter byte for byte.  m is the
    reference's iteration count where the PWMs at caps 0 .. m are pairwise different and m < max_iter is explained by
    the stopping rule alone.  It is not where the run reached a fixed point IN BYTES before max_iter while the loop went
    on counting: a PWM with a NaN entry (its `change` is NaN, which stops nothing), or any repeated PWM under a threshold
    that no positive change meets (0.0, -0.0, NaN) -- the loop then ran on to max_iter, or stopped one iteration after
    the PWM first repeated, and the returned PWMs cannot tell."""
    caps, n = ref.shape[:2]
    out = []
    for i in range(n):
        b = [ref[k, i].tobytes() for k in range(caps)]
        m = next(k for k in range(caps) if b[k] == b[-1])
        distinct = len(set(b[:m + 1])) == m + 1
        stuck = m < caps - 1 and (bool(np.isnan(ref[m, i]).any()) or not np.float32(threshold) > 0)
        out.append((m, distinct and not stuck))
    return out


def em_reference_counts(fix, c):
    """int32 per PWM: the reference's iteration count as the fixture stores it (em_reference_iterations of its own PWMs
    when it was made), -1 where the count is not identifiable"""
    i = fix["index"][c["tag"]]
    return fix["iters"][fix["iters_off"][i]:fix["iters_off"][i + 1]]


def final_normalisation(pwms):
    """IUPACPattern::normalize_pwm as the constructor of the returned pattern applies it once more: per row the float32
    sum ((0 + a) + c) + g) + t and four float32 divisions"""
    p = np.ascontiguousarray(pwms, np.float32)
    with np.errstate(all="ignore"):
        s = np.zeros(p.shape[:-1], np.float32)
        for a in range(4):
            s = (s + p[..., a]).astype(np.float32)
        return (p / s[..., None]).astype(np.float32)


# ---- counts ------------------------------------------------------------------------------------------------------------
def count_file(W):
    return "edges_count_w%d" % W


def count_tag(cls, part, W, both):
    import count_edges_model as cm
    return cm.case_tag(cls, part, W, both)


def count_inputs(part):
    return [part["codes"], part["offs"]]


def count_cases(W):
    import count_edges_model as cm
    return [(cls, k, part, both) for cls in cm.CLASSES for k, part in enumerate(cm.CLASSES[cls](W)) for both in (False, True)]


def count_slice(table, n=256):
    """indices a fixture keeps of a count table beyond FULL_LIMIT: bins that hold a count (every value the table holds
    at least once, the largest first) and the zero bins next to them"""
    nz = np.flatnonzero(table)
    if not nz.size:
        return np.arange(8, dtype=np.int64)
    order = nz[np.argsort(-table[nz].astype(np.int64), kind="stable")]
    first = nz[np.unique(table[nz], return_index=True)[1]]
    spread = nz[::max(1, nz.size // (n // 2))]
    idx = np.unique(np.concatenate([order[:n // 4], first, spread]))[:n]
    near = np.clip(np.concatenate([idx[:16] - 1, idx[:16] + 1]), 0, table.size - 1)
    return np.unique(np.concatenate([idx, near])).astype(np.int64)


# ---- tables ------------------------------------------------------------------------------------------------------------
def table_file(W):
    return "edges_tables_w%d" % W


MISC_FILE = "edges_tables_misc"  # background model, IUPAC aggregation, similarity


def sweep_tag(W, both, case):
    import table_edges_model as tm
    return tm.sweep_tag(W, both, case)


def sweep_inputs(c):
    params = np.array([c["W"], int(c["both"]), c["k"], c["max_k"], c["ltot"]], np.int64)
    return [c["V"], c["counts"], params]


def sweep_cases(W):
    import table_edges_model as tm
    return [(both, case) for both in (False, True) for case in tm.sweep_cases(W, both)]


SWEEP_TABLES = ("bgp0", "bgp1", "bgp2", "expected", "logp", "z")
N_SLICE = 128
SWEEP_FULL_LIMIT = 256  # sweep tables up to this size are stored in full as well (W <= 4)


def sweep_slice(c, seeds=()):
    """the indices a fixture keeps of the tables of a sweep case (N_SLICE at most, -1 padded): bins with a zero count,
    the first bin of every count value the table holds (the mu edges among them), palindromes, patterns of own-twin
    tiles (W >= 12), the first seeds, and a strided sample of the rest"""
    import table_edges_model as tm
    W, counts = c["W"], c["counts"]
    parts = [np.flatnonzero(counts == 0)[:4], np.unique(counts, return_index=True)[1]]
    r = tm.revcomp_ids(W)
    parts.append(np.flatnonzero(r == np.arange(4 ** W, dtype=np.uint32))[:3])
    if W >= 12:
        parts.append(np.flatnonzero(tm.own_twin_tile_mask(W))[:4])
    parts.append(np.asarray(seeds, np.int64)[:6])
    edges = np.unique(np.concatenate([np.asarray(p, np.int64) for p in parts]))[:N_SLICE]
    fill = np.setdiff1d(np.arange(0, 4 ** W, max(1, 4 ** W // N_SLICE), dtype=np.int64), edges)[:N_SLICE - edges.size]
    idx = np.union1d(edges, fill)
    return np.concatenate([idx, np.full(N_SLICE - idx.size, -1, np.int64)])


def sweep_tables(c):
    """name -> table of a sweep case in the model's (the oracle's) or a device's dict form"""
    out = {"bgp%d" % o: c["bgp"][o] for o in range(c["max_k"] + 1)}
    out.update(expected=c["expected"], logp=c["logp"], z=c["z"])
    return out


def bg_cases():
    """(tag, counters int64, K, alpha, in_range): in_range = every counter fits the reference's `int`"""
    import table_edges_model as tm
    out = []
    for name, n, K, alpha, _ in tm.bg_model_cases():
        used = sum(4 ** (k + 1) for k in range(K + 1))
        out.append(("bg/" + name, n[:used], K, alpha, bool(n.max() < 2 ** 31 and n[:4].sum() < 2 ** 31)))
    return out


def bg_inputs(n, K, alpha):
    return [n.astype(np.int64), np.array([K], np.int64), np.asarray(alpha, np.float32)]


IUPAC_CASES = [(W, both, v) for W in (10, 12) for both in (False, True) for v in ("a", "c")]


def iupac_tag(W, both, v):
    return "iupac/W%d/%s/V%s" % (W, "both" if both else "plus", v)


def iupac_inputs(c):
    return [c["counts"], c["bgp"], c["expected"], c["ids"]]


def sim_tag(both):
    return "sim/%s" % ("both" if both else "plus")


def sim_inputs():
    import table_edges_model as tm
    pw, cp, lens, sites = tm.motif_set()
    return [pw, cp, lens, sites, tm.SIM_BG]
