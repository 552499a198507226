#!/usr/bin/env python3
"""Generate tests/golden/edges_*.npz: what the REAL reference makes of the constructed edge cases of
tests/em_edges_model.py, tests/table_edges_model.py and tests/count_edges_model.py.

Run only where the reference exists (oracle/_ref needs its sources), after the product and the oracle are built:

    make -C oracle all ref && python tests/golden/make_edge_golden.py [em] [tables] [counts]

Tables and PWMs are injected into the reference's own objects by oracle/_ref/ref_edges (oracle/ref_edges.cpp); the count
cases are written as FASTA files and go through oracle/_ref/ref_dump ... tables.  Every result is compared with
oracle/peng_oracle.cpp on the way and the disagreements are printed (exit 1 on any), but what is WRITTEN is the
reference's answer alone.  tests/edge_fixtures.py holds the layout both this script and the tests use.  A second run
writes the same bytes.

Cases the reference cannot answer.  UNDEFINED lists, by tag, cases on which the reference's own C++ is undefined (with
the line that makes it so): they stay in the oracle-versus-kernel tests and get no fixture entry; the CPU test holds the
list to 5 % of a class.  NARROWED lists inputs that cannot be put into the reference at all.  Neither list may grow to
make a test pass."""
import io
import os
import subprocess
import sys
import tempfile
import zipfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import edge_fixtures as ef  # noqa: E402
from oracle import oracle as po  # noqa: E402

REF_EDGES = os.path.join(ROOT, "oracle", "_ref", "ref_edges")
REF_DUMP = os.path.join(ROOT, "oracle", "_ref", "ref_dump")
JOBS = min(8, os.cpu_count() or 1)

# tag -> the reference line that makes the case undefined.  (An IUPAC id is tagged <case>#<the model's name of the id>.)
UNDEFINED = {
    "iupac/W10/plus/Va#all_N": "src/iupac_pattern.cpp:443: assert(sum_backgroud_prob >= 0 and sum_backgroud_prob <= 1) aborts: the "
                               "float32 sum of all 4^10 members' probabilities is 1.000009",
}

# What cannot be put into the reference, by tag prefix:
NARROWED = {
    # BackgroundModel::n_ is `int**` (src/shared/BackgroundModel.h:69): counters beyond 2^31 - 1 have no representation
    # there.  The product documents 64-bit counters for them (oracle bg_V(..., wide=True)); oracle-only.
    "bg/above_2_31": "counters beyond INT_MAX cannot be written into BackgroundModel::n_ (int)",
}
# Seed lists are left out of a sweep case (not the case itself) where its z-scores hold a NaN: select_base_patterns
# sorts ids with `z[i] > z[j]` (src/base_pattern.cpp:458, sort_indices :171), no strict weak ordering with a NaN in
# it, so std::sort is undefined.  oracle/ref_edges.cpp decides that from the reference's own z table.


def hexf(x):
    return "%08x" % ef.f32_bits(x)


def save(name, arrays):
    """a deterministic .npz: fixed member order and dates, so that a second run writes the same bytes"""
    path = os.path.join(HERE, name + ".npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    print("wrote %-24s %8d bytes" % (name + ".npz", os.path.getsize(path)))


def run_ref(mode, job, arrays, outputs, optional=()):
    """one ref_edges run in a directory of its own -> {output: array}, or the exit status if the reference died"""
    with tempfile.TemporaryDirectory(prefix="refedges_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as d:
        with open(os.path.join(d, "job.txt"), "w") as f:
            f.write(job)
        for name, a in arrays.items():
            np.ascontiguousarray(a).tofile(os.path.join(d, name))
        r = subprocess.run([REF_EDGES, mode, d], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
        if r.returncode != 0:
            return r.returncode, r.stderr.decode(errors="replace")[-300:]
        out = {}
        for name, dt in list(outputs.items()) + [(n, t) for n, t in optional if os.path.exists(os.path.join(d, n))]:
            out[name] = np.fromfile(os.path.join(d, name), dt)
        return out


def pack(rows, dtype):
    """a list of 1-d arrays -> (offsets int64[n + 1], concatenation)"""
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    cat = np.concatenate([np.asarray(r, dtype).reshape(-1) for r in rows]) if rows else np.zeros(0, dtype)
    return off, cat.astype(dtype)


class Report:
    def __init__(self):
        self.bad = []

    def check(self, tag, what, same):
        if not same:
            self.bad.append("%s: %s" % (tag, what))
            print("   ORACLE != REFERENCE  %s: %s" % (tag, what))


def died(tag, r):
    sys.exit("the reference did not finish %s (status %s: %s).  If its behaviour there is undefined C++, list the tag in "
             "UNDEFINED with the line that makes it so; otherwise this is a bug of the driver." % (tag, r[0], r[1]))


# ---- EM ----------------------------------------------------------------------------------------------------------------
def em_reference(c):
    caps = range(c["max_iter"] + 1)
    job = "%d %d %s %s %s\n" % (c["W"], len(c["pwms"]), hexf(c["saturation"]), hexf(c["threshold"]), " ".join(map(str, caps)))
    r = run_ref("em", job, {"counts.u32": c["counts"], "bg.f32": c["bg"], "pwms.f32": c["pwms"]}, {"out.f32": np.uint32})
    if isinstance(r, tuple):
        died(c["tag"], r)
    return r["out.f32"]


def make_em(rep):
    for W in ef.EM_WS:
        cases = [(cls, c) for cls, c in ef.em_cases(W) if c["tag"] not in UNDEFINED]
        with ThreadPoolExecutor(JOBS if W < 12 else 4) as pool:
            outs = list(pool.map(lambda cc: em_reference(cc[1]), cases))
            # the oracle at the last cap, with its final normalisation, and its iteration count
            jobs = [(c, i) for _, c in cases for i in range(len(c["pwms"]))]
            orc = list(pool.map(lambda j: po.em(W, j[0]["counts"].astype(np.uint64), j[0]["bg"], j[0]["pwms"][j[1]], j[0]["saturation"],
                                                j[0]["threshold"], j[0]["max_iter"], mode=0), jobs))
        at, counts = 0, []
        for (cls, c), out in zip(cases, outs):
            ref = out.view(np.float32).reshape(c["max_iter"] + 1, len(c["pwms"]), W, 4)
            its = ef.em_reference_iterations(ref, c["threshold"])
            counts.append([m if ok else -1 for m, ok in its])
            for i in range(len(c["pwms"])):
                pw, it, _ = orc[at]
                at += 1
                rep.check(c["tag"], "PWM %d" % i, pw.tobytes() == ref[-1, i].tobytes())
                if its[i][1]:
                    rep.check(c["tag"], "iterations of PWM %d: oracle %d, reference %d" % (i, it, its[i][0]), it == its[i][0])
        off, cat = pack(outs, np.uint32)
        it_off, it_cat = pack(counts, np.int32)
        save(ef.em_file(W), dict(iters_off=it_off, iters=it_cat,
                                 tags=np.array([c["tag"] for _, c in cases]), classes=np.array([cls for cls, _ in cases]),
                                 sha_in=np.stack([np.stack([ef.digest(a) for a in ef.em_inputs(c)]) for _, c in cases]),
                                 pwm_off=off, pwm_cat=cat))
        print("em W = %-2d %3d cases, %d PWMs" % (W, len(cases), at))


# ---- counts ------------------------------------------------------------------------------------------------------------
def write_fasta(path, codes, offs):
    letters = np.frombuffer(b"NACGT", np.uint8)
    with open(path, "wb") as f:
        for s, (a, e) in enumerate(zip(offs[:-1], offs[1:])):
            f.write(b">s%d\n" % s + letters[codes[a:e]].tobytes() + b"\n")


def count_reference(part, W, both):
    with tempfile.TemporaryDirectory(prefix="refcount_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as d:
        fa = os.path.join(d, "in.fa")
        write_fasta(fa, part["codes"], part["offs"])
        subprocess.check_call([REF_DUMP, fa, str(W), "BOTH" if both else "PLUS", d, "tables"], stdout=subprocess.DEVNULL,
                              stderr=subprocess.DEVNULL)
        meta = dict(l.split() for l in open(os.path.join(d, "meta.txt")))
        ld = lambda f, t: np.fromfile(os.path.join(d, f), t)  # noqa: E731
        return dict(codes=ld("codes.u8", np.uint8), offs=ld("offs.i64", np.int64), counts=ld("counts.u64", np.uint64),
                    bgcounts=ld("bgcounts.i32", np.int32).astype(np.int64), ltot=int(meta["ltot"]))


def make_counts(rep):
    for W in ef.COUNT_WS:
        cases = ef.count_cases(W)
        with ThreadPoolExecutor(JOBS if W < 12 else 3) as pool:
            refs = list(pool.map(lambda c: count_reference(c[2], W, c[3]), cases))
        g = dict(tags=[], classes=[], sha_in=[], sha_counts=[], ltot=[], bgcounts=[], rows=[], idx=[])
        for (cls, k, part, both), r in zip(cases, refs):
            tag = ef.count_tag(cls, part, W, both)
            # the sequences the reference parsed are the case's: a sequence of the model's never ends up empty or merged
            assert np.array_equal(r["codes"], part["codes"]) and np.array_equal(r["offs"], part["offs"]), tag
            want, ltot = po.count(part["codes"], part["offs"], W, both)
            rep.check(tag, "count table", np.array_equal(want, r["counts"]))
            rep.check(tag, "ltot: oracle %d, reference %d" % (ltot, r["ltot"]), ltot == r["ltot"])
            rep.check(tag, "background counters", np.array_equal(po.bg_counts(part["codes"], part["offs"], 2), r["bgcounts"]))
            idx = np.arange(4 ** W, dtype=np.int64) if 4 ** W <= ef.FULL_LIMIT else ef.count_slice(r["counts"])
            g["tags"].append(tag)
            g["classes"].append(cls)
            g["sha_in"].append(np.stack([ef.digest(a) for a in ef.count_inputs(part)]))
            g["sha_counts"].append(ef.digest(r["counts"]))
            g["ltot"].append(r["ltot"])
            g["bgcounts"].append(r["bgcounts"])
            g["idx"].append(idx)
            g["rows"].append(r["counts"][idx])
        ioff, icat = pack(g["idx"], np.int64)
        _, vcat = pack(g["rows"], np.uint64)
        save(ef.count_file(W), dict(tags=np.array(g["tags"]), classes=np.array(g["classes"]), sha_in=np.stack(g["sha_in"]),
                                    sha_counts=np.stack(g["sha_counts"]), ltot=np.array(g["ltot"], np.uint64),
                                    bgcounts=np.stack(g["bgcounts"]), slice_off=ioff, slice_idx=icat.astype(np.uint32),
                                    slice_val=vcat))
        print("counts W = %-2d %3d cases" % (W, len(cases)))


# ---- tables ------------------------------------------------------------------------------------------------------------
def sweep_reference(c, tag):
    job = "%d %s %d %d %d 1\n" % (c["W"], "BOTH" if c["both"] else "PLUS", c["k"], c["max_k"], c["ltot"])
    job += "".join("%s %d %d\n" % (hexf(z), n, f) for z, n, f in ef.SEED_SELECTIONS)
    outs = {"bgp%d.f32" % o: np.float32 for o in range(c["max_k"] + 1)}
    outs.update({"expected.f32": np.float32, "logp.f32": np.float32, "z.f32": np.float32})
    r = run_ref("sweep", job, {"V.f32": c["V"], "counts.u32": c["counts"]}, outs,
                optional=[("seeds%d.u64" % i, np.uint64) for i in range(len(ef.SEED_SELECTIONS))] + [("seeds_undefined", np.uint8)])
    if isinstance(r, tuple):
        died(tag, r)
    return r


def make_sweeps(rep):
    import table_edges_model as tm
    for W in ef.TABLE_WS:
        cases = [(both, case) for both, case in ef.sweep_cases(W) if ef.sweep_tag(W, both, case) not in UNDEFINED]
        g = dict(tags=[], sha_in=[], sha_out=[], idx=[], vals=[], full=[], seeds=[[] for _ in ef.SEED_SELECTIONS], seed_sha=[], seeds_defined=[])

        # (the model keeps the oracle's probability tables for one (W, V, strand mode) at a time: cases in the model's order,
        # the reference runs of a batch side by side)
        batch = JOBS if W <= 10 else 2
        for b0 in range(0, len(cases), batch):
            cs = [tm.sweep_case(W, both, case) for both, case in cases[b0:b0 + batch]]
            with ThreadPoolExecutor(batch) as pool:
                rs = list(pool.map(lambda i: sweep_reference(cs[i], ef.sweep_tag(W, *cases[b0 + i])), range(len(cs))))
            for (both, case), c, r in zip(cases[b0:b0 + batch], cs, rs):
                tag = ef.sweep_tag(W, both, case)
                ref = {n: r[n + ".f32"] for n in ef.SWEEP_TABLES if n + ".f32" in r}
                for n, t in ef.sweep_tables(c).items():
                    rep.check(tag, n, t.tobytes() == ref[n].tobytes())
                defined = "seeds_undefined" not in r
                seeds = [r["seeds%d.u64" % i] if defined else np.zeros(0, np.uint64) for i in range(len(ef.SEED_SELECTIONS))]
                if defined:
                    for i, (zt, ct, flt) in enumerate(ef.SEED_SELECTIONS):
                        got = po.select(W, c["z"], c["counts"].astype(np.uint64), zt, ct, not both, bool(flt))
                        rep.check(tag, "seed selection %d" % i, np.array_equal(got, seeds[i]))
                idx = ef.sweep_slice(c, seeds[0])
                g["tags"].append(tag)
                g["sha_in"].append(np.stack([ef.digest(a) for a in ef.sweep_inputs(c)]))
                g["sha_out"].append(np.stack([ef.table_digest(ref[n]) if n in ref else np.zeros(32, np.uint8) for n in ef.SWEEP_TABLES]))
                g["idx"].append(idx)
                safe = np.maximum(idx, 0)
                g["vals"].append(np.stack([ref[n][safe].view(np.uint32) if n in ref else np.zeros(len(idx), np.uint32) for n in ef.SWEEP_TABLES]))
                if 4 ** W <= ef.SWEEP_FULL_LIMIT:
                    g["full"].append(np.stack([ref[n].view(np.uint32) if n in ref else np.zeros(4 ** W, np.uint32) for n in ef.SWEEP_TABLES]))
                g["seeds_defined"].append(defined)
                g["seed_sha"].append(np.stack([ef.digest(s) for s in seeds]))
                for i, s in enumerate(seeds):
                    g["seeds"][i].append(s[:64])
                del c, r, ref
            del cs, rs
        out = dict(tags=np.array(g["tags"]), classes=np.array(["sweep"] * len(g["tags"])), sha_in=np.stack(g["sha_in"]),
                   sha_out=np.stack(g["sha_out"]), slice_idx=np.stack(g["idx"]).astype(np.int32), slice_val=np.stack(g["vals"]),
                   seeds_defined=np.array(g["seeds_defined"]), seed_sha=np.stack(g["seed_sha"]))
        if g["full"]:
            out["full"] = np.stack(g["full"])
        for i in range(len(ef.SEED_SELECTIONS)):
            out["seeds%d_off" % i], out["seeds%d_head" % i] = pack(g["seeds"][i], np.uint32)
        save(ef.table_file(W), out)
        print("sweep W = %-2d %4d cases, seed lists defined in %d" % (W, len(cases), int(np.sum(g["seeds_defined"]))))


def make_misc(rep):
    import table_edges_model as tm
    out = dict(tags=[], classes=[], sha_in=[])
    width = 5

    def add(tag, cls, inputs):
        out["tags"].append(tag)
        out["classes"].append(cls)
        d = [ef.digest(a) for a in inputs]
        out["sha_in"].append(np.stack(d + [np.zeros(32, np.uint8)] * (width - len(d))))

    # background model
    cases = [c for c in ef.bg_cases() if c[4]]
    for c in ef.bg_cases():
        assert c[4] or any(c[0].startswith(p) for p in NARROWED), c[0]
    job, arrays, outs = "", {}, {}
    for j, (tag, n, K, alpha, _) in enumerate(cases):
        job += "c%d %d %s %s %s\n" % (j, K, hexf(alpha[0]), hexf(alpha[1]), hexf(alpha[2]))
        arrays["c%d.n.i32" % j] = n.astype(np.int32)
        outs["c%d.V.f32" % j] = np.float32
    r = run_ref("bg", job, arrays, outs)
    if isinstance(r, tuple):
        died("bg", r)
    want = {name: V for name, _, _, _, V in tm.bg_model_cases()}
    V = np.zeros((len(cases), 84), np.float32)
    for j, (tag, n, K, alpha, _) in enumerate(cases):
        got = r["c%d.V.f32" % j]
        V[j, :len(got)] = got
        rep.check(tag, "V", V[j].tobytes() == want[tag[3:]].tobytes())
        add(tag, "bg", ef.bg_inputs(n, K, alpha))
    out["bg_V"] = V.view(np.uint32)

    # IUPAC aggregation
    rows = []
    for W, both, v in ef.IUPAC_CASES:
        tag = ef.iupac_tag(W, both, v)
        c = tm.iupac_case(W, both, v)
        job = "%d %s 2 2 %d 0\n%d\n" % (W, "BOTH" if both else "PLUS", tm.LTOTS[2], len(c["ids"]))
        r = run_ref("iupac", job, {"bgp.f32": c["bgp"], "counts.u32": c["counts"], "ids.u64": c["ids"]},
                    {"sites.u64": np.uint64, "cc.u64": np.uint64, "stats.f32": np.uint32, "died.u8": np.uint8})
        if isinstance(r, tuple):
            died(tag, r)
        st = r["stats.f32"].reshape(-1, 4)
        c64 = c["counts"].astype(np.uint64)
        for j, w in enumerate(c["want"]):
            if r["died.u8"][j] or "%s#%s" % (tag, c["names"][j]) in UNDEFINED:
                if not (r["died.u8"][j] and "%s#%s" % (tag, c["names"][j]) in UNDEFINED):
                    died("%s#%s" % (tag, c["names"][j]), (int(r["died.u8"][j]), "UNDEFINED and the reference's abort do not agree"))
                continue
            got = np.array([w.bg_p, w.expected, w.zscore, w.log_pvalue], np.float32).view(np.uint32)
            rep.check(tag, "%s: sites / stats" % c["names"][j], w.sites == r["sites.u64"][j] and np.array_equal(got, st[j]))
            rep.check(tag, "%s: combined count" % c["names"][j], po.iupac_count(int(c["ids"][j]), W, both, c64) == r["cc.u64"][j])
        add(tag, "iupac", ef.iupac_inputs(c))
        rows.append((r["sites.u64"], r["cc.u64"], st.reshape(-1), r["died.u8"], np.array(c["names"])))
        del c
    out["iupac_off"], out["iupac_sites"] = pack([x[0] for x in rows], np.uint64)
    out["iupac_cc"] = pack([x[1] for x in rows], np.uint64)[1]
    out["iupac_stats"] = pack([x[2] for x in rows], np.uint32)[1]
    out["iupac_died"] = pack([x[3] for x in rows], np.uint8)[1]
    out["iupac_names"] = np.concatenate([x[4] for x in rows])

    # similarity
    pw, cp, lens, sites = tm.motif_set()
    S = []
    for both in (False, True):
        r = run_ref("sim", "%d %d %s\n" % (len(lens), tm.MAX_MOTIF_LEN, "BOTH" if both else "PLUS"),
                    {"pwms.f32": pw, "lens.i32": lens, "sites.u64": sites, "bg.f32": tm.SIM_BG}, {"S.f32": np.float32})
        if isinstance(r, tuple):
            died(ef.sim_tag(both), r)
        S.append(r["S.f32"])
        worst = np.nanmax(np.abs(np.where(np.isfinite(S[-1]), S[-1].astype(np.float64) - tm.exact_grid(both), 0.0)))
        rep.check(ef.sim_tag(both), "-inf pairs", np.array_equal(np.isneginf(S[-1]), np.isneginf(tm.exact_grid(both))))
        print("similarity, %s: the restated float32 sums differ from calculate_S by at most %.3g" % (ef.sim_tag(both), worst))
        add(ef.sim_tag(both), "sim", ef.sim_inputs())
    out["sim_S"] = np.stack(S).view(np.uint32)
    out["tags"], out["classes"], out["sha_in"] = np.array(out["tags"]), np.array(out["classes"]), np.stack(out["sha_in"])
    out["narrowed"] = np.array(sorted(NARROWED))
    save(ef.MISC_FILE, out)


def main():
    for exe in (REF_EDGES, REF_DUMP):
        if not os.path.exists(exe):
            sys.exit("build the reference first: make -C oracle ref")
    which = [a for a in sys.argv[1:] if not a.startswith("-")] or ["em", "tables", "counts"]
    rep = Report()
    if "em" in which:
        make_em(rep)
    if "counts" in which:
        make_counts(rep)
    if "tables" in which:
        make_misc(rep)
        make_sweeps(rep)
    save("edges_excluded", dict(tags=np.array(sorted(UNDEFINED), dtype="U1" if not UNDEFINED else None),
                                reasons=np.array([UNDEFINED[t] for t in sorted(UNDEFINED)], dtype="U1" if not UNDEFINED else None)))
    print("%d disagreements between the oracle and the reference" % len(rep.bad))
    sys.exit(1 if rep.bad else 0)


if __name__ == "__main__":
    main()
