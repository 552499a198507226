"""The scenario of tests/test_gpu_cli_combined.py: one input on which --mask-low-complexity, --holdout, --erase and --dyads
all change what round 1 of the search is run on, and on which a report that scanned that changed input instead of the
whole one would print other lines (every report scans the unmasked, whole input).

A variant of motif_dust_model.tracts: n uniform sequences of L bases, `word` planted in a share f_word of them (every
letter kept with probability p).  In a share f_tract of the word-carrying sequences the word is IMMEDIATELY FOLLOWED by a
poly-A or (CA)n tract of 20-40 bases: the symmetric-DUST mask takes the tract and reaches into the word's last bases, so
these sites hold masked bases.  The other word sites are placed freely.  A second word, `other`, is planted before all
that in a share f_other of the sequences from a random stream of its own (so the first word's sites and the tracts are
where they are without it): every run then reports at least two motifs, and --spacing has a pair to print.
tests/test_cli_combined_cpu.py certifies the conditions the GPU module relies on without a GPU."""
import numpy as np

import motif_compare_model as mc
import motif_dust_model as md
import motif_holdout_model as mh

WORD = "TGACTCAGCA"
OTHER = "GGCTGGAGTG"  # (motif B of tests/motif_erase_model.py)
SEED = 1            # the input's seed
CONTROL_SEED = 11   # the control set's
T = md.DEFAULT_T    # --mask-threshold's default
FRACTION, HOLDOUT_SEED = 0.1, 1  # --holdout-fraction's and --holdout-seed's defaults


def mutated(rng, w, p):
    c = w.copy()
    for j in np.flatnonzero(rng.random(len(w)) >= p).tolist():
        c[j] = (c[j] - 1 + rng.integers(1, 4)) % 4 + 1
    return c


def tracts_behind_the_word(seed, n=2000, L=100, word=WORD, f_word=0.3, f_tract=0.25, p=0.85, other=OTHER, f_other=0.2):
    """(seqs, sites): the sequences (byte codes) and [(sequence, position)] of every planted `word`"""
    rng = np.random.default_rng(seed)
    seqs = [rng.integers(1, 5, L).astype(np.uint8) for _ in range(n)]
    w = md.codes_of(word)
    rng2 = np.random.default_rng([seed, 2])
    o = md.codes_of(other)
    for i in np.flatnonzero(rng2.random(n) < f_other).tolist():
        q = int(rng2.integers(0, L - len(o) + 1))
        seqs[i][q:q + len(o)] = mutated(rng2, o, p)
    sites = []
    for i in np.flatnonzero(rng.random(n) < f_word).tolist():
        c = mutated(rng, w, p)
        if rng.random() < f_tract:
            m = int(rng.integers(20, 41))
            q = int(rng.integers(0, L - len(w) - m + 1))
            seqs[i][q + len(w):q + len(w) + m] = 1 if rng.random() < 0.5 else np.tile(md.codes_of("CA"), 20)[:m]
        else:
            q = int(rng.integers(0, L - len(w) + 1))
        seqs[i][q:q + len(w)] = c
        sites.append((i, q))
    return seqs, sites


def control(seed=CONTROL_SEED):
    """the control set of the --discriminative runs: the same kind of tracts, no planted word"""
    return md.tracts(seed, f_word=0.0)


def names_of(n):
    return ["s%d" % k for k in range(n)]


def fasta_text(seqs, names=None):
    """FASTA text; `names` keeps a subset's records under the names they have in the whole file"""
    names = names_of(len(seqs)) if names is None else names
    return "".join(">%s\n%s\n" % (k, "".join("NACGT"[x] for x in c)) for k, c in zip(names, seqs))


def gone(seqs, masked):
    """bool per base of every sequence: the mask took it"""
    return [np.asarray(c) != np.asarray(m) for c, m in zip(seqs, masked)]


def sites_with_a_masked_base(sites, taken, width=len(WORD)):
    """[(sequence, position, masked bases)] of the sites [position, position + width) that hold a base the mask took"""
    out = []
    for i, q in sites:
        k = int(taken[i][q:q + width].sum())
        if k:
            out.append((i, q, k))
    return out


def split(n, seed=HOLDOUT_SEED, fraction=FRACTION):
    """(training, held-out): the sequences' indices, in file order"""
    return mh.split(seed, 0, n, mh.threshold_of(fraction))


def sites_in(sites, indices):
    s = set(int(i) for i in indices)
    return [x for x in sites if x[0] in s]


def database(n_decoys=20):
    """(names, rows) of a small MEME database as tests/test_gpu_motif_enrich.py builds its own: decoys, then the word motifs"""
    return mc.planted_database(n_decoys=n_decoys)
