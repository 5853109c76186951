"""Seeded k-mer set families shared by the geometry tests (test_oracle_geometry_cpu.py, test_gpu_geometry.py).

The SPSS strings the oracle writes for a set depend on the set alone, not on its bucket geometry (N, key width):
the oracle iterates a set in ascending k-mer order, and bucket-major order is numeric order.  So one oracle run
per family, at a cheap reference geometry, is the expected answer at every geometry; test_oracle_geometry_cpu.py
pins that premise, test_gpu_geometry.py relies on it."""
import numpy as np

from kmersets import synth

U = np.uint64
CANONICAL = ("genome", "difference", "repeats", "random")
FAMILIES = CANONICAL + ("directed",)


def ref_geom(k):
    """The reference geometry of a family: (N, key bytes) with N = min(14, 2k - 1) and the narrowest key."""
    n = min(14, 2 * k - 1)
    kb = 2 * k - n
    return n, (1 if kb <= 8 else 2 if kb <= 16 else 4 if kb <= 32 else 8)


def self_rc(x, k):
    """Which k-mers equal their own reverse complement (even k only)."""
    return x == synth.revcomp(x, k)


def _random_kmers(k, size, seed, canonical):
    space = 4 ** k // (2 if canonical else 1)
    size = min(size, space // 4)
    x = synth.mix64(synth.mix64(U(seed)) + np.arange(4 * size + 64, dtype=U)) >> U(64 - 2 * k)
    if canonical:
        x = synth.canonical(x, k)
    return np.unique(x)[:size]


def family(name, k, size, seed):
    """Sorted unique uint64 k-mers of one family, about `size` of them (fewer where 4^k is small).
    genome: the canonical k-mers of a random genome; difference: A \\ B of two 2 %-diverged genomes (many short
    strings); repeats: a genome with planted repeats (branching unitigs); random: uniform canonical k-mers;
    directed: the forward k-mers of a genome plus uniform k-mers, not canonicalised (GetSPSS / GetUnitigs).
    The canonical families hold no k-mer equal to its own reverse complement (the encode refuses those)."""
    if 4 ** k // 2 < 4 * size:  # a small k: the genome families would saturate the space
        if name == "directed":
            return _random_kmers(k, size, seed + 7, canonical=False)
        x = _random_kmers(k, size, seed + CANONICAL.index(name), canonical=True)
    elif name == "genome":
        x = synth.phylogeny_sets(k, 1, size, seed)[0]
    elif name == "difference":
        a, b = synth.phylogeny_sets(k, 2, 2 * size, seed, rate=0.02)
        x = np.setdiff1d(a, b)
    elif name == "repeats":
        x = synth.phylogeny_sets(k, 1, size, seed, repeats=(max(3, size // 4000), 5))[0]
    elif name == "random":
        x = _random_kmers(k, size, seed, canonical=True)
    elif name == "directed":
        g = synth.random_genome(size // 2 + k - 1, 0x5EED0000 + seed)
        return np.unique(np.concatenate([synth.kmers_of_bases(g, k), _random_kmers(k, size // 2, seed, canonical=False)]))
    else:
        raise ValueError(name)
    x = np.asarray(x, dtype=U)
    return x[~self_rc(x, k)] if k % 2 == 0 else x


def oracle_answers(ol, name, k, kmers, n=None, kb=None):
    """The oracle's strings for a family at one geometry (the reference geometry by default): canonical families
    -> {"spss", "spss_slow", "unitigs"}; the directed family -> {"spss_directed", "unitigs_directed"}."""
    if n is None:
        n, kb = ref_geom(k)
    o = ol.Set.from_kmers(k, n, kb, kmers)
    if name == "directed":
        return {"spss_directed": o.spss_directed(), "unitigs_directed": o.unitigs_directed()}
    return {"spss": o.spss(), "spss_slow": o.spss_slow(), "unitigs": o.unitigs()}


def kmers_of_strings(strings, k, canonical):
    """The sorted unique k-mers of a list of strings (canonical forms or as written)."""
    if not strings:
        return np.zeros(0, dtype=U)
    bases = synth.bases_of_string("".join(strings))
    x = synth.kmers_of_bases(bases, k)
    # keep the windows that lie inside one string
    lens = np.array([len(s) for s in strings], dtype=np.int64)
    ends = np.cumsum(lens)
    start = np.arange(x.size, dtype=np.int64)
    x = x[np.searchsorted(ends, start, side="right") == np.searchsorted(ends, start + k - 1, side="right")]
    return np.unique(synth.canonical(x, k) if canonical else x)
