"""Seeded degenerate families for the KmerSetSet loop (test_loop_families_cpu.py, test_gpu_loop_families.py and
the workers of the multi-rank builds).

Every other loop test builds on synth.phylogeny_sets: independently mutated genomes of equal length, which never
tie at the arg-max, never leave an empty remainder, never see the total SPSS weight go up at a check and never
end on weight 0 after some merges.  The families here do: duplicates and nested inputs (empty j \\ n or k \\ n),
ties that only std::map order decides, empty inputs, one input, more sets (an interval of 4 and 6), and fewer
inputs than a multi-rank build has ranks.  test_loop_families_cpu.py pins, on the oracle alone, that each family
still is what its comment says."""
import numpy as np

from kmersets import synth

U = np.uint64
E = np.zeros(0, dtype=U)

# name -> at least this many empty nodes in the oracle's structure (the families that are there for them)
MIN_EMPTY_NODES = {"two_identical": 2, "three_identical": 4, "dups_of_two": 6, "empties_among": 2, "nested_chain": 1,
                   "star": 7}
# at least two initial weights equal the maximum: only the order of the weight table decides the first merge
TIED = ("three_identical", "dups_of_two", "permuted_ties", "star")

FAMILIES = ("one_input", "two_identical", "three_identical", "dups_of_two", "all_empty", "empties_among",
            "nested_chain", "two_clusters", "permuted_ties", "star", "many_small_24", "many_small_40", "sampled_23",
            "dups_31")


def _union(*parts):
    return np.unique(np.concatenate(parts))


def _sets(name):
    if name in ("sampled_23", "dups_31"):
        raise ValueError(name)
    k = 15
    P = synth.phylogeny_sets(k, 4, 6000, seed=3)
    if name == "one_input":
        return [P[0]]
    if name == "two_identical":
        return [P[0], P[0]]
    if name == "three_identical":
        return [P[0]] * 3
    if name == "dups_of_two":
        return [P[0], P[1], P[0], P[1], P[0]]
    if name == "all_empty":
        return [E, E, E]
    if name == "empties_among":
        return [E, P[0], E, P[1], P[2]]
    if name == "nested_chain":
        return [P[0][:m] for m in (6000, 4500, 3000, 1500, 1)]
    if name == "two_clusters":
        return synth.phylogeny_sets(k, 3, 4000, seed=5) + synth.phylogeny_sets(k, 3, 4000, seed=6)
    if name == "permuted_ties":
        B = synth.uniform_pair(k, 12000, 0.0, seed=11)[0]
        b = [B[i * 1000:(i + 1) * 1000] for i in range(12)]
        return [b[9], _union(b[0], b[1]), _union(b[3], b[4]), _union(b[3], b[5]), _union(b[0], b[2])]
    if name == "star":
        X = synth.uniform_pair(k, 9000, 0.0, seed=9)[0]
        return [_union(P[3][:2000], X[i * 1000:(i + 1) * 1000]) for i in range(9)]
    if name == "many_small_24":
        return synth.phylogeny_sets(k, 24, 1500, seed=24, rate=0.01)
    if name == "many_small_40":
        return synth.phylogeny_sets(k, 40, 1500, seed=40, rate=0.01)
    raise ValueError(name)


def family(name):
    """(k, n, key_bytes, sets, bucket_ids): sets is a list of sorted uint64 arrays of canonical k-mers."""
    if name == "sampled_23":
        Q = synth.phylogeny_sets(23, 2, 30000, seed=5)
        return 23, 14, 4, [Q[0], Q[1], Q[0], Q[1][:len(Q[1]) // 2], E], synth.sample_bucket_ids(14, seed=6)
    if name == "dups_31":
        R = synth.phylogeny_sets(31, 2, 20000, seed=7)
        return 31, 14, 8, [R[0], R[0], R[1]], synth.sample_bucket_ids(14, seed=6)
    sets = [np.ascontiguousarray(s, dtype=U) for s in _sets(name)]
    return 15, 10, 4, sets, np.arange(1 << 10, dtype=np.int32)


def oracle_build(ol, name):
    """The oracle's structure of a family: (k, n, key_bytes, sets, ids, osets, ocompacts, okss)."""
    k, n, kb, sets, ids = family(name)
    osets = [ol.Set.from_kmers(k, n, kb, s) for s in sets]
    ocompacts = [s.compact() for s in osets]
    return k, n, kb, sets, ids, osets, ocompacts, ol.KmerSetSet(ocompacts, ids)
