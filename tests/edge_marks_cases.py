"""Sets for the edge search of the SPSS encode (k_edges / k_link_cut's cut marks, csrc/ksh_encode.hip), shared by
tests/test_gpu_edge_marks.py and its CPU twin tests/test_edge_marks_model_cpu.py (test infrastructure).

A unitig side takes one of three branches in k_edges:
  dead : its link entry is `none` and k_link_cut left no mark -- the side never had a neighbour: four `none`, no search;
  cut  : `none` and marked -- it had neighbours and lost the link: searched;
  live : a link at a unitig end (a non-branching loop spelled from its smallest k-mer): searched.
Every set here has 2 000 to 20 000 k-mers."""
import numpy as np

from kmersets import synth

U = np.uint64

GEOMS = ((23, 14, 4), (15, 14, 2), (31, 14, 8))  # (k, bucket bits, key bytes)


def _stretch_kmers(pieces, k, canonical=True):
    allk = np.concatenate([synth.kmers_of_bases(p, k) for p in pieces])
    return np.unique(synth.canonical(allk, k) if canonical else allk)


def chains(k, seed=3):
    """200 disjoint non-branching stretches of 23 to 60 k-mers cut from one random sequence (k bases dropped
    between two stretches, so that no k-mer spans a cut): every unitig side is a dead end."""
    lens = 23 + (synth.mix64(U(seed) * U(977) + np.arange(200, dtype=U)) % U(38)).astype(np.int64)
    g = synth.random_genome(int(lens.sum()) + 200 * (2 * k - 1), 0xED6E0000 + seed)
    pieces, at = [], 0
    for ln in lens.tolist():
        pieces.append(g[at:at + ln + k - 1])
        at += ln + 2 * k - 1
    return _stretch_kmers(pieces, k)


def _incoming_stretches(bases, k, every, seed, count=24):
    """Stretches of new bases that run INTO the sequence: the last k-mer of a stretch is c + bases[p : p + k - 1]
    with c another base than bases[p - 1], so the k-mer at p has two neighbours on its entering side and the
    stretch's last k-mer has that k-mer as its single neighbour: the k-mer at p cuts the facing entry, and it is
    that k-mer's thread -- not the side's own -- that marks it."""
    out = []
    for j in range(count):
        p = every * (j + 1) + every // 2 + 3
        if p + k - 1 > bases.size:
            break
        tail = synth.random_genome(23 + (j * 5) % 18, 0x1AC00000 + (seed << 8) + j)
        c = np.array([(int(bases[p - 1]) + 1 + j % 3) & 3], dtype=np.uint8)
        out.append(np.concatenate([tail, c, bases[p:p + k - 1]]))
    return out


def fork_pieces(k, name):
    """The sequences behind the two sets of test_encode_branching_sets' generator at a tenth of the size -- `tips`: a
    genome with one-k-mer tips every 150 k-mers; `bubbles`: two diverged copies of a genome -- plus the
    incoming stretches above."""
    if name == "tips":
        size, seed, every = 9000, 7, 150
        bases = synth.random_genome(size + k - 1, 0x5EED0000 + seed)
        pos = np.arange(0, size - 1, every)
        keep = bases[pos + k] != 3
        tips = [np.concatenate([bases[p:p + k][1:], np.array([3], dtype=np.uint8)]) for p in pos[keep].tolist()]
        return [bases] + tips + _incoming_stretches(bases, k, every, seed)
    a, b = synth.phylogeny_genomes(2, 6000 + k - 1, 77, rate=0.004)
    return [a, b] + _incoming_stretches(a, k, 150, 78)


def fork(k, name, canonical=True):
    return _stretch_kmers(fork_pieces(k, name), k, canonical)


def _with_indels(bases, seed):
    """Three one-base deletions and three one-base insertions at seeded places."""
    r = synth.mix64(U(seed) * U(31) + np.arange(6, dtype=U))
    out = bases
    for i, x in enumerate(sorted((int(v) % (bases.size - 200) + 100 for v in r), reverse=True)):
        out = np.delete(out, x) if i % 2 else np.insert(out, x, (int(out[x]) + 1) & 3)
    return out


def mutated_pair(k, seed=5):
    """(remainder, intersection) of the canonical k-mer sets of two mutated copies of one 20 000-base sequence (1 % of
    the bases substituted in each, a few indels): the remainder is stretches of about k k-mers whose ends' neighbours
    went to the intersection, the intersection ends where one copy's k-mer is missing."""
    g = synth.random_genome(20000, 0x5EED0000 + seed)
    a = _with_indels(synth.mutate(g, 0.01, (seed << 20) + 1), seed)
    b = _with_indels(synth.mutate(g, 0.01, (seed << 20) + 2), seed + 1)
    sa, sb = synth.canonical_set_of_bases(a, k), synth.canonical_set_of_bases(b, k)
    inter = np.intersect1d(sa, sb)
    return np.setdiff1d(sa, inter), inter


def loop_with_tails_elsewhere(k, seed=11):
    """A non-branching loop of 3 000 k-mers (nothing hangs off it: the encode takes its stamped second pass, and both
    ends of the loop's unitig hold a live link) beside a genome with tips."""
    g = synth.random_genome(3000, 0xC1AC0000 + seed)
    loop = synth.canonical_set_of_bases(np.concatenate([g, g[:k - 1]]), k)
    return np.union1d(loop, fork(k, "tips"))


def cases():
    """[(name, k, bucket bits, key bytes, k-mers, canonical, mode, oracle method)], in a fixed order."""
    out = []
    for (k, n, kb) in GEOMS:
        tag = "k%d" % k
        out.append(("chains-" + tag, k, n, kb, chains(k), True, 0, "spss"))
        out.append(("fork-tips-" + tag, k, n, kb, fork(k, "tips"), True, 0, "spss"))
        out.append(("fork-bubbles-" + tag, k, n, kb, fork(k, "bubbles"), True, 0, "spss"))
        rem, inter = mutated_pair(k)
        out.append(("remainder-" + tag, k, n, kb, rem, True, 0, "spss"))
        out.append(("intersection-" + tag, k, n, kb, inter, True, 0, "spss"))
    k, n, kb = GEOMS[0]
    out.append(("loop-k23", k, n, kb, loop_with_tails_elsewhere(k), True, 0, "spss"))
    out.append(("directed-tips-k23", k, n, kb, fork(k, "tips", canonical=False), False, 0, "spss_directed"))
    out.append(("slow-tips-k23", k, n, kb, fork(k, "tips"), True, 2, "spss_slow"))
    out.append(("slow-bubbles-k23", k, n, kb, fork(k, "bubbles"), True, 2, "spss_slow"))
    return out
