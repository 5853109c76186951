"""The cells, fabricated structures, requests and route models of the index geometry sweep, shared by
test_index_reference_cpu.py (which checks on the CPU that every structure discriminates) and
test_gpu_index_geometry.py (which runs the seven index calls on them).  numpy only.

A case is (cell, plain): the cell (k, N, key bytes) and whether the structure is the plain one (k-mers as written,
canonical=False / canonicalize=False) or the canonical one."""
import numpy as np

import geometry_families as gf
from index_reference import revcomp_string
from kmersets import synth
from test_gpu_geometry import CELLS, FAMILY_SEED, size_of

U = np.uint64

# Extra cells, local to the index sweep:
DENSE = (8, 1, 2)       # plain and dense: all 4^8 8-mers in two buckets of 2^15 keys.  A u16 slice of 32768 keys is
                        # 64 KiB, above the join's 32 KiB LDS stage (OVERSIZE with 2-byte keys), and every bucket is
                        # cut hundreds of times with 15 key bits; the expectations follow from the moduli
WIDEST = (31, 1, 8)     # 61 key bits in two buckets: the widest key span a tile cut can meet
ONE_BIT_WIDE = (12, 23, 2)  # one key bit at 2^23 buckets
EXTRA = [DENSE, WIDEST, ONE_BIT_WIDE]

FULL_WIDTH = [c for c in CELLS if 2 * c[0] - c[1] == 8 * c[2]]  # the all-ones key fills the key type
# the plain structure: at the full-width-key cells, at one cell per key width, at the extra cells
PLAIN_CELLS = FULL_WIDTH + [(7, 1, 2), (16, 2, 4), (23, 1, 8)] + EXTRA
CASES = [(c, False) for c in CELLS + [WIDEST, ONE_BIT_WIDE]] + [(c, True) for c in PLAIN_CELLS]
K3_CELLS = [c for c in CELLS if c[0] < 4]  # seq_hits refuses these; the other four calls serve them
BORROWED_CELLS = [(7, 7, 2), (16, 2, 4), (23, 24, 4)]


def case_id(case):
    (k, n, kb), plain = case
    return "k%d-N%d-u%d-%s" % (k, n, 8 * kb, "plain" if plain else "canon")


# The tile walk (csrc/ksh_rowtile.h) starts one workgroup per 8192 entries, and a workgroup walks its share of all 2^N
# buckets whatever they hold.  At N >= 22 a pool of size_of(k) would leave 2^N buckets to 7 workgroups or fewer, so
# those cells take a larger pool: about 2.75 entries per pool k-mer, 60 workgroups and more.
LARGE_N, LARGE_N_POOL, LARGE_N_MIN_ENTRIES = 22, 200000, 130000


def pool_size(k, n):
    return size_of(k) if n < LARGE_N else max(size_of(k), LARGE_N_POOL)


CHILDREN = [[4, 5], [4, 6], [5], [], [6], [], []]  # 4, 5 and 6 are shared children
N_NODES = 7
WHOLE, EMPTY_NODE, TWINS = 3, 5, (2, 6)  # the node with the whole pool, the empty node, the two with the same set
NONEMPTY = [0, 1, 2, 3, 4, 6]
PERMUTED = [6, 5, 0, 3, 4]  # a permuted subset with the empty node and the internal nodes 0 and 4
# the three select requests: the core of the non-empty columns, private to node 0 among {0, 1, 2}, Get(0) & Get(3)
# \ Get(4)
SELECTS = [dict(cols=NONEMPTY, min_count=len(NONEMPTY)),
           dict(cols=[0, 1, 2], require=[0], max_count=1),
           dict(cols=PERMUTED, require=[0, 3], exclude=[4])]
# The three class-id requests.  Each of SELECTS picks k-mers of a single class on every fabricated structure, so a
# constant id array would pass on them; these pick several classes of which none holds more than half the selection
# (test_index_reference_cpu.py asserts it per case): (a) the union over all seven nodes, the identity column list;
# (b) the union over the permuted subset, whose rows project; (c) a proper subset, Get(0).
CLASS_REQUESTS = [dict(cols=None), dict(cols=PERMUTED), dict(cols=None, require=[0])]

# The pool without its smallest and largest k-mer (the sentinels, which every non-empty node gets) is dealt into seven
# parts by the rank of each k-mer in a seeded permutation, rank % 16 -> part.  The first six ranks fill the parts the
# checks need (the core, A0, A1, REST and BOTH01 twice), so that the pool of eight 3-mers still discriminates (classes
# of 3, 2 and 1 k-mers); over 16 ranks the parts take 3, 1, 1, 3, 4, 2 and 2, so that the colour classes have distinct sizes.
# BOTH01 is in nodes 0 and 1 and not in their common child: Get(0) & Get(1) is no other column's set.
CORE, A0, A1, TWIN, A4, REST, BOTH01 = range(7)
PART_OF_RANK = np.array([CORE, A0, A1, REST, BOTH01, BOTH01, A4, TWIN, CORE, TWIN, A4, REST, CORE, TWIN, A4, A4])
PARTS_OF_NODE = [(CORE, A0, BOTH01), (CORE, A1, BOTH01), (CORE, TWIN), tuple(range(7)), (CORE, A4), (), (CORE, TWIN)]
DENSE_MODULI = [2, 3, 5, 1, 7, 0, 5]  # the dense cell: node i holds the 8-mers x with x % m == 0 (0: empty)

_pools = {}


def pool_of(k, n):
    key = (k, pool_size(k, n))
    if key not in _pools:
        _pools[key] = gf.family("genome", k, key[1], seed=FAMILY_SEED + k)
    return _pools[key]


def plain_sentinels(k, n):
    """Key 0 and the all-ones key in the first and in the last bucket."""
    key_bits = 2 * k - n
    return np.array([0, (1 << key_bits) - 1, 4 ** k - (1 << key_bits), 4 ** k - 1], dtype=U)


def fabricate(case):
    """The node sets (sorted unique uint64) of a case; the children are CHILDREN."""
    (k, n, kb), plain = case
    if case == (DENSE, True):
        # (no sentinels: node 3 holds all four already, and the closed forms stay those of the moduli)
        every = np.arange(4 ** k, dtype=U)
        return [every[every % U(m) == 0] if m else every[:0] for m in DENSE_MODULI]
    pool = pool_of(k, n)
    inner = pool[1:-1]
    order = np.argsort(synth.mix64(np.arange(inner.size, dtype=U) + U(1000 * k + n)), kind="stable")
    rank = np.empty(inner.size, dtype=np.int64)
    rank[order] = np.arange(inner.size)
    part = PART_OF_RANK[rank % 16]
    sentinels = np.concatenate([pool[:1], pool[-1:], plain_sentinels(k, n) if plain else pool[:0]])
    return [np.unique(np.concatenate([inner[np.isin(part, parts)], sentinels])) if parts else pool[:0]
            for parts in PARTS_OF_NODE]


def count_multiples(moduli, limit):
    """|{x in [0, limit): some m of moduli divides x}| by inclusion and exclusion."""
    total = 0
    for pick in range(1, 1 << len(moduli)):
        chosen = [m for i, m in enumerate(moduli) if pick >> i & 1]
        total += (-1) ** (len(chosen) + 1) * ((limit - 1) // int(np.lcm.reduce(chosen)) + 1)
    return total


SLICE_BYTES = 32 << 10  # kSliceBytes of csrc/ksh_query.hip: the join stages a slice of at most this many bytes
TILE = 512              # kTile of csrc/ksh_rowtile.h: a bucket of more entries (all nodes together) is cut


def route_model(case, node_sets):
    """The largest total of entries in one bucket (all nodes together) and the largest slice of one node in one
    bucket in bytes, and what follows for the routes: the tile walk cuts a bucket iff its entries exceed kTile
    (pc_tile_cut: left > kTile on the bucket's first tile); the join searches a slice in HBM iff its keys exceed
    kSliceBytes / sizeof(KeyT) (k_query_join: len <= kSliceKeys is staged), i.e. its bytes exceed kSliceBytes."""
    (k, n, kb), _ = case
    shift = U(2 * k - n)
    buckets = [(s >> shift) for s in node_sets if s.size]
    largest_slice = max(int(np.unique(b, return_counts=True)[1].max()) for b in buckets)
    largest_bucket = int(np.unique(np.concatenate(buckets), return_counts=True)[1].max())
    return {"largest_bucket": largest_bucket, "largest_slice_bytes": largest_slice * kb,
            "total_entries": int(sum(s.size for s in node_sets)),
            "pair_split": largest_bucket > TILE, "oversize": largest_slice * kb > SLICE_BYTES}


def kmer_strings(kmers, k):
    return ["".join("ACGT"[(int(x) >> (2 * (k - 1 - j))) & 3] for j in range(k)) for x in kmers]


def absent_kmers(ref, count, canonical, seed):
    """Up to `count` distinct 2K-bit patterns (canonical forms if asked) that the structure does not hold."""
    x = synth.mix64(np.arange(2 * count + 64, dtype=U) + U(seed)) >> U(64 - 2 * ref.k)
    if canonical:
        x = synth.canonical(x, ref.k)
    x = np.unique(x)
    return x[~np.isin(x, ref.kmers)][:count]


def queries_of(ref, plain, seed, limit=None):
    """All distinct k-mers (every limit-th share of them where the batch has to stay small), their reverse
    complements, as many absent k-mers again, and three patterns with a bit at or above 2K."""
    k = ref.k
    have = ref.kmers if limit is None else ref.kmers[::max(1, ref.kmers.size // limit)]
    high = np.array([int(ref.kmers[0]) | 1 << (2 * k), int(ref.kmers[-1]) | 1 << 63, 1 << (2 * k)], dtype=U)
    return np.concatenate([have, synth.revcomp(have, k), absent_kmers(ref, have.size, not plain, seed), high])


def sequences_of(ref, plain, seed):
    """Strings of exactly K bases (members and absent k-mers), one random string of 3000 bases, and one whose k-mers
    repeat (a member three times over: the windows at 0, K and 2K are the same k-mer)."""
    k = ref.k
    some = ref.kmers[::max(1, ref.kmers.size // 16)][:16]
    single = kmer_strings(np.concatenate([some, absent_kmers(ref, 4, not plain, seed)]), k)
    random = synth.string_of_bases(synth.random_genome(3000, seed))
    repeat = kmer_strings(ref.kmers[ref.kmers.size // 2:][:1], k)[0] * 3
    return single + [random, repeat]


PAINT_CUT = 400  # positions kept of each of the longest strings


def cut_strings(whole_strings, k):
    """The 6 longest strings and the 4 shortest of the others (ties by the text), each cut to at most PAINT_CUT
    positions: a genome's pool makes a handful of strings of 10^4 positions and more, the shortest among them.
    Where there are fewer than 6 strings, later windows of the longest one, a sixth of it apart, make up the 6."""
    by_len = sorted(whole_strings, key=lambda s: (len(s), s))
    longest = by_len[::-1][:6]
    for j in range(1, 7 - len(longest)):
        a = j * (len(longest[0]) - k + 1) // 6
        longest.append(longest[0][a:])
    return [s[:PAINT_CUT + k - 1] for s in longest + by_len[:-6][:4]]


def paint_strings(whole_strings, ref, plain, seed):
    """The strings a case paints: cut_strings of `whole_strings` -- the strings of node WHOLE as the test's own
    encode made them: that node holds the whole pool, so its strings pass through k-mers of every part -- the
    reverse complements of all ten, and sequences_of.  About 10^4 positions at the most."""
    cut = cut_strings(whole_strings, ref.k)
    return cut + [revcomp_string(s) for s in cut] + sequences_of(ref, plain, seed)


def paint_strings_for_passes(whole_strings, ref, plain, seed):
    """The strings painted in passes of 7 and of 257 positions: sequences_of with its random string cut to 400
    positions, and the two longest cut strings at 250 positions each: at most 1000 positions and more than 257 (a
    pass of 7 positions over more would be thousands of launches)."""
    k = ref.k
    few = sequences_of(ref, plain, seed)
    few[-2] = few[-2][:400 + k - 1]
    return few + [s[:250 + k - 1] for s in cut_strings(whole_strings, k)[:2]]
