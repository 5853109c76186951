"""Designed inputs for the library's lock-free open-addressing tables, with a numpy model of where every key lands:
the class table (cls_insert / cls_find of csrc/ksh_clstable.h: a workgroup's table in LDS and the global table of
ksh_kss_color_classes, the caller's table of ksh_kss_select_class_ids and ksh_seq_class_runs), the end table of
ksh_spss_links (link_insert / link_find of csrc/ksh_links.hip) and the tile table of the index walk (pc_tile_fill of
csrc/ksh_rowtile.h).  Shared by test_hash_table_model_cpu.py, which asserts by predicate that every case is what it
claims, and test_gpu_hash_tables.py, which runs the public calls on them.  numpy only.

The model (pc_mix, cls_hash, the three key words, link_slot, the tile home, the table sizes) says where things land.
It is never an expected answer: those come from tests/index_reference.py, tests/paint_reference.py and
tests/spss_links_reference.py.  Its constants are read from the kernels' text, and the lines it restates must stand
there as written (constants()): a changed constant or hash fails the CPU test instead of moving the cases off their
collisions silently.

Concurrent lanes insert in no fixed order, so the cases state only what holds for every order:
  - the set of occupied slots of a linear-probing table does not depend on the order of insertion (occupied());
  - g keys with one home are displaced by at least 0, 1, ..., g - 1 slots, whoever wins: the keys met on the way are
    exactly the other keys of the group (and whatever lay in the run before);
  - how many keys pass the table's last slot is the number of keys whose home lies in the run that ends there less
    the slots of that run up to the last one: a property of the occupied set (wrapped()).
Rows that share the low 63 bits of r0 share key word 0 of the class table, so every meeting of two of them in a
probe chain is a partial-key match: the rows of the class families are (x, y) with one x throughout."""
import os
import re
from collections import namedtuple

import numpy as np

import spss_links_cases as lc
import spss_links_reference as lref
from kmersets import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmer-sets-compression_amd", "csrc")
FILES = {"rowtile": "ksh_rowtile.h", "rowtile_host": "ksh_rowtile.hip", "clstable": "ksh_clstable.h",
         "classes": "ksh_classes.hip", "classids": "ksh_classids.hip", "links": "ksh_links.hip"}
U = np.uint64
B63 = 1 << 63
M64 = (1 << 64) - 1


# ---- constants from the kernels' text --------------------------------------------------------------------------------
def sources():
    return {name: open(os.path.join(CSRC, f)).read() for name, f in FILES.items()}


# anchored patterns with one number each: (constant, file, pattern, base); each must match exactly once
NUMBERS = (
    ("shift_a", "rowtile", r"^__device__ __forceinline__ uint64_t pc_mix\(uint64_t x\) \{[^\n]*\n  x \^= x >> (\d+);\n"
                           r"  x \*= 0x[0-9A-F]+ull;\n", 10),
    ("mul_a", "rowtile", r"^  x \^= x >> 29;\n  x \*= 0x([0-9A-F]+)ull;\n  x \^= x >> 32;\n", 16),
    ("shift_b", "rowtile", r"^  x \*= 0xBF58476D1CE4E5B9ull;\n  x \^= x >> (\d+);\n", 10),
    ("mul_b", "rowtile", r"^  x \^= x >> 32;\n  x \*= 0x([0-9A-F]+)ull;\n  x \^= x >> 29;\n  return x;\n", 16),
    ("shift_c", "rowtile", r"^  x \*= 0x94D049BB133111EBull;\n  x \^= x >> (\d+);\n  return x;\n", 10),
    ("gold", "clstable", r"^  return uint32_t\(pc::pc_mix\(r0 \^ pc::pc_mix\(r1 \+ 0x([0-9A-F]+)ull\)\)\);$", 16),
    ("valid_bit", "clstable", r"^constexpr unsigned long long kValid = 1ull << (\d+);", 10),
    ("cls_slots", "classes", r"^constexpr int kClsSlots = (\d+);", 10),
    ("tile", "rowtile", r"^constexpr int kTile = (\d+);", 10),
    ("rows_per_group", "rowtile", r"^constexpr int64_t kRowsPerGroup = (\d+);", 10),
    ("threads", "rowtile", r"^constexpr int kThreads = (\d+);", 10),
    ("global_floor", "classes", r"^  int64_t slots = (\d+);\n  while \(slots < 2 \* capacity\) slots <<= 1;", 10),
    ("global_factor", "classes", r"^  while \(slots < (\d+) \* capacity\) slots <<= 1;", 10),
    ("caller_floor", "classids", r"^  int64_t slots = (\d+);\n  while \(slots < 2 \* n_classes\) slots <<= 1;", 10),
    ("caller_factor", "classids", r"^  while \(slots < (\d+) \* n_classes\) slots <<= 1;", 10),
    ("link_floor", "links", r"^  uint64_t slots = (\d+);\n  while \(slots < 4 \* uint64_t\(n\)\) slots <<= 1;", 10),
    ("link_factor", "links", r"^  while \(slots < (\d+) \* uint64_t\(n\)\) slots <<= 1;", 10),
)
# the lines the model restates: (file, line, how often it stands there)
RESTATED = (
    ("rowtile", "  x ^= x >> 29;", 2),
    ("rowtile", "  x *= 0xBF58476D1CE4E5B9ull;", 1),
    ("rowtile", "  x ^= x >> 32;", 1),
    ("rowtile", "  x *= 0x94D049BB133111EBull;", 1),
    ("clstable", "  return uint32_t(pc::pc_mix(r0 ^ pc::pc_mix(r1 + 0x9E3779B97F4A7C15ull)));", 1),
    # cls_insert and cls_find form the key words alike, start alike and step alike
    ("clstable", "  const unsigned long long w0 = (r0 & ~kValid) | kValid, w1 = (r1 & ~kValid) | kValid;", 2),
    ("clstable", "  const unsigned long long w2 = (r0 >> 63) | ((r1 >> 63) << 1) | kValid;", 2),
    ("clstable", "  uint32_t h = cls_hash(r0, r1) & mask;", 2),
    ("clstable", "  for (uint32_t probe = 0; probe <= mask; probe++, h = (h + 1) & mask) {", 2),
    ("clstable", "    if (k0 == w0 && s[kPlane] == w1 && s[2 * kPlane] == w2) return s[3 * kPlane];", 1),
    ("classes", "constexpr int kClsSpill = kClsSlots * 3 / 4 - kTile;  // spill above this: the next tile's <= kTile "
                "new classes", 1),
    ("classes", "      if (!cls_insert<1, kClsSlots>(c_tab, kClsSlots - 1, s.r0, s.r1, static_cast<unsigned long long>"
                "(mine), &claims))", 1),
    ("classes", "  __device__ __forceinline__ void tile_done(int) { pending = s_ctl[0] > kClsSpill; }", 1),
    ("classes", "                     ClassConsumer{g_tab, uint32_t(slots - 1), capacity, ctl});", 1),
    ("classids", "      const unsigned long long v = cls_find<4, 1>(g_tab, g_mask, s.r0, s.r1);", 1),
    ("rowtile", "constexpr int kSlots = 2 * kTile;      // table slots: at most half load (a single-key tile fills "
                "one slot)", 1),
    ("rowtile", "    uint32_t h = uint32_t(pc_mix(key)) & (kSlots - 1);", 1),
    ("rowtile", "      h = (h + 1) & (kSlots - 1);", 1),
    ("rowtile", "  if (left <= kTile) {", 1),
    ("rowtile_host", "  const int64_t want = (x.total_keys + kRowsPerGroup - 1) / kRowsPerGroup;", 1),
    ("rowtile_host", "  *grid = unsigned(std::max<int64_t>(1, std::min({want, int64_t(n_buckets(&x.g)), "
                     "per_cu * n_cu})));", 1),
    ("links", "__device__ __forceinline__ uint64_t link_slot(uint64_t key, uint64_t mask) { return pc::pc_mix(key) & "
              "mask; }", 1),
    ("links", "  uint64_t h = link_slot(key, mask);", 2),
    ("links", "  for (uint64_t probe = 0; probe <= mask; probe++, h = (h + 1) & mask) {", 2),
    ("links", "    if (r < x) {", 1),
    ("links", "                     n, k, canon, ends, tab, slots - 1, bad);", 1),
)

Consts = namedtuple("Consts", [name for name, _, _, _ in NUMBERS])


def anchor_counts(src=None):
    """How often every anchor stands in its file: [(what, found, wanted)]."""
    src = src or sources()
    out = [(name, len(re.findall(pat, src[f], flags=re.M)), 1) for name, f, pat, _ in NUMBERS]
    out += [(line, src[f].count(line), times) for f, line, times in RESTATED]
    return out


def constants(src=None):
    src = src or sources()
    for what, found, wanted in anchor_counts(src):
        assert found == wanted, "the kernels' text has %d x (wanted %d x): %s" % (found, wanted, what)
    return Consts(*[int(re.search(pat, src[f], flags=re.M).group(1), base) for _, f, pat, base in NUMBERS])


C = constants()
CLS_SLOTS = C.cls_slots                       # slots of a workgroup's class table
CLS_SPILL = C.cls_slots * 3 // 4 - C.tile     # kClsSpill, as its line states it
TILE = C.tile
TILE_SLOTS = 2 * C.tile                       # kSlots
assert C.valid_bit == 63 and (CLS_SLOTS, TILE_SLOTS) == (1024, 1024) and CLS_SPILL == 256


# ---- the model -------------------------------------------------------------------------------------------------------
def pc_mix(x, c=C):
    """pc_mix of csrc/ksh_rowtile.h over a uint64 array (wrapping arithmetic)."""
    x = np.array(x, dtype=U, copy=True)
    with np.errstate(over="ignore"):
        x ^= x >> U(c.shift_a)
        x *= U(c.mul_a)
        x ^= x >> U(c.shift_b)
        x *= U(c.mul_b)
        x ^= x >> U(c.shift_c)
    return x


def pc_mix_int(x, c=C):
    """The same on one Python integer."""
    x &= M64
    x ^= x >> c.shift_a
    x = (x * c.mul_a) & M64
    x ^= x >> c.shift_b
    x = (x * c.mul_b) & M64
    x ^= x >> c.shift_c
    return x


def cls_hash(r0, r1, c=C):
    """uint32(pc_mix(r0 ^ pc_mix(r1 + gold))) of rows given as uint64 arrays (or scalars)."""
    with np.errstate(over="ignore"):
        inner = pc_mix(np.asarray(r1, dtype=U) + U(c.gold), c)
    return (pc_mix(np.asarray(r0, dtype=U) ^ inner, c) & U(0xFFFFFFFF)).astype(np.int64)


def key_words(r0, r1):
    """(w0, w1, w2) of one row, Python integers: 63 bits of r0, 63 bits of r1, the two top bits, each with kValid."""
    r0, r1 = int(r0), int(r1)
    return (r0 & ~B63 & M64) | B63, (r1 & ~B63 & M64) | B63, (r0 >> 63) | ((r1 >> 63) << 1) | B63


def pow2_at_least(floor, need):
    slots = floor
    while slots < need:
        slots <<= 1
    return slots


def global_slots(capacity, c=C):
    return pow2_at_least(c.global_floor, c.global_factor * capacity)


def caller_slots(n_classes, c=C):
    return pow2_at_least(c.caller_floor, c.caller_factor * n_classes)


def link_slots(n_strings, c=C):
    return pow2_at_least(c.link_floor, c.link_factor * n_strings)


def row_homes(rows, slots):
    """The home of every row of uint64[n, 2] in a class table of `slots` slots."""
    rows = np.ascontiguousarray(rows, dtype=U).reshape(-1, 2)
    return cls_hash(rows[:, 0], rows[:, 1]) & (slots - 1)


def link_homes(keys, slots):
    return (pc_mix(np.asarray(keys, dtype=U)) & U(slots - 1)).astype(np.int64)


def tile_homes(keys):
    return ((pc_mix(np.asarray(keys, dtype=U)) & U(0xFFFFFFFF)) & U(TILE_SLOTS - 1)).astype(np.int64)


def occupied(homes, slots):
    """The occupied slots after the distinct keys with these homes are inserted by linear probing: bool[slots].  The
    set is the same for every order of insertion; this takes the given one."""
    occ = np.zeros(slots, dtype=bool)
    for h in homes:
        h = int(h)
        while occ[h]:
            h = (h + 1) & (slots - 1)
        occ[h] = True
    return occ


def run_of(occ, slot):
    """(start, length) of the cyclic run of occupied slots that holds `slot` (length 0 if it is empty)."""
    n = occ.size
    if not occ[slot]:
        return slot, 0
    if occ.all():
        return 0, n
    start = slot
    while occ[(start - 1) % n]:
        start = (start - 1) % n
    length = 0
    while occ[(start + length) % n]:
        length += 1
    return start, length


def wrapped(homes, slots):
    """How many keys are stored past the table's last slot (at a slot below their home), whoever wins."""
    occ = occupied(homes, slots)
    start, length = run_of(occ, slots - 1)
    if length == 0 or start + length <= slots:
        return 0
    return start + length - slots


def shared_homes(homes):
    """{home: how many keys} of the homes that more than one key has."""
    u, c = np.unique(np.asarray(homes), return_counts=True)
    return {int(h): int(n) for h, n in zip(u, c) if n > 1}


def popcount(x):
    return np.unpackbits(np.ascontiguousarray(x, dtype=U).view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1)


# ---- searchers -------------------------------------------------------------------------------------------------------
X0 = (1 << 9) | (1 << 41)  # the r0 of the class families: two columns, bit 63 free
DRAWS = 1 << 22


def sparse_words(rng, n, ands=3):
    """n seeded uint64 draws, the AND of `ands` uniform 63-bit words each: one column in 2^ands set, bit 63 clear (a
    row of few columns is a k-mer in few nodes: few index entries)."""
    y = rng.integers(0, 1 << 63, size=n, dtype=U)
    for _ in range(ands - 1):
        y &= rng.integers(0, 1 << 63, size=n, dtype=U)
    return y


Pool = namedtuple("Pool", "seed x y h both_r0 both_r1 y1")


def search_pool(seed=1, x=X0, draws=DRAWS):
    """The first seed from `seed` on whose `draws` sparse values y hold a y1 with (x, y1), (x | bit 63, y1) and
    (x, y1 | bit 63) on one home of the 1024-slot table.  h: the 32-bit hash of every (x, y); both_r0 / both_r1: the
    y whose row shares its home with the row that differs in bit 63 of r0 / of r1 alone."""
    for s in range(seed, seed + 64):
        rng = np.random.default_rng(s)
        y = sparse_words(rng, draws)
        y = y[y != 0]
        with np.errstate(over="ignore"):
            m = pc_mix(y + U(C.gold))
            m_top = pc_mix((y | U(B63)) + U(C.gold))
        h = (pc_mix(U(x) ^ m) & U(0xFFFFFFFF)).astype(np.int64)
        h_r0 = (pc_mix(U(x | B63) ^ m) & U(0xFFFFFFFF)).astype(np.int64)
        h_r1 = (pc_mix(U(x) ^ m_top) & U(0xFFFFFFFF)).astype(np.int64)
        mask = CLS_SLOTS - 1
        both_r0 = (h & mask) == (h_r0 & mask)
        both_r1 = (h & mask) == (h_r1 & mask)
        hit = np.flatnonzero(both_r0 & both_r1)
        if hit.size:
            return Pool(s, x, y, h, both_r0, both_r1, int(y[hit[0]]))
    raise AssertionError("no y1 from seed %d" % seed)


def pick(pool, slots, home, count, taken, most_bits=64):
    """`count` distinct y of the pool, none in `taken`, whose row (x, y) has `home` in a table of `slots` slots
    (home None: any): those of fewest columns first, then ascending."""
    cand = np.unique(pool.y[:1 << 16] if home is None else pool.y[(pool.h & (slots - 1)) == home])
    cand = cand[~np.isin(cand, np.array(sorted(taken), dtype=U))]
    cand = cand[popcount(cand) <= most_bits]
    cand = cand[np.lexsort((cand, popcount(cand)))]
    assert cand.size >= count, (slots, home, count)
    out = [int(v) for v in cand[:count]]
    taken.update(out)
    return out


_quads = {}


def search_quadruples(slots, seed=1, draws=1 << 20):
    """-> (x, y1, y2, y3) uint64 arrays: the drawn quadruples whose five rows (x, y1), (x, y2), (x | bit 63, y1),
    (x, y1 | bit 63) and (x, y3) have one home in a class table of `slots` slots."""
    if (seed, draws) not in _quads:  # (the draws and the two hashes that every candidate needs: once)
        rng = np.random.default_rng(seed)
        x, y1, y2, y3 = (sparse_words(rng, draws) for _ in range(4))
        _quads[(seed, draws)] = (x, y1, y2, y3, cls_hash(x, y1), cls_hash(x, y2))
    x, y1, y2, y3, h1, h2 = _quads[(seed, draws)]
    top = U(B63)
    home = h1 & (slots - 1)
    keep = np.flatnonzero(home == (h2 & (slots - 1)))
    for r0, r1 in ((x | top, y1), (x, y1 | top), (x, y3)):
        keep = keep[(cls_hash(r0[keep], r1[keep]) & (slots - 1)) == home[keep]]
    keep = keep[(x[keep] != 0) & (y1[keep] != y2[keep]) & (y1[keep] != y3[keep]) & (y2[keep] != y3[keep])
                & (y1[keep] != 0) & (y2[keep] != 0) & (y3[keep] != 0)]
    return x[keep], y1[keep], y2[keep], y3[keep]


def search_r0(r1, slots, seed, draws=1 << 20):
    """For a fixed r1 (the structures of 64 and 65 columns): (r0 values whose row shares its home in the workgroup's
    table with the row that differs in bit 63 of r0 alone, their hashes, all drawn r0, all hashes)."""
    rng = np.random.default_rng(seed)
    r0 = np.unique(sparse_words(rng, draws))
    r0 = r0[r0 != 0]
    h = cls_hash(r0, np.full(r0.size, r1, dtype=U))
    h_top = cls_hash(r0 | U(B63), np.full(r0.size, r1, dtype=U))
    both = ((h ^ h_top) & (CLS_SLOTS - 1)) == 0
    return r0[both], h[both], r0, h


# ---- fabricated structures: nodes without edges, column = node ------------------------------------------------------
def row_bits(rows, n_cols):
    rows = np.ascontiguousarray(rows, dtype=U).reshape(-1, 2)
    bits = np.unpackbits(rows.view(np.uint8).reshape(rows.shape[0], 16), axis=1, bitorder="little").astype(bool)
    assert not bits[:, n_cols:].any(), "a row has a bit at or above n_cols"
    return bits[:, :n_cols]


def sort_rows(rows):
    rows = np.ascontiguousarray(rows, dtype=U).reshape(-1, 2)
    return rows[np.lexsort((rows[:, 0], rows[:, 1]))]


def plain_keys(count, key_bits, salt):
    """`count` distinct seeded keys of key_bits bits."""
    keys = synth.mix64(np.arange(2 * count + 16, dtype=U) + U(salt << 20)) >> U(64 - key_bits)
    _, first = np.unique(keys, return_index=True)
    keys = keys[np.sort(first)][:count]
    assert keys.size == count
    return keys


def node_sets_of(kmers, row_of, rows, n_cols, perm=None):
    """Node perm[a] (a itself without perm) holds the k-mers whose row has bit a: sorted unique uint64 arrays."""
    bits = row_bits(rows, n_cols)[np.asarray(row_of)]
    kmers = np.asarray(kmers, dtype=U)
    assert np.unique(kmers).size == kmers.size
    out = [None] * n_cols
    for a in range(n_cols):
        out[a if perm is None else int(perm[a])] = np.sort(kmers[bits[:, a]])
    return out


def permutation(n_cols, seed=5):
    return [int(v) for v in np.random.default_rng(seed).permutation(n_cols)]


def place(rows, counts, k, n, buckets, salt):
    """(kmers, row_of): counts[r] k-mers of row r, k-mer number i of row r in bucket buckets(r, i), each with a
    distinct seeded key below it."""
    key_bits = 2 * k - n
    row_of = np.repeat(np.arange(len(counts)), counts)
    within = np.concatenate([np.arange(c) for c in counts]) if len(counts) else np.zeros(0, dtype=np.int64)
    keys = plain_keys(row_of.size, key_bits, salt)
    bucket = np.array([buckets(int(r), int(i)) for r, i in zip(row_of, within)], dtype=U)
    return (bucket << U(key_bits)) | keys, row_of


def entries_per_bucket(node_sets, k, n):
    every = np.concatenate([s for s in node_sets if s.size] or [np.zeros(0, dtype=U)])
    return np.bincount((every >> U(2 * k - n)).astype(np.int64), minlength=1 << n)


# ---- properties -----------------------------------------------------------------------------------------------------
SHARED_WG = "the rows (x, y1), (x, y2), (x | bit 63, y1), (x, y1 | bit 63) have one home in the workgroup's table"
WORD1_BRANCH = "two rows of one home that agree in key word 0 and differ in key word 1"
WORD2_R0 = "two rows of one home that differ only in bit 63 of r0 (column 63): key word 2 alone tells them apart"
WORD2_R1 = "two rows of one home that differ only in bit 63 of r1 (column 127): key word 2 alone tells them apart"
ONE_TILE = "every k-mer in one bucket of at most kTile entries: one tile, one slot round"
ONE_GROUP = "at most kRowsPerGroup entries: one workgroup walks every bucket"
WRAP_WG = "at least 4 rows whose home is the last slot of the workgroup's table"
WRAP_GLOBAL = "at least 3 rows whose home is the last slot of the global table"
SHARE3_GLOBAL = "at least 3 rows share a home of the global table"
EXACT_CAPACITY = "capacity equal to the number of classes"
SPILL = "more than kClsSpill classes in the workgroup's stream before its last bucket: the table spills"
SPILL_MERGE = "a designed row has k-mers before and behind the spill: its counts meet in the global table"
COLS_64 = "64 columns: bit 63 of r0 is the top column"
COLS_65 = "65 columns: r1 holds one column"
COLS_128 = "128 columns: bit 63 of r1 is the top column"
DISTINCT_COUNTS = "every class has a k-mer count of its own"
SHARED_CALLER = "four table rows with the partial-key matches on one home of the caller's table"
ABSENT_SHARED = "the data holds a row of that home that the table does not hold"
WRAP_CALLER = "at least 3 table rows whose home is the last slot of the caller's table"
ABSENT_LAST = "the data holds an absent row whose home is the last slot"
SHARE3_CALLER = "at least 3 table rows share a home of the caller's table"
TABLE_ONLY_ROWS = "the table holds rows that no k-mer has"
ALTERNATE_CHANGE = "neighbouring positions alternate between colliding rows of different classes"
ALTERNATE_SAME = "neighbouring positions alternate between colliding absent rows: the class does not change"
E_GROUP = "at least 3 ends that are link targets share one home"
E_MIXED = "that group holds flipped and unflipped owners, and a first, a last and a single end"
E_WRAP = "the occupied slots include the last slot and slot 0 in one run, with a link target in it"
E_SMALL = "2 to 4 strings: 8 or 16 slots"
E_ABSENT = "an extension that is no end has its home inside an occupied run of at least 3 slots"
E_MANY = "a few hundred strings with at least 10 shared homes and a wrap"
HAS_LINKS = "at least one link"
T_LAST = "at least 16 distinct keys whose home is the last slot of the tile table"
T_FIRST = "at least 16 distinct keys whose home is slot 0: one run wraps"
T_MULTI = "keys held by 2 to 7 nodes among both groups"
T_ONE_TILE = "one bucket of at most kTile entries"
T_CUT = "the same keys in a bucket of more than kTile entries: cut by key range"


# ---- the class families ---------------------------------------------------------------------------------------------
K_CLS, N_CLS = 15, 4
BUCKET = 5


def _designed():
    """The rows of the class families, from the pool's first seed: A .. D and E, F (one home H of the 1024-slot table,
    hence of every smaller one), W[0 .. 5] (home 1023, the last slot of every table up to 1024 slots), others."""
    pool = search_pool()
    x, y1 = pool.x, pool.y1
    home = int(cls_hash(U(x), U(y1))) & (CLS_SLOTS - 1)
    taken = {y1}
    y2, y3, y4 = pick(pool, CLS_SLOTS, home, 3, taken)
    w = pick(pool, CLS_SLOTS, CLS_SLOTS - 1, 6, taken)
    other = pick(pool, CLS_SLOTS, None, 24, taken, most_bits=4)
    rows = {"A": (x, y1), "B": (x, y2), "C": (x | B63, y1), "D": (x, y1 | B63), "E": (x, y3), "F": (x, y4)}
    rows.update({"W%d" % i: (x, v) for i, v in enumerate(w)})
    rows.update({"O%d" % i: (x, v) for i, v in enumerate(other)})
    return pool, home, rows


POOL, HOME, ROW = _designed()


def rows_of(names):
    return np.array([ROW[name] for name in names], dtype=U).reshape(-1, 2)


def counts_for(rows, base=1):
    """Distinct counts base, base + 1, ...: the rows of most columns get the smallest."""
    order = np.argsort(-popcount(rows[:, 0]) - popcount(rows[:, 1]), kind="stable")
    counts = np.zeros(rows.shape[0], dtype=np.int64)
    counts[order] = np.arange(base, base + rows.shape[0])
    return counts


def class_case(cid, family, rows, counts, covers, capacity=None, n_cols=128, buckets=None, salt=1):
    rows = np.ascontiguousarray(rows, dtype=U).reshape(-1, 2)
    assert np.unique(rows, axis=0).shape[0] == rows.shape[0], cid
    return {"id": cid, "family": family, "k": K_CLS, "n": N_CLS, "n_cols": n_cols, "rows": rows,
            "counts": np.asarray(counts, dtype=np.int64), "capacity": capacity or rows.shape[0],
            "buckets": buckets or (lambda r, i: BUCKET), "salt": salt, "covers": tuple(covers)}


def case_structure(case, perm=None):
    """(node_sets, kmers, row_of) of a class case."""
    kmers, row_of = place(case["rows"], case["counts"], case["k"], case["n"], case["buckets"], case["salt"])
    return node_sets_of(kmers, row_of, case["rows"], case["n_cols"], perm), kmers, row_of


def _count_cases():
    out = []
    small = {1: ["A"], 2: ["A", "B"], 3: ["A", "C", "D"], 4: ["A", "B", "C", "D"], 5: ["A", "B", "C", "D", "E"],
             8: ["A", "B", "C", "D", "E", "W0", "W1", "W2"], 9: ["A", "B", "C", "D", "E", "W0", "W1", "W2", "O0"]}
    for n, names in small.items():
        rows = rows_of(names)
        covers = [EXACT_CAPACITY, ONE_TILE, ONE_GROUP, DISTINCT_COUNTS, COLS_128]
        covers += [WORD1_BRANCH] if n in (2,) else []
        covers += [WORD2_R0, WORD2_R1] if n == 3 else []
        covers += [SHARED_WG, WORD1_BRANCH, WORD2_R0, WORD2_R1] if n >= 4 else []
        covers += [SHARE3_GLOBAL] if n >= 5 else []
        covers += [WRAP_GLOBAL] if n >= 8 else []
        out.append(class_case("small_%d" % n, "C-small", rows, counts_for(rows), covers, salt=10 + n))
    rows = rows_of(["A", "B", "C", "D", "E"])
    out.append(class_case("shared", "C-shared", rows, counts_for(rows, 2),
                          [SHARED_WG, WORD1_BRANCH, WORD2_R0, WORD2_R1, ONE_TILE, ONE_GROUP, DISTINCT_COUNTS, COLS_128],
                          capacity=64, salt=30))
    rows = rows_of(["W0", "W1", "W2", "W3", "A", "B"])
    out.append(class_case("wrap", "C-wrap", rows, counts_for(rows, 3),
                          [WRAP_WG, WRAP_GLOBAL, WORD1_BRANCH, ONE_TILE, ONE_GROUP, DISTINCT_COUNTS], capacity=16,
                          salt=31))
    # 64 and 65 columns: r1 is 0, or 0 and 1; P and Q differ in column 63 alone and share their home in the
    # workgroup's table, three more rows share P's home in the global table of 16 slots
    for n_cols, r1 in ((64, 0), (65, 1)):
        both, h_both, r0, h = search_r0(r1, CLS_SLOTS, seed=64 + r1)
        order = np.lexsort((both, popcount(both)))
        p = int(both[order[0]])
        hp = int(h_both[order[0]])
        more = r0[((h & 15) == (hp & 15)) & (r0 != U(p))]
        more = more[np.lexsort((more, popcount(more)))][:3]
        rows = [(p, r1), (p | B63, r1)] + [(int(v), r1) for v in more] + ([(p, 0)] if r1 else [])
        rows = np.array(rows, dtype=U)
        out.append(class_case("cols_%d" % n_cols, "C-small", rows, counts_for(rows),
                              [WORD2_R0, SHARE3_GLOBAL, ONE_TILE, ONE_GROUP, DISTINCT_COUNTS, EXACT_CAPACITY,
                               COLS_64 if n_cols == 64 else COLS_65],
                              n_cols=n_cols, salt=40 + r1))
    # the spill: 300 fillers of one or two columns and one k-mer each over the buckets 0 .. 13, the designed rows
    # with 3 .. 12 k-mers, alternately in bucket 0 and in bucket 15
    designed = rows_of(["A", "B", "C", "D", "E", "W0", "W1", "W2", "W3"])
    fill = [(1 << a, 0) if a < 64 else (0, 1 << (a - 64)) for a in range(128)]
    fill += [((1 << a) | (1 << (a + 1)), 0) for a in range(0, 62)]
    fill += [(0, (1 << a) | (1 << (a + 2))) for a in range(0, 61)]
    fill += [(1 << a, 1 << a) for a in range(49)]
    rows = np.concatenate([designed, np.array(fill, dtype=U)])
    counts = np.concatenate([counts_for(designed, 3), np.ones(len(fill), dtype=np.int64)])
    n_designed = designed.shape[0]
    out.append(class_case("spill", "C-spill", rows, counts,
                          [SPILL, SPILL_MERGE, SHARED_WG, WORD1_BRANCH, WORD2_R0, WORD2_R1, WRAP_WG, ONE_GROUP,
                           EXACT_CAPACITY],
                          buckets=lambda r, i: (0 if i % 2 == 0 else 15) if r < n_designed else (r % 14), salt=50))
    return out


COUNT_CASES = _count_cases()
# capacities below the class count: (case id, capacity)
REFUSALS = [("small_%d" % n, n - 1) for n in (2, 3, 4, 5, 8, 9)] + [("small_3", 1)]


# ---- the look-up families -------------------------------------------------------------------------------------------
def lookup_case(cid, family, data, table, covers, salt):
    """data: [(row name, k-mers)], the rows the structure holds; table: the names of the caller's rows."""
    names = [name for name, _ in data]
    rows = rows_of(names) if all(isinstance(nm, str) for nm in names) else np.array(names, dtype=U)
    case = class_case(cid, family, rows, [c for _, c in data], covers, salt=salt)
    trows = rows_of(table) if all(isinstance(nm, str) for nm in table) else np.array(table, dtype=U)
    case["table"] = sort_rows(trows)
    case["in_data"] = np.array([any((r == t).all() for r in rows) for t in case["table"]])
    return case


def _lookup_cases():
    out = []
    # L-shared on the pool's rows, and on the first quadruples of the 8-slot and the 16-slot search
    out.append(lookup_case("shared_pool_4", "L-shared", [("A", 5), ("B", 6), ("C", 3), ("D", 4), ("E", 7)],
                           ["A", "B", "C", "D"], [SHARED_CALLER, ABSENT_SHARED, WORD1_BRANCH, WORD2_R0, WORD2_R1], 60))
    for slots, extra in ((8, []), (16, ["W0"])):
        x, y1, y2, y3 = (int(v[0]) for v in search_quadruples(slots))
        four = [(x, y1), (x, y2), (x | B63, y1), (x, y1 | B63)]
        data = list(zip(four + [(x, y3)] + [ROW[e] for e in extra], [5, 6, 3, 4, 7, 2]))
        out.append(lookup_case("shared_%d" % slots, "L-shared", data, four + [ROW[e] for e in extra],
                               [SHARED_CALLER, ABSENT_SHARED, WORD1_BRANCH, WORD2_R0, WORD2_R1], 61 + slots))
    out.append(lookup_case("wrap", "L-wrap", [("W0", 4), ("W1", 5), ("W2", 6), ("W3", 3), ("A", 7), ("B", 2)],
                           ["W0", "W1", "W2", "A", "B"], [WRAP_CALLER, ABSENT_LAST, WORD1_BRANCH], 80))
    order = ["A", "B", "D", "C", "W0", "W1", "W2", "O0", "O1"] + ["O%d" % i for i in range(2, 10)]
    for n in (1, 2, 3, 4, 5, 8, 9, 16, 17):
        table = order[:n]
        held = [name for name in table if name not in ("O1", "O3", "O5", "O7")]  # those are table-only rows
        data = [(name, 3 + i) for i, name in enumerate(held)] + [("E", 2), ("W3", 1)]
        covers = [ABSENT_SHARED, ABSENT_LAST] + ([SHARE3_CALLER] if n >= 3 else []) + \
                 ([TABLE_ONLY_ROWS] if n >= 9 else []) + ([WRAP_CALLER] if n >= 8 else [])
        out.append(lookup_case("sizes_%d" % n, "L-sizes", data, table, covers, 90 + n))
    return out


LOOKUP_CASES = _lookup_cases()


# ---- the paint case --------------------------------------------------------------------------------------------------
K_PAINT, N_PAINT = 15, 10
PAINT_TABLE = ["A", "B", "C", "D", "W0", "W1", "W2"]   # 16 slots: A .. D on one home, W on the last
PAINT_ABSENT = ["E", "F", "W3"]                        # E, F on the home of A .. D, W3 on the last slot
PAINT_PASSES = (1, 7, 0)


def paint_case():
    """The genome-cut construction of test_gpu_paint.py's `edges`: a genome of distinct canonical k-mers cut into
    consecutive sequences that overlap by K - 1 bases; position p's k-mer has the row names[pattern[p]].  Stretches:
    A C A C ... (a change at every position between rows that only key word 2 tells apart), A D, A B, C D, E F E F
    (absent rows of that home: one run), W0 W1 W2, W3 W0, and plain runs of one row."""
    k, total = K_PAINT, 600
    names = PAINT_TABLE + PAINT_ABSENT
    at = {name: i for i, name in enumerate(names)}
    pattern = []
    for pair, length in ((("A", "C"), 40), (("A",), 9), (("A", "D"), 40), (("E", "F"), 30), (("A", "B"), 41),
                         (("C", "D"), 40), (("D",), 70), (("W0", "W1", "W2"), 60), (("W3", "W0"), 40),
                         (("E", "A"), 30), (("F", "W3"), 20), (("B", "W1"), 64), (("C",), 16)):
        pattern += [at[pair[i % len(pair)]] for i in range(length)]
    pattern = np.array(pattern + [at["A"]] * (total - len(pattern)))
    assert pattern.size == total
    for seed in range(4300, 4400):
        genome = synth.random_genome(total + k - 1, seed)
        x = synth.canonical(synth.kmers_of_bases(genome, k), k)
        if np.unique(x).size == total:
            break
    cuts = [0, 20, 21, 22, 64, 130, 131, 256, 300, 447, total]
    text = synth.string_of_bases(genome)
    strings = [text[a:b + k - 1] for a, b in zip(cuts[:-1], cuts[1:])]
    rows = rows_of(names)
    node_sets = node_sets_of(x, pattern, rows, 128)
    return {"id": "paint", "k": k, "n": N_PAINT, "names": names, "rows": rows, "pattern": pattern, "kmers": x,
            "strings": strings, "cuts": cuts, "node_sets": node_sets, "table": sort_rows(rows_of(PAINT_TABLE)),
            "covers": (ALTERNATE_CHANGE, ALTERNATE_SAME, SHARED_CALLER, WRAP_CALLER, ABSENT_SHARED, ABSENT_LAST)}


PAINT = paint_case()


# ---- the end table ---------------------------------------------------------------------------------------------------
_DIGITS = str.maketrans("ACGT", "0123")


def kmer_int(s):
    return int(s.translate(_DIGITS), 4)


def end_entries(strings, k, canonical):
    """[(key, string, kind, flipped)] of the end table: kind 'first', 'last' or 'single'; the key is the k-mer, in
    canonical mode its canonical form, flipped saying that this is the reverse complement of the k-mer as written."""
    out = []
    for s, t in enumerate(strings):
        ends = [(t[:k], "single")] if len(t) == k else [(t[:k], "first"), (t[-k:], "last")]
        for e, kind in ends:
            r = lref.rc(e)
            flipped = canonical and r < e
            out.append((kmer_int(r if flipped else e), s, kind, flipped))
    return out


def link_model(strings, k, canonical):
    """What the model says of a container: slots, the entries with their homes, the occupied set, the keys that
    links lead to, and the keys of the extensions that are looked up and are no end."""
    slots = link_slots(len(strings))
    entries = end_entries(strings, k, canonical)
    keys = np.array([e[0] for e in entries], dtype=U)
    homes = link_homes(keys, slots)
    occ = occupied(homes, slots)
    off, to = lref.links(strings, k, canonical)
    key_of = lambda y: kmer_int(lref.canon(y) if canonical else y)  # noqa: E731
    targets = {key_of(lref.oriented(strings, int(w))[:k]) for w in to}
    have = {int(v) for v in keys}
    absent = set()
    for v in range(2 * len(strings)):
        if canonical or not v & 1:
            last = lref.oriented(strings, v)[-k:]
            for b in "ACGT":
                y = last[1:] + b
                if key_of(y) != key_of(last) and key_of(y) not in have:
                    absent.add(key_of(y))
    return {"slots": slots, "entries": entries, "homes": homes, "occ": occ, "targets": targets, "absent": absent,
            "n_links": int(to.size)}


def target_groups(model):
    """{home: [entries that are link targets]} for the homes with at least 3 of them."""
    by = {}
    for e, h in zip(model["entries"], model["homes"]):
        if e[0] in model["targets"]:
            by.setdefault(int(h), []).append(e)
    return {h: g for h, g in by.items() if len(g) >= 3}


def has_group(model, mixed):
    for g in target_groups(model).values():
        if not mixed or ({e[2] for e in g} == {"first", "last", "single"} and len({e[3] for e in g}) == 2):
            return True
    return False


def has_wrap(model):
    """The run that holds the last slot passes it, and a link target has its home in that run."""
    occ, slots = model["occ"], model["slots"]
    start, length = run_of(occ, slots - 1)
    if length == 0 or start + length <= slots or length == slots:
        return False
    inside = lambda h: (h - start) % slots < length  # noqa: E731
    return any(inside(int(h)) for e, h in zip(model["entries"], model["homes"]) if e[0] in model["targets"])


def has_absent(model):
    slots = model["slots"]
    homes = link_homes(np.array(sorted(model["absent"]), dtype=U), slots) if model["absent"] else []
    return any(run_of(model["occ"], int(h))[1] >= 3 for h in homes)


def link_search(build, k, modes, design_mode, predicate, seed, tries=4000):
    """build(seed) for the first seed from `seed` on whose container is legal in every mode and has the property in
    the designed mode."""
    for s in range(seed, seed + tries):
        strings = build(s)
        if all(lc.legal(strings, k, m) for m in modes) and predicate(link_model(strings, k, design_mode)):
            return strings
    raise AssertionError("no container from seed %d" % seed)


def link_case(cid, family, k, strings, modes, design_mode, covers):
    return {"id": "%s-k%d-%s" % (cid, k, "canonical" if design_mode else "directed"), "family": family, "k": k,
            "strings": list(strings), "modes": tuple(modes), "design_mode": design_mode, "covers": tuple(covers)}


def _pieces(n, seed, longest=3):
    rng = np.random.default_rng(seed)
    return [int(v) for v in rng.integers(1, longest + 1, size=n)], [int(v) for v in rng.integers(0, 2, size=n)]


def _link_cases():
    out = []
    both = (True, False)
    for k in (5, 16, 31):
        n = 10 if k == 5 else 40
        for mode in both:
            sizes, flips = _pieces(n, 7 * k + mode, longest=2 if k == 5 else 3)
            if not mode:
                flips = [0] * n  # (as written: every piece links to the next)
            build = lambda s, sizes=sizes, flips=flips: lc.chain(k, sizes, flips, s)  # noqa: E731
            mixed = mode and k > 5
            strings = link_search(build, k, both, mode, lambda m, mixed=mixed: has_group(m, mixed), 2000 + 10 * k)
            out.append(link_case("group", "E-group", k, strings, both, mode,
                                 [E_GROUP, HAS_LINKS] + ([E_MIXED] if mixed else [])))
        for mode in both:
            n = 3 if mode else 4
            sizes, flips = _pieces(n, 11 * k + mode, longest=2)
            if not mode:
                flips = [0] * n
            build = lambda s, sizes=sizes, flips=flips: lc.chain(k, sizes, flips, s)  # noqa: E731
            strings = link_search(build, k, both, mode, has_wrap, 3000 + 10 * k)
            out.append(link_case("wrap", "E-wrap", k, strings, both, mode, [E_WRAP, E_SMALL, HAS_LINKS]))
        n = 8 if k == 5 else 12
        sizes, flips = _pieces(n, 13 * k, longest=2)
        build = lambda s, sizes=sizes, flips=flips: lc.chain(k, sizes, flips, s, gaps=(n // 2,))  # noqa: E731
        for mode in both:
            strings = link_search(build, k, both, mode, has_absent, 4000 + 10 * k)
            out.append(link_case("absent", "E-absent", k, strings, both, mode, [E_ABSENT, HAS_LINKS]))
    k, n = 23, 300
    sizes, flips = _pieces(n, 23)
    build = lambda s: lc.chain(k, sizes, flips, s, gaps=tuple(range(50, n, 50)))  # noqa: E731
    many = lambda m: wrapped(m["homes"], m["slots"]) >= 1 and len(shared_homes(m["homes"])) >= 10  # noqa: E731
    out.append(link_case("many", "E-many", k, link_search(build, k, both, True, many, 5000), both, True,
                         [E_MANY, HAS_LINKS]))
    return out


LINK_CASES = _link_cases()


# ---- the tile table --------------------------------------------------------------------------------------------------
TILE_CELLS = [(8, 1, 2), (15, 4, 4), (31, 1, 8)]  # (k, N, key bytes): 15, 26 and 61 key bits
TILE_NODES = 7
TILE_GROUP = 16


def tile_case(cell, cut):
    """Seven nodes without edges and one bucket.  16 keys whose home is the last slot and 16 whose home is slot 0 (the
    smallest such keys of the key space at 15 bits, of 2^20 seeded draws otherwise), key i of a group held by 1 + i % 7
    nodes from node i % 7 on; 24 keys of other homes in one node each; with `cut`, 700 more keys in one node each."""
    k, n, kb = cell
    key_bits = 2 * k - n
    if key_bits <= 16:
        space = np.arange(1 << key_bits, dtype=U)
    else:
        space = np.unique(np.random.default_rng(100 + k).integers(0, 1 << key_bits, size=1 << 20, dtype=U))
    homes = tile_homes(space)
    last, first = space[homes == TILE_SLOTS - 1][:TILE_GROUP], space[homes == 0][:TILE_GROUP]
    rest = space[(homes > 40) & (homes < TILE_SLOTS - 40)]
    rest = rest[:: max(1, rest.size // (24 + (700 if cut else 0) + 1))][:24 + (700 if cut else 0)]
    bucket = U((1 << n) - 1 if kb == 2 else BUCKET if kb == 4 else 0) << U(key_bits)
    holders = {}
    for group in (last, first):
        for i, key in enumerate(group):
            holders[int(key)] = [(i + j) % TILE_NODES for j in range(1 + i % TILE_NODES)]
    for i, key in enumerate(rest):
        holders[int(key)] = [(3 * i) % TILE_NODES]
    node_sets = [np.sort(np.array([key for key, h in holders.items() if j in h], dtype=U) | bucket)
                 for j in range(TILE_NODES)]
    return {"id": "tile-k%d-N%d-u%d-%s" % (k, n, 8 * kb, "cut" if cut else "one"), "k": k, "n": n, "kb": kb,
            "cut": cut, "keys": np.array(sorted(holders), dtype=U), "holders": holders, "node_sets": node_sets,
            "covers": (T_LAST, T_FIRST, T_MULTI, T_CUT if cut else T_ONE_TILE)}


TILE_CASES = [tile_case(cell, cut) for cell in TILE_CELLS for cut in (False, True)]
