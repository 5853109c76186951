"""The designed inputs of tests/hash_table_cases.py are what they claim, judged by predicate on the model; every
family has every property it lists; the anchors stand in the kernels' text; the searchers find what the arithmetic
says they should, in seconds; and no expected value of test_gpu_hash_tables.py is vacuous.  No GPU."""
import time

import numpy as np
import pytest

import hash_table_cases as ht
import paint_reference as pr
import spss_links_cases as lc
import spss_links_reference as lref
from index_reference import IndexReference

U = np.uint64
B63 = ht.B63


# ---- the anchors and the model ---------------------------------------------------------------------------------------
def test_anchors_stand_in_the_kernels_text():
    for what, found, wanted in ht.anchor_counts():
        assert found == wanted, what
    c = ht.constants()
    assert (c.cls_slots, c.tile, c.rows_per_group, c.threads) == (1024, 512, 8192, 256)
    assert (c.global_floor, c.global_factor, c.caller_floor, c.caller_factor, c.link_floor, c.link_factor) == \
        (2, 2, 2, 2, 1, 4)


@pytest.mark.parametrize("file,old,new", [
    ("rowtile", "x ^= x >> 32;", "x ^= x >> 31;"),
    ("rowtile", "0x94D049BB133111EBull", "0x94D049BB133111E9ull"),
    ("clstable", "pc::pc_mix(r1 + 0x9E3779B97F4A7C15ull)", "pc::pc_mix(r1 ^ 0x9E3779B97F4A7C15ull)"),
    ("clstable", "const unsigned long long w2 = (r0 >> 63) | ((r1 >> 63) << 1) | kValid;",
     "const unsigned long long w2 = (r0 >> 63) | ((r1 >> 62) << 1) | kValid;"),
    ("classes", "constexpr int kClsSlots = 1024;", "constexpr int kClsSlots = 2048;"),
    ("classes", "kClsSlots * 3 / 4 - kTile;", "kClsSlots / 2 - kTile;"),
    ("rowtile", "constexpr int kSlots = 2 * kTile;", "constexpr int kSlots = 4 * kTile;"),
    ("classes", "while (slots < 2 * capacity)", "while (slots < 4 * capacity)"),
    ("classids", "while (slots < 2 * n_classes)", "while (slots <= 2 * n_classes)"),
    ("links", "while (slots < 4 * uint64_t(n))", "while (slots < 2 * uint64_t(n))"),
    ("links", "return pc::pc_mix(key) & mask;", "return pc::pc_mix(key >> 1) & mask;"),
    ("rowtile", "uint32_t(pc_mix(key)) & (kSlots - 1);", "uint32_t(pc_mix(key) >> 32) & (kSlots - 1);")])
def test_a_changed_kernel_text_is_noticed(file, old, new):
    """A changed hash, constant or table size does not move the cases off their collisions silently: either an anchor
    is gone, or the constants read differ from those the cases were built with."""
    src = ht.sources()
    assert old in src[file]
    src[file] = src[file].replace(old, new)
    try:
        changed = ht.constants(src)
    except AssertionError:
        return
    assert changed != ht.C


def test_pc_mix_against_big_integers():
    x = np.concatenate([np.random.default_rng(3).integers(0, 1 << 63, size=4000, dtype=U) << U(1),
                        np.array([0, 1, ht.M64, B63, 0xFFFFFFFF, 1 << 32], dtype=U)])
    got = ht.pc_mix(x)
    assert [int(v) for v in got] == [ht.pc_mix_int(int(v)) for v in x]
    assert np.unique(got).size == x.size  # (a bijection)
    r0, r1 = x[:2000], x[2000:4000]
    want = [ht.pc_mix_int(int(a) ^ ht.pc_mix_int(int(b) + ht.C.gold)) & 0xFFFFFFFF for a, b in zip(r0, r1)]
    assert [int(v) for v in ht.cls_hash(r0, r1)] == want
    assert ht.key_words(ht.M64, 0) == (ht.M64, B63, B63 | 1) and ht.key_words(0, B63) == (B63, B63, B63 | 2)


def test_table_sizes():
    assert [ht.global_slots(c) for c in (1, 2, 3, 4, 5, 8, 9, 16, 17)] == [2, 4, 8, 8, 16, 16, 32, 32, 64]
    assert [ht.caller_slots(c) for c in (1, 2, 3, 4, 5, 8, 9, 16, 17)] == [2, 4, 8, 8, 16, 16, 32, 32, 64]
    assert [ht.link_slots(n) for n in (1, 2, 3, 4, 5, 300)] == [4, 8, 16, 16, 32, 2048]


def test_occupied_set_does_not_depend_on_the_order():
    rng = np.random.default_rng(9)
    for slots, n in ((8, 4), (16, 8), (64, 30), (1024, 500)):
        homes = rng.integers(0, slots, size=n)
        homes[: n // 3] = slots - 1 - rng.integers(0, 2, size=n // 3)  # a crowd at the end: wraps
        want = ht.occupied(homes, slots)
        for _ in range(5):
            assert np.array_equal(ht.occupied(rng.permutation(homes), slots), want)
        assert ht.wrapped(homes, slots) >= n // 3 - 2 and want.sum() == n


def test_searchers_find_what_the_arithmetic_says_in_seconds():
    """2^22 drawn y: about 2^22 / 1024 rows share their home in the 1024-slot table with the row that differs in bit
    63 of r0 alone, as many for bit 63 of r1, as many share slot 1023 with the fixed x; 2^20 drawn quadruples: about
    2^20 / 8^4 put the five rows of L-shared on one home of an 8-slot table (and 2^20 / 16^4 of a 16-slot one)."""
    ht._quads.clear()
    t0 = time.perf_counter()
    pool = ht.search_pool()
    quads = ht.search_quadruples(8)
    quads16 = ht.search_quadruples(16)
    spent = time.perf_counter() - t0
    print("pool seed %d: %d candidates, %d / %d pairs on one home (bit 63 of r0 / of r1), %d rows on slot 1023; "
          "%d quadruples at 8 slots, %d at 16; %.2f s"
          % (pool.seed, pool.y.size, pool.both_r0.sum(), pool.both_r1.sum(),
             ((pool.h & 1023) == 1023).sum(), quads[0].size, quads16[0].size, spent))
    assert pool.seed == ht.POOL.seed and pool.y1 == ht.POOL.y1  # seeded and repeatable
    assert (1 << 22) - 2048 <= pool.y.size <= 1 << 22  # (less the draws without a column)
    for found in (pool.both_r0.sum(), pool.both_r1.sum(), ((pool.h & 1023) == 1023).sum()):
        assert 3700 <= found <= 4500, found
    assert 200 <= quads[0].size <= 320 and 4 <= quads16[0].size <= 40
    assert spent < 3.0
    x, y1, y2, y3 = (int(v[0]) for v in quads)
    rows = np.array([(x, y1), (x, y2), (x | B63, y1), (x, y1 | B63), (x, y3)], dtype=U)
    assert np.unique(ht.row_homes(rows, 8)).size == 1 and np.unique(rows, axis=0).shape[0] == 5


def test_designed_rows():
    """A .. F on one home of the 1024-slot table, W on its last slot; all with the same key word 0."""
    homes = ht.row_homes(ht.rows_of(["A", "B", "C", "D", "E", "F"]), ht.CLS_SLOTS)
    assert (homes == ht.HOME).all() and ht.HOME not in (0, ht.CLS_SLOTS - 1)
    assert (ht.row_homes(ht.rows_of(["W%d" % i for i in range(6)]), ht.CLS_SLOTS) == ht.CLS_SLOTS - 1).all()
    assert len({ht.key_words(*r)[0] for r in ht.ROW.values()}) == 1
    assert len(set(ht.ROW.values())) == len(ht.ROW)
    a, c, d = (ht.key_words(*ht.ROW[n]) for n in "ACD")
    assert a[:2] == c[:2] == d[:2] and len({a[2], c[2], d[2]}) == 3


# ---- the class families ----------------------------------------------------------------------------------------------
def same_home_pairs(rows, slots):
    homes = ht.row_homes(rows, slots)
    return [(i, j) for i in range(len(rows)) for j in range(i + 1, len(rows)) if homes[i] == homes[j]]


def pair_kinds(rows, slots):
    """Which partial-key meetings the rows guarantee in a table of `slots` slots."""
    kinds = set()
    for i, j in same_home_pairs(rows, slots):
        a, b = (int(v) for v in rows[i]), (int(v) for v in rows[j])
        (a0, a1), (b0, b1) = a, b
        wa, wb = ht.key_words(a0, a1), ht.key_words(b0, b1)
        if wa[0] == wb[0] and wa[1] != wb[1]:
            kinds.add(ht.WORD1_BRANCH)
        if a0 ^ b0 == B63 and a1 == b1:
            kinds.add(ht.WORD2_R0)
        if a1 ^ b1 == B63 and a0 == b0:
            kinds.add(ht.WORD2_R1)
    return kinds


def has_shared_four(rows, slots):
    have = {(int(r[0]), int(r[1])): int(h) for r, h in zip(rows, ht.row_homes(rows, slots))}
    for (x, y1), h in have.items():
        if x & B63 or y1 & B63:
            continue
        if have.get((x | B63, y1)) == h and have.get((x, y1 | B63)) == h and \
                any(hx == h and rx == x and ry not in (y1, y1 | B63) for (rx, ry), hx in have.items()):
            return True
    return False


def reference_of(case, perm=None):
    node_sets, kmers, row_of = ht.case_structure(case, perm)
    return IndexReference(case["k"], node_sets, [[] for _ in node_sets]), node_sets, kmers, row_of


SMALL_SLOTS = {1: 2, 2: 4, 3: 8, 4: 8, 5: 16, 8: 16, 9: 32}


@pytest.mark.parametrize("case", ht.COUNT_CASES, ids=[c["id"] for c in ht.COUNT_CASES])
def test_count_case_is_what_it_claims(case):
    rows, counts, covers = case["rows"], case["counts"], case["covers"]
    ref, node_sets, kmers, row_of = reference_of(case)
    entries = ht.entries_per_bucket(node_sets, case["k"], case["n"])
    g_slots = ht.global_slots(case["capacity"])
    g_homes = ht.row_homes(rows, g_slots)
    wg_homes = ht.row_homes(rows, ht.CLS_SLOTS)
    # the fabricated structure has exactly the designed rows with the designed counts
    want_rows, want_counts = ref.color_classes()
    order = np.lexsort((rows[:, 0], rows[:, 1]))
    assert np.array_equal(want_rows, rows[order]) and np.array_equal(want_counts, counts[order])
    assert len(node_sets) == case["n_cols"] and rows.any(axis=1).all()
    kinds = pair_kinds(rows, ht.CLS_SLOTS)
    for cover in covers:
        if cover in (ht.WORD1_BRANCH, ht.WORD2_R0, ht.WORD2_R1):
            assert cover in kinds, cover
            if g_slots <= ht.CLS_SLOTS:  # one home in the workgroup's table is one home in a smaller table
                assert cover in pair_kinds(rows, g_slots)
        elif cover == ht.SHARED_WG:
            assert has_shared_four(rows, ht.CLS_SLOTS)
        elif cover == ht.ONE_TILE:
            assert (entries > 0).sum() == 1 and entries.max() <= ht.TILE
        elif cover == ht.ONE_GROUP:
            assert entries.sum() <= ht.C.rows_per_group
        elif cover == ht.WRAP_WG:
            assert (wg_homes == ht.CLS_SLOTS - 1).sum() >= 4 and ht.wrapped(wg_homes, ht.CLS_SLOTS) >= 3
        elif cover == ht.WRAP_GLOBAL:
            assert (g_homes == g_slots - 1).sum() >= 3 and ht.wrapped(g_homes, g_slots) >= 2
        elif cover == ht.SHARE3_GLOBAL:
            assert max(ht.shared_homes(g_homes).values()) >= 3
        elif cover == ht.EXACT_CAPACITY:
            assert case["capacity"] == rows.shape[0]
            if case["id"].startswith("small_"):
                assert g_slots == SMALL_SLOTS[rows.shape[0]]
        elif cover in (ht.SPILL, ht.SPILL_MERGE):
            assert ht.ONE_GROUP in covers
            bucket = (kmers >> U(2 * case["k"] - case["n"])).astype(np.int64)
            last = bucket.max()
            before = set(row_of[bucket < last].tolist())
            if cover == ht.SPILL:  # tile_done sees more than kClsSpill slots taken, and another tile follows
                assert len(before) > ht.CLS_SPILL and entries[last] > 0
                assert len(before) <= ht.CLS_SLOTS * 3 // 4  # (and a table that never spills would still hold them)
            else:
                assert before & set(row_of[bucket == last].tolist()) & set(range(9))
        elif cover == ht.COLS_128:
            assert case["n_cols"] == 128 and (rows.shape[0] < 3 or (rows[:, 1] >> U(63)).any())
        elif cover == ht.COLS_64:
            assert case["n_cols"] == 64 and (rows[:, 0] >> U(63)).any() and not rows[:, 1].any()
        elif cover == ht.COLS_65:
            assert case["n_cols"] == 65 and (rows[:, 1] == 1).any() and (rows[:, 0] >> U(63)).any()
        elif cover == ht.DISTINCT_COUNTS:
            assert np.unique(want_counts).size == want_counts.size
        else:
            raise AssertionError("no predicate for: " + cover)
    if ht.DISTINCT_COUNTS not in covers:  # the spill: the designed rows' counts are their own, the fillers' are 1
        assert case["family"] == "C-spill" and np.unique(counts[:9]).size == 9 and counts[:9].min() > counts[9:].max()


def test_refusals_name_real_cases():
    by_id = {c["id"]: c for c in ht.COUNT_CASES}
    for cid, capacity in ht.REFUSALS:
        assert 1 <= capacity < by_id[cid]["rows"].shape[0]
    assert ("small_3", 1) in ht.REFUSALS and {by_id[c]["rows"].shape[0] - cap for c, cap in ht.REFUSALS} == {1, 2}


def expected_ids(case, perm=None):
    ref = reference_of(case, perm)[0]
    return ref, ref.class_ids(case["table"], cols=perm)


@pytest.mark.parametrize("case", ht.LOOKUP_CASES, ids=[c["id"] for c in ht.LOOKUP_CASES])
def test_lookup_case_is_what_it_claims(case):
    rows, table, covers = case["rows"], case["table"], case["covers"]
    n = table.shape[0]
    slots = ht.caller_slots(n)
    t_homes = ht.row_homes(table, slots)
    in_table = np.array([any((r == t).all() for t in table) for r in rows])
    absent_homes = ht.row_homes(rows[~in_table], slots)
    assert np.array_equal(table, ht.sort_rows(table)) and np.unique(table, axis=0).shape[0] == n
    kinds = pair_kinds(table, slots)
    for cover in covers:
        if cover in (ht.WORD1_BRANCH, ht.WORD2_R0, ht.WORD2_R1):
            assert cover in kinds, cover
        elif cover == ht.SHARED_CALLER:
            assert has_shared_four(table, slots) and n in (4, 5) and slots in (8, 16)
        elif cover == ht.ABSENT_SHARED:  # the look-up of an absent row starts on an occupied slot
            assert any(h in t_homes and h != slots - 1 for h in absent_homes)
            if n >= 3:
                crowd = {h for h, c in ht.shared_homes(t_homes).items() if c >= 3}
                assert crowd & set(absent_homes.tolist())
        elif cover == ht.WRAP_CALLER:
            assert (t_homes == slots - 1).sum() >= 3 and ht.wrapped(t_homes, slots) >= 2
        elif cover == ht.ABSENT_LAST:
            assert (absent_homes == slots - 1).any()
        elif cover == ht.SHARE3_CALLER:
            assert max(ht.shared_homes(t_homes).values()) >= 3
        elif cover == ht.TABLE_ONLY_ROWS:
            assert not case["in_data"].all() and case["in_data"].sum() >= 3
        else:
            raise AssertionError("no predicate for: " + cover)
    # no expected value is vacuous, with the identity column list and with the permuted one
    for perm in (None, ht.permutation(128)):
        ref, (kmers, ids) = expected_ids(case, perm)
        assert kmers.size == case["counts"].sum() == ref.n_distinct
        assert np.array_equal(ref.color_classes(perm)[0], ht.sort_rows(rows))  # the permuted list gives the rows back
        values, share = np.unique(ids, return_counts=True)
        assert values.size >= min(3, n + 1), values  # (a table of one row has two values to give: its id and none)
        assert 2 * share[values >= 0].max() <= ids.size
        assert 0 < (ids < 0).sum() < ids.size
        if perm is not None:  # ... and the identity list on the permuted structure would give other rows
            assert not np.array_equal(ref.color_classes()[0], ht.sort_rows(rows))


def test_paint_case_is_what_it_claims():
    p = ht.PAINT
    table, names, pattern, cuts = p["table"], p["names"], p["pattern"], p["cuts"]
    slots = ht.caller_slots(table.shape[0])
    assert slots == 16 and has_shared_four(table, slots)
    home = {name: int(ht.row_homes(ht.rows_of([name]), slots)[0]) for name in names}
    assert len({home[n] for n in "ABCDEF"}) == 1 and {home[n] for n in ("W0", "W1", "W2", "W3")} == {slots - 1}
    assert (ht.row_homes(table, slots) == slots - 1).sum() >= 3
    in_table = [name in ht.PAINT_TABLE for name in names]
    inner = np.setdiff1d(np.arange(1, pattern.size), cuts)  # a position and the one before it in one sequence
    a, b = pattern[inner - 1], pattern[inner]
    differ = (a != b) & np.array([home[names[i]] == home[names[j]] for i, j in zip(a, b)])
    both_in = np.array([in_table[i] and in_table[j] for i, j in zip(a, b)])
    both_out = np.array([not in_table[i] and not in_table[j] for i, j in zip(a, b)])
    assert (differ & both_in).sum() >= 100 and (differ & both_out).sum() >= 20
    met = {frozenset((names[i], names[j])) for i, j in zip(a[differ], b[differ])}
    assert {frozenset("AC"), frozenset("AD"), frozenset("AB"), frozenset("EF"), frozenset(("W0", "W1"))} <= met
    # the reference: the classes are the pattern's, the absent rows read none, E F E F is one run
    ref = IndexReference(p["k"], p["node_sets"], [[] for _ in p["node_sets"]])
    ids = np.concatenate(pr.position_ids(ref, p["strings"], None, table, True))
    at = {(int(r[0]), int(r[1])): c for c, r in enumerate(table)}
    assert np.array_equal(ids, [at.get(ht.ROW[names[v]], pr.NONE) for v in pattern])
    off, start, cls, missing = pr.class_runs(ref, p["strings"], None, table, True)
    assert 0 < missing < ids.size and np.unique(ids).size >= 3 and off[-1] > 300
    assert 2 * np.unique(ids, return_counts=True)[1].max() <= ids.size
    first_ef = int(np.flatnonzero((pattern[:-1] == names.index("E")) & (pattern[1:] == names.index("F")))[0])
    assert (ids[first_ef:first_ef + 30] == pr.NONE).all() and first_ef not in cuts


CLASS_FAMILIES = {
    "C-shared": {ht.SHARED_WG, ht.WORD1_BRANCH, ht.WORD2_R0, ht.WORD2_R1, ht.ONE_TILE, ht.ONE_GROUP, ht.COLS_128},
    "C-wrap": {ht.WRAP_WG, ht.WRAP_GLOBAL},
    "C-small": {ht.EXACT_CAPACITY, ht.SHARE3_GLOBAL, ht.COLS_64, ht.COLS_65, ht.COLS_128, ht.DISTINCT_COUNTS},
    "C-spill": {ht.SPILL, ht.SPILL_MERGE, ht.SHARED_WG},
    "L-shared": {ht.SHARED_CALLER, ht.ABSENT_SHARED, ht.WORD1_BRANCH, ht.WORD2_R0, ht.WORD2_R1},
    "L-wrap": {ht.WRAP_CALLER, ht.ABSENT_LAST},
    "L-sizes": {ht.SHARE3_CALLER, ht.TABLE_ONLY_ROWS, ht.ABSENT_SHARED},
    "E-group": {ht.E_GROUP, ht.E_MIXED, ht.HAS_LINKS},
    "E-wrap": {ht.E_WRAP, ht.E_SMALL},
    "E-absent": {ht.E_ABSENT},
    "E-many": {ht.E_MANY},
}


def test_every_family_has_every_property_it_lists():
    seen = {}
    for case in ht.COUNT_CASES + ht.LOOKUP_CASES + ht.LINK_CASES:
        seen.setdefault(case["family"], set()).update(case["covers"])
    for family, wanted in CLASS_FAMILIES.items():
        assert wanted <= seen.get(family, set()), (family, wanted - seen.get(family, set()))
    small = sorted(c["rows"].shape[0] for c in ht.COUNT_CASES if c["id"].startswith("small_"))
    assert small == [1, 2, 3, 4, 5, 8, 9]
    sizes = sorted(c["table"].shape[0] for c in ht.LOOKUP_CASES if c["family"] == "L-sizes")
    assert sizes == [1, 2, 3, 4, 5, 8, 9, 16, 17]
    assert {c["table"].shape[0] for c in ht.LOOKUP_CASES if c["family"] == "L-shared"} == {4, 5}
    for family in ("E-group", "E-wrap", "E-absent"):
        ks = {(c["k"], c["design_mode"]) for c in ht.LINK_CASES if c["family"] == family}
        assert ks == {(k, m) for k in (5, 16, 31) for m in (True, False)}, family
    assert set(ht.PAINT["covers"]) >= {ht.ALTERNATE_CHANGE, ht.ALTERNATE_SAME} and ht.PAINT_PASSES == (1, 7, 0)
    assert {(c["kb"], c["cut"]) for c in ht.TILE_CASES} == {(kb, cut) for kb in (2, 4, 8) for cut in (False, True)}


# ---- the end table ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ht.LINK_CASES, ids=[c["id"] for c in ht.LINK_CASES])
def test_link_case_is_what_it_claims(case):
    k, strings, mode = case["k"], case["strings"], case["design_mode"]
    for m in case["modes"]:
        lref.check_container(strings, k, m)
        assert lc.legal(strings, k, m)
    model = ht.link_model(strings, k, mode)
    n = len(strings)
    assert model["slots"] == ht.link_slots(n) >= 4 * n and model["occ"].sum() == len(model["entries"])
    assert len({e[0] for e in model["entries"]}) == len(model["entries"])  # every end has a key of its own
    for cover in case["covers"]:
        if cover == ht.E_GROUP:
            groups = ht.target_groups(model)
            assert groups and max(len(g) for g in groups.values()) >= 3
        elif cover == ht.E_MIXED:
            assert mode and ht.has_group(model, True)
        elif cover == ht.E_WRAP:
            assert ht.has_wrap(model) and model["occ"][0] and model["occ"][-1]
            assert ht.wrapped(model["homes"], model["slots"]) >= 1
        elif cover == ht.E_SMALL:
            assert 2 <= n <= 4 and model["slots"] in (8, 16)
        elif cover == ht.E_ABSENT:
            assert ht.has_absent(model)
        elif cover == ht.E_MANY:
            assert n >= 200 and len(ht.shared_homes(model["homes"])) >= 10
            assert ht.wrapped(model["homes"], model["slots"]) >= 1
        elif cover == ht.HAS_LINKS:
            assert model["n_links"] >= 1
        else:
            raise AssertionError("no predicate for: " + cover)
    if ht.E_GROUP in case["covers"]:  # whoever wins: links found after 1 and after 2 or more steps
        assert sum(len(g) - 1 for g in ht.target_groups(model).values()) >= 2


# ---- the tile table --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ht.TILE_CASES, ids=[c["id"] for c in ht.TILE_CASES])
def test_tile_case_is_what_it_claims(case):
    k, n, kb = case["k"], case["n"], case["kb"]
    key_bits = 2 * k - n
    assert kb == (2 if key_bits <= 16 else 4 if key_bits <= 32 else 8) and (case["keys"] >> U(key_bits) == 0).all()
    homes = ht.tile_homes(case["keys"])
    entries = ht.entries_per_bucket(case["node_sets"], k, n)
    assert (entries > 0).sum() == 1 and len(case["node_sets"]) == ht.TILE_NODES
    for group in (ht.TILE_SLOTS - 1, 0):
        held = sorted(len(case["holders"][int(key)]) for key in case["keys"][homes == group])
        assert len(held) >= 16 and set(range(2, 8)) <= set(held), (group, held)
    if case["cut"]:
        assert entries.max() > ht.TILE
    else:
        assert entries.max() <= ht.TILE
        assert ht.wrapped(homes, ht.TILE_SLOTS) >= 16  # the 16 keys of slot 0 lie behind those that came round
        occ = ht.occupied(homes, ht.TILE_SLOTS)
        assert ht.run_of(occ, 0) == (ht.TILE_SLOTS - 1, 32)
    # nothing vacuous: several classes of distinct sizes, a selection that is neither empty nor everything
    ref = IndexReference(k, case["node_sets"], [[] for _ in range(ht.TILE_NODES)])
    rows, counts = ref.color_classes()
    assert rows.shape[0] >= 10 and np.unique(counts).size >= 3
    chosen = ref.select(min_count=2)
    assert 20 <= chosen.size < ref.n_distinct
    _, ids = ref.class_ids(rows, min_count=2)
    assert np.unique(ids).size >= 3 and 2 * np.unique(ids, return_counts=True)[1].max() <= ids.size
    table = ref.pair_table()
    assert (table[~np.eye(ht.TILE_NODES, dtype=bool)] > 0).all()
