"""The lock-free open-addressing tables under designed collisions and wraps (tests/hash_table_cases.py): the class
table on its count side (ksh_kss_color_classes: the workgroup's table in LDS, the global table, the spill) and on its
look-up side (ksh_kss_select_class_ids, ksh_seq_class_runs: the caller's table), the end table of ksh_spss_links and
the tile table of the index walk, through the public calls of kmersets.capi alone.  Every expected value comes from
tests/index_reference.py, tests/paint_reference.py or tests/spss_links_reference.py; the model of
hash_table_cases.py only chose the inputs (test_hash_table_model_cpu.py checks that they are what they claim).  Every
comparison is integer or array equality."""
import ctypes as C

import numpy as np
import pytest
import torch

import hash_table_cases as ht
import paint_reference as pr
import spss_links_reference as lref
from index_reference import IndexReference
from kmersets import capi

pytestmark = pytest.mark.gpu

U = np.uint64
GUARD = 0xA5A5A5A5A5A5A5A5
TAIL, PATTERN, KEY_BYTE = 64, 0x5A5A5A5A, 0xA5
COUNT_BY_ID = {c["id"]: c for c in ht.COUNT_CASES}
PERM = ht.permutation(128)


@pytest.fixture(scope="module")
def ctx(gpu):
    c = capi.Context(0)
    yield c
    c.close()


def kmer_strings(kmers, k):
    return ["".join("ACGT"[(int(x) >> (2 * (k - 1 - j))) & 3] for j in range(k)) for x in kmers]


@pytest.fixture(scope="module")
def built(ctx):
    """key -> (index, reference) of nodes without edges: made once per structure, shared and left unchanged."""
    made = {}

    def get(key, k, n, node_sets, canonical=False):
        if key not in made:
            g = capi.geom(k, n)
            comps = [capi.DeviceSpss.from_strings(g, kmer_strings(s, k), ctx.device) for s in node_sets]
            none = [[] for _ in node_sets]
            made[key] = (capi.KssIndex.from_nodes(ctx, comps, none, canonical=canonical),
                         IndexReference(k, node_sets, none))
        return made[key]

    yield get
    for idx, _ in made.values():
        idx.close()


def class_structure(built, case, perm=None):
    return built((case["id"], case["family"], perm is not None), case["k"], case["n"], ht.case_structure(case, perm)[0])


# ---- the class table: count side -------------------------------------------------------------------------------------
def raw_call(idx, cols, capacity, room, guard=GUARD):
    """The C call with host arrays of `room` >= capacity classes filled with a guard pattern (the recipe of
    tests/test_gpu_classes.py, copied: importing a test module would collect its tests twice)."""
    ids = (C.c_int32 * len(cols))(*cols)
    rows = np.full(2 * room, guard, dtype=np.uint64)
    counts = np.full(room, guard, dtype=np.uint64).view(np.int64)
    n = C.c_int64(-1)
    rc = capi.lib().ksh_kss_color_classes(ids, len(cols), idx._handle(), capacity,
                                          rows.ctypes.data_as(C.POINTER(C.c_uint64)),
                                          counts.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(n))
    return rc, n.value, rows, counts.view(np.uint64), capi.lib().ksh_last_error()


def check_exact(idx, cols, capacity, want):
    n = want[1].size
    rc, n_classes, rows, counts, _ = raw_call(idx, cols, capacity, capacity + 8)
    assert rc == capi.KSH_OK and n_classes == n
    print("classes: %d, counts %s" % (n_classes, counts[:n].tolist() if n <= 16 else "..."))
    assert np.array_equal(rows[:2 * n].reshape(-1, 2), want[0])
    assert np.array_equal(counts[:n].view(np.int64), want[1])
    assert (rows[2 * n:] == GUARD).all() and (counts[n:] == GUARD).all()


@pytest.mark.parametrize("case", ht.COUNT_CASES, ids=[c["id"] for c in ht.COUNT_CASES])
def test_count_side(built, case):
    idx, ref = class_structure(built, case)
    cols = list(range(case["n_cols"]))
    want = ref.color_classes()
    check_exact(idx, cols, case["capacity"], want)
    routes = idx.routes()
    if ht.ONE_TILE in case["covers"]:
        assert not routes & (capi.QROUTE_PAIR_SPLIT | capi.QROUTE_CLASS_SPILL)
    assert bool(routes & capi.QROUTE_CLASS_SPILL) == (ht.SPILL in case["covers"])
    check_exact(idx, cols, case["capacity"], want)  # the call made twice: fresh tables each time
    rows, counts = idx.color_classes()  # cols = NULL and the wrapper's capacity: a global table of 2^17 slots
    assert np.array_equal(rows, want[0]) and np.array_equal(counts, want[1])
    table, n_distinct = idx.pair_counts(with_distinct=True)  # the marginals of the classes are the pair table
    m = capi.KssIndex.class_matrix(rows, case["n_cols"]).astype(np.int64)
    assert n_distinct == counts.sum() and np.array_equal(table, m.T @ (m * counts[:, None]))


@pytest.mark.parametrize("cid,capacity", ht.REFUSALS, ids=["%s-cap%d" % r for r in ht.REFUSALS])
def test_capacity_below_the_class_count(built, cid, capacity):
    case = COUNT_BY_ID[cid]
    idx, ref = class_structure(built, case)
    cols = list(range(case["n_cols"]))
    rc, n_classes, rows, counts, msg = raw_call(idx, cols, capacity, capacity + 8)
    assert rc == capi.KSH_FAILED_PRECONDITION and n_classes == capacity + 1 and b"capacity" in msg
    assert (rows[2 * capacity:] == GUARD).all() and (counts[capacity:] == GUARD).all()
    check_exact(idx, cols, case["capacity"], ref.color_classes())  # the index serves the exact capacity afterwards


# ---- the class table: look-up side -----------------------------------------------------------------------------------
def fresh_ids(ctx, g, n_keys):
    with torch.cuda.stream(ctx.stream):
        return (torch.full(((n_keys + TAIL) * g.key_bytes,), KEY_BYTE, dtype=torch.uint8, device=ctx.device),
                torch.full((n_keys + TAIL,), PATTERN, dtype=torch.int32, device=ctx.device))


def host_runs(result):
    off, start, cls, missing = result
    return off.cpu().numpy(), start.cpu().numpy(), cls.cpu().numpy(), missing


def same_runs(got, want):
    return all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3])) and got[3] == want[3]


@pytest.mark.parametrize("permuted", [False, True], ids=["identity", "permuted"])
@pytest.mark.parametrize("case", ht.LOOKUP_CASES, ids=[c["id"] for c in ht.LOOKUP_CASES])
def test_lookup_side(ctx, built, case, permuted):
    """The permuted structure holds the k-mers of column a in node PERM[a], so the column list PERM projects its rows
    onto the designed ones: both runs look the same rows up in the same table."""
    perm = PERM if permuted else None
    idx, ref = class_structure(built, case, perm)
    g, table = idx.g, case["table"]
    want_kmers, want_ids = ref.class_ids(table, cols=perm)
    want_off, want_keys = ref.bucketed(want_kmers, g.n_bucket_bits, g.key_bytes)
    n_keys, n_none = int(want_kmers.size), int((want_ids < 0).sum())
    off, got_n, _ = idx.select_count(cols=perm)
    assert got_n == n_keys and np.array_equal(off.cpu().numpy(), want_off)
    keys, ids = fresh_ids(ctx, g, n_keys)
    missing = idx.select_class_ids(off, n_keys, table, keys, ids, cols=perm, allow_unmatched=True)
    raw_keys, raw_ids = keys.cpu().numpy(), ids.cpu().numpy()
    got_ids = raw_ids[:n_keys].astype(np.int64)
    print("ids %s, unmatched %d of %d" % (np.unique(got_ids).tolist(), missing, n_keys))
    assert np.array_equal(got_ids, want_ids) and missing == n_none
    assert np.array_equal(raw_ids[:n_keys].view(np.uint32) == capi.CLASS_NONE, want_ids < 0)
    assert np.array_equal(raw_keys[:n_keys * g.key_bytes].view(capi.KEY_DTYPE[g.key_bytes]), want_keys)
    assert (raw_keys[n_keys * g.key_bytes:] == KEY_BYTE).all() and (raw_ids[n_keys:] == PATTERN).all()
    with pytest.raises(capi.KshError) as e:  # without n_unmatched the absent rows are a refusal
        idx.select_class_ids(off, n_keys, table, keys, ids, cols=perm)
    assert e.value.code == capi.KSH_FAILED_PRECONDITION and "%d selected" % n_none in str(e.value)
    # ksh_seq_class_runs reads the same table: every k-mer of the structure as a sequence of its own
    strings = kmer_strings(ref.kmers, ref.k)
    want = pr.class_runs(ref, strings, perm, table, False)
    assert want[3] == n_none and np.array_equal(np.sort(want[2]), np.sort(want_ids))
    got = host_runs(idx.class_runs(strings, table, perm, canonicalize=False, route=1))
    assert same_runs(got, want)


@pytest.fixture(scope="module")
def painted(built):
    p = ht.PAINT
    idx, ref = built("paint", p["k"], p["n"], p["node_sets"], canonical=True)
    return idx, ref, pr.class_runs(ref, p["strings"], None, p["table"], True)


@pytest.mark.parametrize("pass_positions", ht.PAINT_PASSES)
def test_paint_alternating_rows(ctx, painted, pass_positions):
    idx, ref, want = painted
    p = ht.PAINT
    dseqs = capi.DeviceSpss.from_strings(idx.g, p["strings"], ctx.device)
    got = host_runs(idx.class_runs(dseqs, p["table"], None, route=1, pass_positions=pass_positions))
    print("runs %d, unmatched %d" % (got[0][-1], got[3]))
    assert same_runs(got, want)
    assert bool(idx.routes() & capi.QROUTE_SEQ_PASSES) == (0 < pass_positions < p["pattern"].size)


# ---- the end table ---------------------------------------------------------------------------------------------------
MODAL = [(c, m) for c in ht.LINK_CASES for m in c["modes"]]


@pytest.fixture(scope="module")
def links_want():
    return {(c["id"], m): lref.links(c["strings"], c["k"], m) for c, m in MODAL}


@pytest.mark.parametrize("case,canonical", MODAL,
                         ids=["%s-run-%s" % (c["id"], "canonical" if m else "directed") for c, m in MODAL])
def test_links(ctx, links_want, case, canonical):
    want_off, want_to = links_want[(case["id"], canonical)]
    n, n_links = len(case["strings"]), int(want_to.size)
    k = case["k"]
    seqs = capi.DeviceSpss.from_strings(capi.geom(k, 10 if k > 5 else 4), case["strings"], ctx.device)
    off, to = ctx.spss_links(seqs, canonical=canonical)  # one call counts, a second one fills
    print("links %d of %d strings" % (to.numel(), n))
    assert np.array_equal(off.cpu().numpy(), want_off) and np.array_equal(to.cpu().numpy(), want_to)
    if n_links:  # the exact capacity in one call, and nothing behind either output
        g_off = torch.full((2 * n + 1 + TAIL,), PATTERN, dtype=torch.int64, device=ctx.device)
        g_to = torch.full((n_links + TAIL,), PATTERN, dtype=torch.int64, device=ctx.device)
        assert ctx.spss_links_raw(seqs, canonical, n_links, g_off, g_to) == (capi.KSH_OK, n_links)
        assert np.array_equal(g_off[:2 * n + 1].cpu().numpy(), want_off)
        assert np.array_equal(g_to[:n_links].cpu().numpy(), want_to)
        assert bool((g_off[2 * n + 1:] == PATTERN).all()) and bool((g_to[n_links:] == PATTERN).all())


# ---- the tile table --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ht.TILE_CASES, ids=[c["id"] for c in ht.TILE_CASES])
def test_tile_table(ctx, built, case):
    idx, ref = built(case["id"], case["k"], case["n"], case["node_sets"])
    g = idx.g
    assert g.key_bytes == case["kb"]

    def cut():
        assert bool(idx.routes() & capi.QROUTE_PAIR_SPLIT) == case["cut"]

    table, n_distinct = idx.pair_counts(with_distinct=True)
    cut()
    assert np.array_equal(table, ref.pair_table()) and n_distinct == ref.n_distinct
    for request in (dict(min_count=2), dict(cols=[6, 2, 4, 0], min_count=1)):
        chosen = idx.select(**request)
        cut()
        want = ref.select(**request)
        assert chosen.n_keys == want.size and np.array_equal(chosen.kmers(), want)
        assert np.array_equal(chosen.to_numpy()[1], ref.bucketed(want, g.n_bucket_bits, g.key_bytes)[1])
    rows, counts = idx.color_classes()
    cut()
    want_rows, want_counts = ref.color_classes()
    assert np.array_equal(rows, want_rows) and np.array_equal(counts, want_counts)
    for request in (dict(), dict(min_count=2)):
        ds, ids, _, _ = idx.select_classes(rows=want_rows, **request)
        cut()
        want_kmers, want_ids = ref.class_ids(want_rows, **request)
        assert np.array_equal(ds.kmers(), want_kmers) and np.array_equal(ids.cpu().numpy().astype(np.int64), want_ids)
