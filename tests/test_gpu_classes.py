"""Colour classes of a KmerSetSet index (ksh_kss_color_classes, capi.KssIndex.color_classes): every distinct
membership pattern over the chosen columns with the number of distinct k-mers that have it.  The expected table comes
from numpy alone: the Get(i) k-mers of the columns (the oracle's, or a numpy closure of a fabricated DAG), a row per
distinct k-mer of all node sets with np.isin, np.unique(rows, axis=0, return_counts=True), sorted as the call sorts.
The contended insertion (few classes, every workgroup), split tiles, many classes (the spill and the probing), the
capacity refusal and its guard, both column words and the rows that leave no value to spare, wide buckets, empty
indexes, the refusals that read the index, and pending plans staying exact.  Every comparison is integer or array
equality."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle_lib as ol
from kmersets import capi, synth

pytestmark = pytest.mark.gpu

CASES = [(9, 10, 1, 6, 3000, 11), (15, 14, 2, 8, 20000, 3), (23, 14, 4, 8, 30000, 5), (31, 14, 8, 4, 20000, 7)]
# of the inputs of each case, from the oracle on the CPU: (distinct k-mers, classes, largest class, smallest class)
INPUT_CLASSES = [(3538, 29, 2462, 2), (28223, 82, 13153, 1), (49435, 112, 15016, 1), (27223, 15, 13760, 32)]
EMPTY = np.zeros(0, dtype=np.uint64)
ONES = (1 << 64) - 1


@pytest.fixture(scope="module")
def ctx(gpu):
    c = capi.Context(0)
    yield c
    c.close()


# ---- recipes of tests/test_gpu_select.py (copied: importing a test module would collect its tests twice) ----------
def build_both(ctx, k, n, kb, n_sets, size, seed, max_iterations=-1):
    sets = synth.phylogeny_sets(k, n_sets, size, seed=seed)
    osets = [ol.Set.from_kmers(k, n, kb, s) for s in sets]
    ocompacts = [s.compact() for s in osets]
    ids = synth.sample_bucket_ids(n, seed=seed + 1)
    okss = ol.KmerSetSet(ocompacts, ids, max_iterations=max_iterations)
    g = capi.geom(k, n)
    dcompacts = [capi.DeviceSpss.from_strings(g, c.strings(), ctx.device) for c in ocompacts]
    dkss = capi.DeviceKmerSetSet(ctx, dcompacts, ids, max_iterations=max_iterations)
    return sets, ocompacts, okss, dkss


def closure(n, children):
    anc = np.eye(n, dtype=bool)  # anc[j, i]: j reachable from i
    indeg = [0] * n
    for i in range(n):
        for c in children[i]:
            indeg[c] += 1
    order = [i for i in range(n) if indeg[i] == 0]
    for p in order:
        for c in children[p]:
            anc[c] |= anc[p]
            indeg[c] -= 1
            if indeg[c] == 0:
                order.append(c)
    return anc


def closure_gets(node_sets, children):
    """Get(i) of a fabricated DAG: the union of the sets of the nodes reachable from i."""
    n = len(node_sets)
    anc = closure(n, children)
    return [np.unique(np.concatenate([EMPTY] + [node_sets[j] for j in range(n) if anc[j, i]])) for i in range(n)]


def kmer_strings(kmers, k):
    return ["".join("ACGT"[(int(x) >> (2 * (k - 1 - j))) & 3] for j in range(k)) for x in kmers]


# ---- the numpy reference ---------------------------------------------------------------------------------------
def pack_rows(bits):
    """bool[n, n_cols] -> uint64[n, 2], bit a of the row = column a."""
    wide = np.zeros((bits.shape[0], 128), dtype=bool)
    wide[:, :bits.shape[1]] = bits
    return np.packbits(wide, axis=1, bitorder="little").view(np.uint64).reshape(-1, 2)


def want_classes(gets, every, cols):
    """(rows, counts) of the distinct k-mers `every` of all node sets over the columns, in the call's order."""
    cols = list(cols)
    if every.size == 0:
        return np.zeros((0, 2), dtype=np.uint64), np.zeros(0, dtype=np.int64)
    bits = np.stack([np.isin(every, gets[c]) for c in cols], axis=1)
    u, cnt = np.unique(bits, axis=0, return_counts=True)
    rows = pack_rows(u)
    order = np.lexsort((rows[:, 0], rows[:, 1]))
    return rows[order], cnt[order].astype(np.int64)


def check_classes(got, want, n_cols=None):
    rows, counts = got
    assert rows.dtype == np.uint64 and counts.dtype == np.int64
    assert rows.shape == (counts.size, 2)
    print("classes: %d of %d k-mers, largest %d, smallest %d"
          % (counts.size, counts.sum(), counts.max() if counts.size else 0, counts.min() if counts.size else 0))
    assert rows.shape == want[0].shape
    assert np.array_equal(rows, want[0])
    assert np.array_equal(counts, want[1])
    if n_cols is not None:  # class_matrix gives the reference's bits back
        assert np.array_equal(pack_rows(capi.KssIndex.class_matrix(rows, n_cols)), rows)


def check_identities(idx, cols, rows, counts):
    """The sum is n_distinct, the spectrum the sum by popcount, the pair table the sum over the classes with both
    bits."""
    n_cols = len(cols)
    m = capi.KssIndex.class_matrix(rows, n_cols).astype(np.int64)
    table, nd = idx.pair_counts(cols=cols, with_distinct=True)
    assert counts.sum() == nd
    spec = np.zeros(n_cols + 1, dtype=np.int64)
    np.add.at(spec, m.sum(axis=1), counts)
    assert np.array_equal(idx.spectrum(cols), spec)
    assert np.array_equal(table, m.T @ (m * counts[:, None]))


@pytest.fixture(scope="module")
def built(ctx):
    """case -> (structure, the oracle's Get(i) k-mers, the distinct k-mers of its node sets): made once per case,
    shared by the tests and left unchanged."""
    made = {}

    def get(case):
        if case not in made:
            k, n, kb, n_sets, size, seed = case
            sets, ocompacts, okss, dkss = build_both(ctx, k, n, kb, n_sets, size, seed)
            gets = [okss.get(i).kmers() for i in range(okss.size())]
            nodes = [okss.node(i).to_set().kmers() for i in range(okss.size())]
            made[case] = (dkss, gets, np.unique(np.concatenate(nodes)))
        return made[case]

    yield get
    for dkss, *_ in made.values():
        dkss.close()


@pytest.mark.parametrize("which", range(len(CASES)))
def test_classes_vs_oracle(ctx, built, which):
    """The inputs as columns (and once internal nodes, and all nodes), on an index that borrows the structure's sets
    and on one that decodes the node containers.  Few classes and every workgroup adds to them: the contended
    insertion.  The class counts are pinned, so no wrong answer hides in an absent class."""
    case = CASES[which]
    k, n, kb, n_sets = case[:4]
    dkss, gets, every = built(case)
    n_nodes = len(gets)
    inputs = list(range(n_sets))
    want = want_classes(gets, every, inputs)
    summary = (int(every.size), int(want[1].size), int(want[1].max()), int(want[1].min()))
    print("expected (distinct, classes, largest, smallest):", summary, "of", (1 << n_sets) - 1, "possible")
    assert summary == INPUT_CLASSES[which]
    inner = list(range(n_sets, n_nodes))[::-1][:5]
    assert len(inner) >= 2
    g = capi.geom(k, n)
    assert g.key_bytes == max(kb, 2)
    comps = [capi.DeviceSpss.from_strings(g, dkss.node_strings(i), ctx.device) for i in range(n_nodes)]
    owned = capi.KssIndex.from_nodes(ctx, comps, [dkss.children(i) for i in range(n_nodes)])
    borrowed = capi.KssIndex.from_kss(dkss)
    for idx in (borrowed, owned):
        got = idx.color_classes(inputs)
        check_classes(got, want, n_sets)
        assert not idx.routes() & (capi.QROUTE_PAIR_SPLIT | capi.QROUTE_CLASS_SPILL)  # one tile per bucket, few classes
        check_identities(idx, inputs, *got)
        got = idx.color_classes(inner)
        check_classes(got, want_classes(gets, every, inner), len(inner))
        assert (got[0] == 0).all(axis=1).any()  # the zero row: k-mers that no chosen internal node holds
        check_identities(idx, inner, *got)
        mixed = [inner[0], 1, inner[1]]
        check_classes(idx.color_classes(mixed), want_classes(gets, every, mixed), 3)
        if n_nodes <= 128:
            check_classes(idx.color_classes(), want_classes(gets, every, range(n_nodes)), n_nodes)  # cols = NULL
    owned.close()
    borrowed.close()


def test_split_tiles(ctx):
    """(15, 4): 16 buckets of about 10^4 entries, a tile holds 512: every bucket is cut by key range many times and
    every tile adds to the same classes.  The nodes are the oracle's containers of 8 sets under a fabricated DAG."""
    k, n, kb, n_sets, size = 15, 4, 4, 8, 20000
    g = capi.geom(k, n)
    sets = synth.phylogeny_sets(k, n_sets, size, seed=31)
    osets = [ol.Set.from_kmers(k, n, kb, s) for s in sets]
    node_sets = [s.kmers() for s in osets]
    comps = [capi.DeviceSpss.from_strings(g, s.compact().strings(), ctx.device) for s in osets]
    children = [[1, 2], [3], [3, 4], [], [5], [], [7], []]
    gets = closure_gets(node_sets, children)
    every = np.unique(np.concatenate(node_sets))
    idx = capi.KssIndex.from_nodes(ctx, comps, children)
    for cols in (list(range(n_sets)), [6, 0, 3], [5]):
        want = want_classes(gets, every, cols)
        assert want[1].size > 1
        got = idx.color_classes(cols)
        assert idx.routes() & capi.QROUTE_PAIR_SPLIT
        check_classes(got, want, len(cols))
        check_identities(idx, cols, *got)
    idx.close()


def raw_call(idx, cols, capacity, room, guard=0xA5A5A5A5A5A5A5A5):
    """The C call with host arrays of `room` >= capacity classes filled with a guard pattern."""
    ids = (C.c_int32 * len(cols))(*cols)
    rows = np.full(2 * room, guard, dtype=np.uint64)
    counts = np.full(room, guard, dtype=np.uint64).view(np.int64)
    n = C.c_int64(-1)
    rc = capi.lib().ksh_kss_color_classes(ids, len(cols), idx._handle(), capacity,
                                          rows.ctypes.data_as(C.POINTER(C.c_uint64)),
                                          counts.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(n))
    return rc, n.value, rows, counts.view(np.uint64), capi.lib().ksh_last_error()


def test_many_classes(ctx):
    """(15, 4), 20 nodes without edges, 30000 k-mers each in a node with probability 1/2: 29583 classes, the largest
    of 3 k-mers, about 1850 k-mers and as many classes per bucket, so each of the 16 workgroups meets far more
    classes than a tile holds: its class table is spilled between tiles (KSH_QROUTE_CLASS_SPILL) and the global
    table is probed at up to half load.  Exactly enough room is enough; one class less, or far too little, is the
    refusal with nothing written behind the capacity; the index serves afterwards."""
    k, n, n_nodes = 15, 4, 20
    g = capi.geom(k, n)
    rng = np.random.default_rng(77)
    pool = np.unique(synth.canonical(rng.integers(0, 1 << 30, 30000), k))
    assert pool.size == 30000
    member = rng.random((n_nodes, 30000)) < 0.5
    node_sets = [pool[member[j]] for j in range(n_nodes)]
    comps = [ctx.spss_encode(capi.DeviceSet.from_kmers(g, s, ctx.device), mode=0) for s in node_sets]
    cols = list(range(n_nodes))
    every = np.unique(np.concatenate(node_sets))
    want = want_classes(node_sets, every, cols)
    assert want[1].size == 29583 and want[1].max() == 3 and want[0].any(axis=1).all()
    idx = capi.KssIndex.from_nodes(ctx, comps, [[] for _ in range(n_nodes)])
    got = idx.color_classes(cols)
    routes = idx.routes()
    check_classes(got, want, n_nodes)
    assert routes & capi.QROUTE_CLASS_SPILL and routes & capi.QROUTE_PAIR_SPLIT
    check_identities(idx, cols, *got)

    check_classes(idx.color_classes(cols, capacity=29583), want)  # exactly enough room
    rc, n_classes, rows, counts, msg = raw_call(idx, cols, 29583, 29583 + 64)
    assert rc == capi.KSH_OK and n_classes == 29583
    assert np.array_equal(rows[:2 * 29583].reshape(-1, 2), want[0]) and np.array_equal(counts[:29583], want[1])
    assert (rows[2 * 29583:] == 0xA5A5A5A5A5A5A5A5).all() and (counts[29583:] == 0xA5A5A5A5A5A5A5A5).all()

    with pytest.raises(capi.KshError) as e:  # a given capacity is tried once
        idx.color_classes(cols, capacity=29582)
    assert e.value.code == capi.KSH_FAILED_PRECONDITION and "capacity" in str(e.value)
    rc, n_classes, rows, counts, msg = raw_call(idx, cols, 29582, 29582 + 64)
    assert rc == capi.KSH_FAILED_PRECONDITION and n_classes == 29583 and b"capacity" in msg
    assert (rows[2 * 29582:] == 0xA5A5A5A5A5A5A5A5).all() and (counts[29582:] == 0xA5A5A5A5A5A5A5A5).all()

    rc, n_classes, rows, counts, msg = raw_call(idx, cols, 1000, 4096)
    assert rc == capi.KSH_FAILED_PRECONDITION and n_classes == 1001 and b"capacity" in msg
    assert (rows[2000:] == 0xA5A5A5A5A5A5A5A5).all() and (counts[1000:] == 0xA5A5A5A5A5A5A5A5).all()

    check_classes(idx.color_classes(cols), want)  # a call with room on the same index
    few = [3, 11]
    check_classes(idx.color_classes(few), want_classes(node_sets, every, few), 2)
    idx.close()


@pytest.fixture(scope="module")
def two_words(ctx):
    """131 fabricated nodes, the columns are nodes 0 .. 127.  Node 63 is reached by the columns 0 .. 63 and node 127
    by 64 .. 127 (each by itself and the columns before it), node 128 by 0 .. 64, the sink 130 by every column, and
    the root 129 by none.  Each of the five holds k-mers that no other node holds, so their rows are in the table:
    (~0, 0), (0, ~0), (~0, 1), (~0, ~0) and zero -- rows that share their first or second word with another and
    that leave no word a value to spare.  The other nodes hold random k-mers of a common pool."""
    k, n, n_nodes = 15, 10, 131
    g = capi.geom(k, n)
    rng = np.random.default_rng(131)
    drawn = np.unique(synth.canonical(rng.integers(0, 1 << 30, 1400), k))
    rng.shuffle(drawn)
    own, pool = drawn[:25].reshape(5, 5), drawn[25:]
    special = {63: 0, 127: 1, 128: 2, 129: 3, 130: 4}
    node_sets = [np.unique(rng.choice(pool, size=12)) for _ in range(n_nodes)]
    for j, s in special.items():
        node_sets[j] = np.unique(np.concatenate([own[s], node_sets[j] if j < 128 else EMPTY]))
    children = [[] for _ in range(n_nodes)]
    for i in range(63):
        children[i].append(63)
    for i in range(64, 127):
        children[i].append(127)
    for i in range(65):
        children[i].append(128)
    for i in (63, 127, 129):
        children[i].append(130)
    comps = [capi.DeviceSpss.from_strings(g, kmer_strings(s, k), ctx.device) for s in node_sets]
    gets = closure_gets(node_sets, children)
    every = np.unique(np.concatenate(node_sets))
    idx = capi.KssIndex.from_nodes(ctx, comps, children)
    yield idx, gets, every, own
    idx.close()


@pytest.mark.parametrize("n_cols,present", [
    (128, [(ONES, 0, 63), (0, ONES, 127), (ONES, 1, 128), (ONES, ONES, 130), (0, 0, 129)]),
    (64, [(ONES, 0, 63), (0, 0, 129)]),
    (65, [(ONES, 0, 63), (ONES, 1, 128), (0, 0, 129)])])
def test_both_column_words(two_words, n_cols, present):
    idx, gets, every, own = two_words
    cols = list(range(n_cols))
    want = want_classes(gets, every, cols)
    have = {(int(r[0]), int(r[1])): int(c) for r, c in zip(*want)}
    for r0, r1, node in present:  # the reference itself holds the rows the case is about
        assert have.get((r0, r1), 0) >= 5, (hex(r0), hex(r1), node)
    got = idx.color_classes(cols)
    check_classes(got, want, n_cols)
    check_identities(idx, cols, *got)
    shuffled = [int(c) for c in np.random.default_rng(n_cols).permutation(128)[:n_cols]]
    check_classes(idx.color_classes(shuffled), want_classes(gets, every, shuffled), n_cols)


def test_refusals_that_read_the_index(two_words):
    idx, gets, every, own = two_words
    serve = want_classes(gets, every, [7, 63])
    for bad, word in ((dict(cols=None), "131 nodes"), (dict(cols=[0, 131]), "outside"), (dict(cols=[-1]), "outside"),
                      (dict(cols=[5, 9, 5]), "repeated"), (dict(cols=list(range(129))), "n_cols"),
                      (dict(cols=[]), "n_cols")):
        with pytest.raises(capi.KshError) as e:
            idx.color_classes(**bad)
        assert e.value.code == capi.KSH_INVALID_ARGUMENT and word in str(e.value), bad
        check_classes(idx.color_classes([7, 63]), serve, 2)  # still serving


def test_wide_buckets(ctx):
    """(23, 18): 2^18 buckets, 4 sets of 2 * 10^4 k-mers: most buckets are empty and the workgroups stride over
    them."""
    sets, ocompacts, okss, dkss = build_both(ctx, 23, 18, 4, 4, 20000, 19)
    gets = [okss.get(i).kmers() for i in range(okss.size())]
    every = np.unique(np.concatenate(gets))  # (Get(i) holds node i)
    idx = capi.KssIndex.from_kss(dkss)
    for cols in (list(range(4)), list(range(okss.size()))[::-1][:6]):
        want = want_classes(gets, every, cols)
        assert want[1].size > 2
        got = idx.color_classes(cols)
        check_classes(got, want, len(cols))
        check_identities(idx, cols, *got)
    idx.close()
    dkss.close()


def test_many_nodes(ctx):
    """450 nodes: the walk's 20 bytes per node take the kernel's LDS past the 64 KiB a kernel gets without asking
    (from 406 nodes on), so the first call asks for more and the second finds it granted.  The nodes are nearly
    empty -- 3 k-mers of a common pool each, every third one empty -- and six columns reach overlapping runs of
    them."""
    k, n, n_nodes = 15, 10, 450
    g = capi.geom(k, n)
    rng = np.random.default_rng(450)
    pool = np.unique(synth.canonical(rng.integers(0, 1 << 30, 1200), k))
    node_sets = [EMPTY if j % 3 == 2 else np.unique(rng.choice(pool, size=3)) for j in range(n_nodes)]
    children = [[] for _ in range(n_nodes)]
    cols = list(range(6))
    for c in cols:
        children[c] = list(range(6 + 60 * c, 6 + 60 * c + 100))
    children[449] = [448]  # (outside every column: the zero row)
    comps = [capi.DeviceSpss.from_strings(g, kmer_strings(s, k), ctx.device) for s in node_sets]
    gets = closure_gets(node_sets, children)
    every = np.unique(np.concatenate(node_sets))
    want = want_classes(gets, every, cols)
    assert want[1].size > 8 and not want[0][0].any()
    idx = capi.KssIndex.from_nodes(ctx, comps, children)
    for _ in range(2):
        got = idx.color_classes(cols)
        check_classes(got, want, len(cols))
    check_identities(idx, cols, *got)
    far = [449, 3, 200]
    check_classes(idx.color_classes(far), want_classes(gets, every, far), 3)
    with pytest.raises(capi.KshError) as e:  # cols = NULL on more than 128 nodes
        idx.color_classes()
    assert e.value.code == capi.KSH_INVALID_ARGUMENT and "450 nodes" in str(e.value)
    idx.close()


def test_empty_index(ctx):
    """An index whose nodes are all empty has no class; empty nodes among full ones are columns without a bit."""
    k, n = 15, 10
    g = capi.geom(k, n)
    nothing = [capi.DeviceSpss.from_strings(g, [], ctx.device) for _ in range(3)]
    idx = capi.KssIndex.from_nodes(ctx, nothing, [[1], [2], []])
    for cols in (None, [2, 0]):
        rows, counts = idx.color_classes(cols)
        assert rows.shape == (0, 2) and counts.shape == (0,)
    rc, n_classes, rows, counts, msg = raw_call(idx, [0, 1, 2], 4, 8)
    assert rc == capi.KSH_OK and n_classes == 0
    assert (rows == 0xA5A5A5A5A5A5A5A5).all() and (counts == 0xA5A5A5A5A5A5A5A5).all()
    idx.close()

    rng = np.random.default_rng(9)
    pool = np.unique(synth.canonical(rng.integers(0, 1 << 30, 200), k))
    node_sets = [EMPTY if j % 2 == 0 else np.unique(rng.choice(pool, size=40)) for j in range(6)]
    children = [[1, 2], [3], [3], [4], [], [4]]
    comps = [capi.DeviceSpss.from_strings(g, kmer_strings(s, k), ctx.device) for s in node_sets]
    gets = closure_gets(node_sets, children)
    every = np.unique(np.concatenate(node_sets))
    idx = capi.KssIndex.from_nodes(ctx, comps, children)
    check_classes(idx.color_classes(), want_classes(gets, every, range(6)), 6)  # cols = NULL
    check_classes(idx.color_classes([4, 2]), want_classes(gets, every, [4, 2]), 2)  # an empty sink, an empty parent
    got = idx.color_classes([4])
    assert got[0].tolist() == [[0, 0]] and got[1].tolist() == [every.size]
    idx.close()


def test_plans_stay_exact(ctx):
    """One victim of each plan group: plan, a class table on a structure of the same context, then the write: served,
    and equal to a fresh plan + write (include/kmersets_hip.h, "Plans")."""
    k, n = 23, 14
    g = capi.geom(k, n)
    sets = synth.phylogeny_sets(k, 2, 20000, seed=17)
    a, b = (capi.DeviceSet.from_kmers(g, s, ctx.device) for s in sets)
    ca, cb = ctx.spss_encode(a, mode=0), ctx.spss_encode(b, mode=0)
    idx = capi.KssIndex.from_nodes(ctx, [ca, cb], [[1], []])
    both, nb = np.union1d(sets[0], sets[1]).size, np.asarray(sets[1]).size
    assert 0 < nb < both

    def intrude():  # Get(0) holds Get(1): the k-mers of a alone have bit 0, those of b both bits
        rows, counts = idx.color_classes([0, 1])
        assert rows.tolist() == [[1, 0], [3, 0]] and counts.tolist() == [both - nb, nb]

    intrude()
    # pair
    fresh = [s.kmers() for s in ctx.pair_algebra(a, b)]
    outs = [capi.DeviceSet.empty_like_offsets(g, 0, ctx.device) for _ in range(3)]
    totals = ctx.pair_plan(a, b, *outs)
    for o, t in zip(outs, totals):
        o.n_keys = t
        o.keys = torch.empty(max(t * g.key_bytes, 16), dtype=torch.uint8, device=ctx.device)
    intrude()
    ctx.pair_write(a, b, *outs)
    assert all(np.array_equal(o.kmers(), f) for o, f in zip(outs, fresh))
    # decode
    fresh = ctx.spss_decode(ca).kmers()
    plan = ctx.spss_decode_plan(ca)
    intrude()
    assert np.array_equal(ctx.spss_decode_write(plan).kmers(), fresh) and np.array_equal(fresh, np.sort(sets[0]))
    # encode
    fresh = ctx.spss_encode(a, mode=0).to_strings()
    plan = ctx.spss_encode_plan(a, mode=0)
    intrude()
    assert ctx.spss_encode_write(plan).to_strings() == fresh
    # text
    text = ctx.spss_to_text(ca)
    fresh = ctx.spss_from_text(g, text).to_strings()
    plan = ctx.spss_from_text_plan(g, text)
    intrude()
    assert ctx.spss_from_text_write(plan).to_strings() == fresh == ca.to_strings()
    idx.close()
