"""The colour class of every selected k-mer (ksh_kss_select_class_ids, capi.KssIndex.select_classes /
select_class_ids).  The expected keys and ids come from numpy alone: the membership matrix of the distinct k-mers of
all node sets over the columns (np.isin against the Get(i) k-mers of the oracle, of a numpy closure of a fabricated
DAG, or rank arithmetic), the selection as a predicate on its lines, and the id of a k-mer as the position of its
line in np.unique(lines as (high, low) words, axis=0, return_inverse=True) -- the order ksh_kss_color_classes gives
its table.  Oracle-built structures on a borrowed and an owned index, split tiles, many classes, both column words,
dense keys, many nodes, wide buckets, partial tables, the write guard, and pending plans staying exact.  Every
comparison is integer or array equality."""
import numpy as np
import pytest
import torch

import oracle_lib as ol
from kmersets import capi, synth

pytestmark = pytest.mark.gpu

CASES = [(9, 10, 1, 6, 3000, 11), (15, 14, 2, 8, 20000, 3), (23, 14, 4, 8, 30000, 5), (31, 14, 8, 4, 20000, 7)]
EMPTY = np.zeros(0, dtype=np.uint64)
ONES = (1 << 64) - 1


@pytest.fixture(scope="module")
def ctx(gpu):
    c = capi.Context(0)
    yield c
    c.close()


# ---- recipes of tests/test_gpu_classes.py (copied: importing a test module would collect its tests twice) ---------
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


def pack_rows(bits):
    """bool[n, n_cols] -> uint64[n, 2], bit a of the row = column a."""
    wide = np.zeros((bits.shape[0], 128), dtype=bool)
    wide[:, :bits.shape[1]] = bits
    return np.packbits(wide, axis=1, bitorder="little").view(np.uint64).reshape(-1, 2)


# ---- the numpy reference ---------------------------------------------------------------------------------------
class Reference:
    """The distinct k-mers `every` (ascending) of all node sets with their membership matrix over the columns."""

    def __init__(self, every, bits, cols):
        self.every, self.bits, self.cols = every, bits, list(cols)
        self.arg = self.cols  # what the calls are given for cols: the list, or None where it is all nodes in order
        self.rows = pack_rows(bits)
        if every.size:  # the class table: distinct lines, ascending by (high, low); line -> its position
            u, inv = np.unique(self.rows[:, ::-1], axis=0, return_inverse=True)
            self.table, self.cls = np.ascontiguousarray(u[:, ::-1]), inv.reshape(-1).astype(np.int64)
        else:
            self.table, self.cls = np.zeros((0, 2), dtype=np.uint64), np.zeros(0, dtype=np.int64)
        self.counts = np.bincount(self.cls, minlength=self.table.shape[0]).astype(np.int64)

    @classmethod
    def of_gets(cls, gets, every, cols):
        cols = list(cols)
        return cls(every, np.stack([np.isin(every, gets[c]) for c in cols], axis=1), cols)

    def chosen(self, lo=1, hi=None, require=(), exclude=()):
        c = self.bits.sum(axis=1)
        keep = (c >= lo) & (c <= (len(self.cols) if hi is None else hi))
        for r in require:
            keep &= self.bits[:, self.cols.index(r)]
        for x in exclude:
            keep &= ~self.bits[:, self.cols.index(x)]
        return keep

    def ids_in(self, keep, table):
        """int32 ids of the kept k-mers in `table` (any subset of lines), -1 where it does not hold the line."""
        at = {(int(r[0]), int(r[1])): c for c, r in enumerate(np.asarray(table, dtype=np.uint64).reshape(-1, 2))}
        per_class = np.array([at.get((int(r[0]), int(r[1])), -1) for r in self.table], dtype=np.int32)
        return per_class[self.cls[keep]] if keep.any() else np.zeros(0, dtype=np.int32)


def host_ids(ids):
    assert ids.dtype == torch.int32 and ids.is_cuda
    return ids.cpu().numpy()


def check_request(idx, ref, lo=1, hi=None, require=(), exclude=(), rows=None):
    """select_classes equals the reference; its keys are those of select(); the ids without keys are the same ids."""
    keep = ref.chosen(lo, hi, require, exclude)
    want_keys = ref.every[keep]
    ds, ids, table, counts = idx.select_classes(ref.arg, lo, hi, require, exclude, rows=rows)
    if rows is None:
        assert table.dtype == np.uint64 and np.array_equal(table, ref.table) and np.array_equal(counts, ref.counts)
    else:
        assert table is rows and counts is None
    want_ids = ref.ids_in(keep, table)
    got = host_ids(ids)
    assert ds.n_keys == want_keys.size and got.shape == (want_keys.size,)
    kmers = ds.kmers()
    assert np.array_equal(kmers, want_keys)
    assert np.array_equal(got, want_ids)
    assert (want_ids >= 0).all()
    plain = idx.select(ref.arg, lo, hi, require, exclude)
    assert np.array_equal(plain.kmers(), kmers)
    assert np.array_equal(plain.offsets.cpu().numpy(), ds.offsets.cpu().numpy())
    alone = torch.full((max(ds.n_keys, 1),), 0x5A5A5A5A, dtype=torch.int32, device=ids.device)
    idx.select_class_ids(ds.offsets, ds.n_keys, table, None, alone, ref.arg, lo, hi, require, exclude)  # d_keys = NULL
    assert np.array_equal(alone[:ds.n_keys].cpu().numpy(), want_ids)
    return want_keys.size, got


def check_histogram(ref, union_ids):
    """The ids of the union selection counted per class are the counts of the class table; the zero row has none."""
    hist = np.bincount(union_ids, minlength=ref.table.shape[0])
    zero = ~ref.table.any(axis=1)
    assert np.array_equal(hist[~zero], ref.counts[~zero]) and not hist[zero].any()


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
def test_class_ids_vs_oracle(ctx, built, which):
    """The inputs as columns, a mix with internal nodes, and all nodes, on an index that borrows the structure's sets
    and on one that decodes the node containers: the union, the core, private to one column, in two but not in a
    third."""
    case = CASES[which]
    k, n, kb, n_sets = case[:4]
    dkss, gets, every = built(case)
    n_nodes = len(gets)
    inputs = list(range(n_sets))
    inner = list(range(n_sets, n_nodes))[::-1][:5]
    assert len(inner) >= 2
    g = capi.geom(k, n)
    assert g.key_bytes == max(kb, 2)
    column_sets = [inputs, [inner[0], 1, inner[1], 0]] + ([list(range(n_nodes))] if n_nodes <= 128 else [])
    refs = [Reference.of_gets(gets, every, cols) for cols in column_sets]
    if n_nodes <= 128:
        refs[-1].arg = None  # cols = NULL
    comps = [capi.DeviceSpss.from_strings(g, dkss.node_strings(i), ctx.device) for i in range(n_nodes)]
    owned = capi.KssIndex.from_nodes(ctx, comps, [dkss.children(i) for i in range(n_nodes)])
    borrowed = capi.KssIndex.from_kss(dkss)
    for idx in (borrowed, owned):
        sizes = []
        for ref in refs:
            cols = ref.cols
            n_union, union_ids = check_request(idx, ref)
            assert not idx.routes() & capi.QROUTE_PAIR_SPLIT  # these buckets fit one tile each
            check_histogram(ref, union_ids)
            rows, counts = idx.color_classes(ref.arg)
            assert np.array_equal(np.bincount(union_ids, minlength=counts.size)[rows.any(axis=1)],
                                  counts[rows.any(axis=1)])
            sizes.append((n_union, check_request(idx, ref, lo=len(cols))[0],
                          check_request(idx, ref, hi=1, require=[cols[1]], rows=rows)[0],
                          check_request(idx, ref, require=cols[:2], exclude=[cols[2]])[0]))
        print("(union, core, private, a & b \\ c) per column set:", sizes)
        assert all(sizes[0])  # over the inputs no selection is empty
    owned.close()
    borrowed.close()


def test_split_tiles(ctx):
    """(15, 4): 16 buckets of about 10^4 entries, a tile holds 512: every bucket is cut by key range many times.  The
    ids must follow their keys through each tile's sort and across the tiles of a bucket."""
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
    for cols in (list(range(n_sets)), [6, 0, 3]):
        ref = Reference.of_gets(gets, every, cols)
        assert ref.table.shape[0] > 2
        n_union, union_ids = check_request(idx, ref)
        assert idx.routes() & capi.QROUTE_PAIR_SPLIT
        check_histogram(ref, union_ids)
        assert np.unique(union_ids).size > 2
        ds = idx.select_classes(cols)[0]
        off, kmers = ds.offsets.cpu().numpy(), ds.kmers()
        for b in range(1 << n):  # every bucket ascending
            assert np.all(np.diff(kmers[off[b]:off[b + 1]].astype(np.int64)) > 0)
        assert check_request(idx, ref, lo=2, hi=len(cols) - 1)[0] > 0
    idx.close()


def test_many_classes(ctx):
    """(15, 4), 20 nodes without edges, 30000 k-mers each in a node with probability 1/2: 29583 classes, the largest
    of 3 k-mers.  Almost every lane of a wave holds a different row, so a wave makes up to 64 look-ups side by side,
    and the table of 2^16 slots is probed at 0.45 load."""
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
    ref = Reference.of_gets(node_sets, every, cols)
    assert ref.table.shape[0] == 29583 and ref.counts.max() == 3 and ref.table.any(axis=1).all()
    idx = capi.KssIndex.from_nodes(ctx, comps, [[] for _ in range(n_nodes)])
    n_union, union_ids = check_request(idx, ref)  # the table color_classes makes
    assert idx.routes() & capi.QROUTE_PAIR_SPLIT
    assert n_union == every.size
    check_histogram(ref, union_ids)
    given = ref.table.copy()  # n_classes = 29583 exactly, from the caller
    assert given.shape == (29583, 2)
    check_request(idx, ref, rows=given)
    check_request(idx, ref, lo=9, hi=11, require=[3], exclude=[17], rows=given)
    idx.close()


@pytest.fixture(scope="module")
def two_words(ctx):
    """The 131 fabricated nodes of tests/test_gpu_classes.py: the columns are nodes 0 .. 127.  Node 63 is reached by
    the columns 0 .. 63 and node 127 by 64 .. 127 (each by itself and the columns before it), node 128 by 0 .. 64,
    the sink 130 by every column, and the root 129 by none.  Each of the five holds k-mers that no other node holds."""
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
    yield idx, gets, every, {j: own[s] for j, s in special.items()}
    idx.close()


@pytest.mark.parametrize("n_cols,present", [
    (128, [(ONES, 0, 63), (0, ONES, 127), (ONES, 1, 128), (ONES, ONES, 130)]),
    (64, [(ONES, 0, 63)]),
    (65, [(ONES, 0, 63), (ONES, 1, 128)])])
def test_both_column_words(two_words, n_cols, present):
    """The rows (~0, 0), (~0, 1), (0, ~0), (~0, ~0) share a word with another row and leave no word a value to spare:
    a look-up that compared fewer than all three key words, or took a row word for "empty", would mix them up."""
    idx, gets, every, own = two_words
    cols = list(range(n_cols))
    ref = Reference.of_gets(gets, every, cols)
    have = {(int(r[0]), int(r[1])): c for c, r in enumerate(ref.table)}
    n_union, union_ids = check_request(idx, ref)
    check_histogram(ref, union_ids)
    kmers = ref.every[ref.chosen()]
    for r0, r1, node in present:  # the reference itself holds the rows the case is about
        assert (r0, r1) in have and ref.counts[have[(r0, r1)]] >= 5, (hex(r0), hex(r1), node)
        at = np.searchsorted(kmers, own[node])
        assert np.array_equal(kmers[at], own[node])
        assert (union_ids[at] == have[(r0, r1)]).all(), node
    assert not np.isin(own[129], kmers).any()  # the root's own k-mers are in no column: the union leaves them out
    shuffled = [int(c) for c in np.random.default_rng(n_cols).permutation(128)[:n_cols]]
    check_request(idx, Reference.of_gets(gets, every, shuffled))


def test_dense_keys(ctx):
    """Every canonical 9-mer (131 072 of them; k = 9, N = 10: every bucket full, consecutive keys, so the cut ends at
    single-key tiles).  Node j holds the k-mers whose rank is divisible by m_j.  Expected from the ranks."""
    k, n = 9, 10
    g = capi.geom(k, n)
    every = np.unique(synth.canonical(np.arange(1 << (2 * k), dtype=np.uint64), k))
    assert every.size == 131072
    rank = np.arange(every.size)
    mods = (1, 2, 3, 5, 7, 4)
    children = [[], [5], [4], [4, 5], [], []]
    comps = [ctx.spss_encode(capi.DeviceSet.from_kmers(g, every[rank % m == 0], ctx.device), mode=0) for m in mods]
    direct = np.stack([rank % m == 0 for m in mods])
    member = (closure(len(mods), children).T.astype(np.int64) @ direct.astype(np.int64)) > 0  # [i, rank]: in Get(i)
    idx = capi.KssIndex.from_nodes(ctx, comps, children)
    ref = Reference(every, member.T.copy(), range(len(mods)))
    assert ref.table.shape[0] > 8
    n_union, union_ids = check_request(idx, ref)
    assert n_union == every.size
    check_histogram(ref, union_ids)
    cols = [3, 2, 1]
    ref = Reference(every, member[cols].T.copy(), cols)
    assert check_request(idx, ref, require=[1, 3], exclude=[2])[0] > 0
    assert check_request(idx, ref)[0] < every.size  # (some k-mers are in none of the three: the zero row, left out)
    idx.close()


def test_many_nodes(ctx):
    """450 nodes, more than the workgroup has threads: nearly empty nodes -- 3 k-mers of a common pool each, every
    third one empty -- and six columns that reach overlapping runs of them."""
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
    ref = Reference.of_gets(gets, every, cols)
    assert ref.table.shape[0] > 8 and not ref.table[0].any()
    idx = capi.KssIndex.from_nodes(ctx, comps, children)
    n_union, union_ids = check_request(idx, ref)
    assert 0 < n_union < every.size
    check_histogram(ref, union_ids)
    check_request(idx, Reference.of_gets(gets, every, [449, 3, 200]))
    with pytest.raises(capi.KshError) as e:  # cols = NULL on more than 128 nodes
        idx.select_classes(rows=ref.table)
    assert e.value.code == capi.KSH_INVALID_ARGUMENT and "450 nodes" in str(e.value)
    check_request(idx, ref, hi=1)  # still serving
    idx.close()


def test_wide_buckets(ctx):
    """(23, 18): 2^18 buckets, 4 sets of 2 * 10^4 k-mers: most buckets are empty and the workgroups stride over
    them."""
    sets, ocompacts, okss, dkss = build_both(ctx, 23, 18, 4, 4, 20000, 19)
    gets = [okss.get(i).kmers() for i in range(okss.size())]
    every = np.unique(np.concatenate(gets))  # (Get(i) holds node i)
    idx = capi.KssIndex.from_kss(dkss)
    for cols in (list(range(4)), list(range(okss.size()))[::-1][:6]):
        ref = Reference.of_gets(gets, every, cols)
        assert ref.table.shape[0] > 2
        n_union, union_ids = check_request(idx, ref)
        check_histogram(ref, union_ids)
        assert check_request(idx, ref, hi=1)[0] > 0
    idx.close()
    dkss.close()


def test_partial_table(ctx, built):
    """Only the one-bit rows: with allow_unmatched every other k-mer reads CLASS_NONE and the call counts them;
    without it the call is refused by name and the index serves afterwards.  A table with a bit at or above n_cols
    is that of other columns."""
    case = CASES[1]
    n_sets = case[3]
    dkss, gets, every = built(case)
    cols = list(range(n_sets))
    ref = Reference.of_gets(gets, every, cols)
    one_bit = ref.table[np.unpackbits(ref.table.view(np.uint8), axis=1).sum(axis=1) == 1]
    assert one_bit.shape[0] == n_sets and ref.table.shape[0] > n_sets
    keep = ref.chosen()
    want = ref.ids_in(keep, one_bit)
    missing = int((want < 0).sum())
    assert 0 < missing < want.size
    idx = capi.KssIndex.from_kss(dkss)
    ds, ids, rows, counts = idx.select_classes(cols, rows=one_bit, allow_unmatched=True)
    assert rows is one_bit and counts is None
    assert np.array_equal(ds.kmers(), every[keep])
    got = host_ids(ids)
    assert np.array_equal(got, want)
    assert np.array_equal(got.view(np.uint32) == capi.CLASS_NONE, want < 0)
    off, n, _ = idx.select_count(cols)
    again = torch.empty(n, dtype=torch.int32, device=ctx.device)
    assert idx.select_class_ids(off, n, one_bit, None, again, cols, allow_unmatched=True) == missing
    assert np.array_equal(again.cpu().numpy(), want)
    assert idx.select_class_ids(off, n, ref.table, None, again, cols, allow_unmatched=True) == 0
    with pytest.raises(capi.KshError) as e:
        idx.select_classes(cols, rows=one_bit)
    assert e.value.code == capi.KSH_FAILED_PRECONDITION and "rows" in str(e.value) and str(missing) in str(e.value)
    check_request(idx, ref)  # still serving
    # the private k-mers alone need no more than the one-bit rows
    assert check_request(idx, ref, hi=1, rows=one_bit)[0] == want.size - missing

    for bad in (np.array([[1, 0], [1 << n_sets, 0]], dtype=np.uint64), np.array([[1, 0], [1, 1]], dtype=np.uint64)):
        for allow in (False, True):
            with pytest.raises(capi.KshError) as e:
                idx.select_classes(cols, rows=bad, allow_unmatched=allow)
            assert e.value.code == capi.KSH_INVALID_ARGUMENT and "n_cols" in str(e.value) and "rows[1]" in str(e.value)
    check_request(idx, ref, lo=n_sets)
    idx.close()


def test_write_guard(ctx, built):
    """The offsets of the union with the request of the core: KSH_FAILED_PRECONDITION, and nothing written at or
    beyond the n_keys keys and ids the call was given.  (The buffers hold every distinct k-mer of the structure, so
    even a wrong kernel stays inside them.)  A correct call on the same index is exact afterwards; a call for
    nothing takes no buffers; an index without k-mers gives nothing."""
    case = CASES[2]
    n_sets = case[3]
    dkss, gets, every = built(case)
    distinct = int(every.size)
    inputs = list(range(n_sets))
    ref = Reference.of_gets(gets, every, inputs)
    idx = capi.KssIndex.from_kss(dkss)
    kb = idx.g.key_bytes
    off_union, n_union, _ = idx.select_count(inputs)
    off_core, n_core, _ = idx.select_count(inputs, n_sets)
    assert 0 < n_core < n_union <= distinct
    keys = torch.full((distinct * kb,), 0xA5, dtype=torch.uint8, device=ctx.device)
    ids = torch.full((distinct,), 0x5A5A5A5A, dtype=torch.int32, device=ctx.device)

    def untouched():
        return bool((keys[n_core * kb:] == 0xA5).all()) and bool((ids[n_core:] == 0x5A5A5A5A).all())

    for allow in (False, True):
        with pytest.raises(capi.KshError) as e:
            idx.select_class_ids(off_union, n_core, ref.table, keys, ids, inputs, n_sets, allow_unmatched=allow)
        assert e.value.code == capi.KSH_FAILED_PRECONDITION and "ksh_kss_select_class_ids" in str(e.value)
        assert "d_offsets" in str(e.value) and untouched()
    with pytest.raises(capi.KshError) as e:  # the right offsets, too little room
        idx.select_class_ids(off_core, n_core - 1, ref.table, keys, ids, inputs, n_sets)
    assert e.value.code == capi.KSH_FAILED_PRECONDITION and untouched()
    idx.select_class_ids(off_core, n_core, ref.table, keys, ids, inputs, n_sets)
    assert untouched()
    core = ref.chosen(lo=n_sets)
    assert np.array_equal(capi.DeviceSet(idx.g, off_core, keys, n_core).kmers(), every[core])
    assert np.array_equal(ids[:n_core].cpu().numpy(), ref.ids_in(core, ref.table))

    # nothing selected (require a, exclude b with Get(b) holding Get(a)): zero offsets, no buffers
    b = next(i for i in range(len(gets)) if dkss.children(i))
    a = dkss.children(b)[0]
    off, n, _ = idx.select_count([a, b], require=[a], exclude=[b])
    assert n == 0 and not off.cpu().numpy().any()
    one_row = np.array([[3, 0]], dtype=np.uint64)
    assert idx.select_class_ids(off, 0, one_row, None, None, [a, b], require=[a], exclude=[b]) is None
    assert idx.select_class_ids(off, 0, one_row, None, None, [a, b], require=[a], exclude=[b],
                                allow_unmatched=True) == 0
    assert untouched()
    idx.close()

    g = capi.geom(15, 10)
    nothing = [capi.DeviceSpss.from_strings(g, [], ctx.device) for _ in range(3)]
    idx = capi.KssIndex.from_nodes(ctx, nothing, [[1], [2], []])
    for cols in (None, [2, 0]):
        ds, got, rows, counts = idx.select_classes(cols)
        assert ds.n_keys == 0 and got.numel() == 0 and rows.shape == (0, 2) and counts.shape == (0,)
        off, n, _ = idx.select_count(cols)
        assert n == 0 and idx.select_class_ids(off, 0, one_row, None, None, cols, allow_unmatched=True) == 0
    idx.close()


def test_plans_stay_exact(ctx):
    """One victim of each plan group: plan, the class ids of a structure of the same context, then the write: served,
    and equal to a fresh plan + write (include/kmersets_hip.h, "Plans")."""
    k, n = 23, 14
    g = capi.geom(k, n)
    sets = synth.phylogeny_sets(k, 2, 20000, seed=17)
    a, b = (capi.DeviceSet.from_kmers(g, s, ctx.device) for s in sets)
    ca, cb = ctx.spss_encode(a, mode=0), ctx.spss_encode(b, mode=0)
    idx = capi.KssIndex.from_nodes(ctx, [ca, cb], [[1], []])
    union = np.union1d(sets[0], sets[1]).astype(np.uint64)
    in_b = np.isin(union, sets[1])
    assert 0 < in_b.sum() < union.size
    table = np.array([[1, 0], [3, 0]], dtype=np.uint64)  # Get(0) holds Get(1): a alone has bit 0, b both bits

    def intrude():
        ds, ids, rows, counts = idx.select_classes([0, 1], rows=table)
        assert np.array_equal(ds.kmers(), union) and np.array_equal(host_ids(ids), in_b.astype(np.int32))

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
