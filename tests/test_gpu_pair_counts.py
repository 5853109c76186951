"""Exact pairwise intersection counts on a KmerSetSet index (ksh_kss_pair_counts, capi.KssIndex.pair_counts /
jaccard): counts[a, b] = |Get(cols[a]) & Get(cols[b])| against the oracle's Get(i) with np.intersect1d, numpy
closures of fabricated DAGs and rank arithmetic on the dense 9-mer space; split tiles, column lists, flushes, wide
buckets, and pending plans of the context staying exact across the call.  Every comparison is integer equality."""
import numpy as np
import pytest
import torch

import oracle_lib as ol
from kmersets import capi, synth

pytestmark = pytest.mark.gpu

CASES = [(9, 10, 1, 6, 3000, 11), (15, 14, 2, 8, 20000, 3), (23, 14, 4, 8, 30000, 5), (31, 14, 8, 4, 20000, 7)]


@pytest.fixture(scope="module")
def ctx(gpu):
    c = capi.Context(0)
    yield c
    c.close()


# ---- recipes of tests/test_gpu_seq_hits.py (copied: importing a test module would collect its tests twice) ----
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


def kmer_strings(kmers, k):
    return ["".join("ACGT"[(int(x) >> (2 * (k - 1 - j))) & 3] for j in range(k)) for x in kmers]


def fabricated(ctx, n_nodes, seed, k=15, n=10, per_node=12, empty_every=0):
    rng = np.random.default_rng(seed)
    g = capi.geom(k, n)
    pool = np.unique(synth.canonical(rng.integers(0, 1 << (2 * k), size=n_nodes * per_node, dtype=np.uint64), k))
    node_sets, comps = [], []
    for i in range(n_nodes):
        s = np.unique(rng.choice(pool, size=per_node)) if not (empty_every and i % empty_every == 0) else \
            np.zeros(0, dtype=np.uint64)
        node_sets.append(s.astype(np.uint64))
        comps.append(capi.DeviceSpss.from_strings(g, kmer_strings(s, k), ctx.device))
    children = [[] for _ in range(n_nodes)]
    for i in range(n_nodes - 1):
        for c in rng.choice(np.arange(i + 1, n_nodes), size=min(2, n_nodes - 1 - i), replace=False):
            children[i].append(int(c))
    return g, pool, node_sets, comps, children


# ---- the numpy references ------------------------------------------------------------------------------------
def pair_table(gets):
    """|a & b| for sorted arrays of distinct k-mers."""
    n = len(gets)
    out = np.zeros((n, n), dtype=np.int64)
    for a in range(n):
        for b in range(a, n):
            out[a, b] = out[b, a] = np.intersect1d(gets[a], gets[b], assume_unique=True).size
    return out


def closure_table(node_sets, children):
    """The table and the number of distinct k-mers of a fabricated DAG: Get(i) = the union of the sets of the nodes
    reachable from i, as a bool matrix over the distinct k-mers of all nodes."""
    n = len(node_sets)
    allk = np.unique(np.concatenate(node_sets)) if n else np.zeros(0, dtype=np.uint64)
    direct = np.stack([np.isin(allk, s) for s in node_sets]).astype(np.int64)  # [j, k-mer]
    member = ((closure(n, children).T.astype(np.int64) @ direct) > 0).astype(np.int64)  # [i, k-mer]
    return member @ member.T, int(allk.size)


def jaccard_of(table):
    d = np.diag(table).astype(np.float64)
    union = d[:, None] + d[None, :] - table
    out = np.ones(table.shape, dtype=np.float64)
    np.divide(table, union, out=out, where=union > 0)
    return out


@pytest.fixture(scope="module")
def built(ctx):
    """case -> (structure, the oracle's node sets and Get(i) sets, the expected table and distinct count): made once
    per case, shared by the tests and left unchanged."""
    made = {}

    def get(case):
        if case not in made:
            k, n, kb, n_sets, size, seed = case
            sets, ocompacts, okss, dkss = build_both(ctx, k, n, kb, n_sets, size, seed)
            gets = [okss.get(i).kmers() for i in range(okss.size())]
            nodes = [okss.node(i).to_set().kmers() for i in range(okss.size())]
            distinct = int(np.unique(np.concatenate(nodes)).size)
            made[case] = (dkss, gets, pair_table(gets), distinct)
        return made[case]

    yield get
    for dkss, *_ in made.values():
        dkss.close()


@pytest.mark.parametrize("case", CASES)
def test_pair_counts_vs_oracle(ctx, built, case):
    """All nodes as columns, on an index that borrows the structure's sets and on one that decodes the node
    containers: the oracle's table, the distinct k-mers of all nodes, symmetry, the diagonal = |Get(i)| of the
    structure itself; these buckets fit one tile each."""
    k, n = case[:2]
    dkss, gets, want, distinct = built(case)
    n_nodes = len(gets)
    off = want[~np.eye(n_nodes, dtype=bool)]
    print("expected table: %d nodes, off-diagonal %d zero, %d non-zero" % (n_nodes, (off == 0).sum(), (off > 0).sum()))
    assert (off > 0).any() and len(set(np.diag(want))) > 1  # a wrong answer cannot hide in a trivial table
    g = capi.geom(k, n)
    comps = [capi.DeviceSpss.from_strings(g, dkss.node_strings(i), ctx.device) for i in range(n_nodes)]
    owned = capi.KssIndex.from_nodes(ctx, comps, [dkss.children(i) for i in range(n_nodes)])
    borrowed = capi.KssIndex.from_kss(dkss)
    for idx in (borrowed, owned):
        got, nd = idx.pair_counts(with_distinct=True)
        assert got.dtype == np.int64 and got.shape == (n_nodes, n_nodes)
        assert np.array_equal(got, want)
        assert nd == distinct
        assert np.array_equal(got, got.T)
        assert not idx.routes() & (capi.QROUTE_PAIR_SPLIT | capi.QROUTE_PAIR_FLUSH)
        dev = idx.pair_counts(device=True)
        assert dev.device.type == "cuda" and dev.dtype == torch.int64 and np.array_equal(dev.cpu().numpy(), want)
    assert [int(x) for x in np.diag(want)] == [dkss.get_size_and_hash(i)[0] for i in range(n_nodes)]
    owned.close()
    borrowed.close()


def test_split_tiles(ctx):
    """(15, 4): 16 buckets.  8 sets of 2 * 10^4 k-mers is the smallest family of the issue's ladder (it starts
    there) that sets QROUTE_PAIR_SPLIT: a bucket holds about 10^4 entries, a tile 512.  The nodes are the oracle's
    containers of the sets under a fabricated DAG; expected from the oracle sets' k-mers and a numpy closure."""
    k, n, kb, n_sets, size = 15, 4, 4, 8, 20000
    g = capi.geom(k, n)
    sets = synth.phylogeny_sets(k, n_sets, size, seed=31)
    osets = [ol.Set.from_kmers(k, n, kb, s) for s in sets]
    comps = [capi.DeviceSpss.from_strings(g, s.compact().strings(), ctx.device) for s in osets]
    children = [[1, 2], [3], [3, 4], [], [5], [], [7], []]
    want, distinct = closure_table([s.kmers() for s in osets], children)
    idx = capi.KssIndex.from_nodes(ctx, comps, children)
    got, nd = idx.pair_counts(with_distinct=True)
    assert idx.routes() & capi.QROUTE_PAIR_SPLIT
    assert np.array_equal(got, want) and nd == distinct
    got = idx.pair_counts(cols=[6, 0, 3], flush_rows=5000)
    assert idx.routes() & capi.QROUTE_PAIR_SPLIT and idx.routes() & capi.QROUTE_PAIR_FLUSH
    assert np.array_equal(got, want[np.ix_([6, 0, 3], [6, 0, 3])])
    idx.close()


def test_dense_keys(ctx):
    """Every canonical 9-mer (131 072 of them; k = 9, N = 10: every bucket full, consecutive keys).  Node j holds the
    k-mers whose rank is divisible by m_j; every k-mer is in node 0.  Encoded on the device; expected counts from
    the ranks."""
    k, n = 9, 10
    g = capi.geom(k, n)
    every = np.unique(synth.canonical(np.arange(1 << (2 * k), dtype=np.uint64), k))
    assert every.size == 131072
    rank = np.arange(every.size)
    mods = (1, 2, 3, 5, 7, 4)
    children = [[], [5], [4], [4, 5], [], []]
    comps = [ctx.spss_encode(capi.DeviceSet.from_kmers(g, every[rank % m == 0], ctx.device), mode=0) for m in mods]
    direct = np.stack([rank % m == 0 for m in mods]).astype(np.int64)
    member = ((closure(len(mods), children).T.astype(np.int64) @ direct) > 0).astype(np.int64)
    want = member @ member.T
    assert want[0, 0] == every.size and want[1, 1] == (direct[1] | direct[5]).sum()
    idx = capi.KssIndex.from_nodes(ctx, comps, children)
    for flush_rows in (0, 777):
        got, nd = idx.pair_counts(flush_rows=flush_rows, with_distinct=True)
        assert np.array_equal(got, want), flush_rows
        assert nd == every.size
    idx.close()


def test_columns(ctx):
    """130 fabricated nodes (every 7th holds nothing of its own) against a numpy closure: 1 to 128 columns in a
    shuffled order, nodes that have parents only, the sub-table in the order given; cols=None is refused at 130 nodes
    and serves 128; ids out of range, repeated ids and too many columns are refused; nodes whose Get is empty give
    zero rows and columns."""
    g, pool, node_sets, comps, children = fabricated(ctx, 130, 130, per_node=12, empty_every=7)
    want, distinct = closure_table(node_sets, children)
    idx = capi.KssIndex.from_nodes(ctx, comps, children)
    rng = np.random.default_rng(4)
    for n_cols in (1, 2, 63, 64, 65, 127, 128):
        cols = rng.permutation(130)[:n_cols]
        got, nd = idx.pair_counts(cols=cols, with_distinct=True)
        assert got.shape == (n_cols, n_cols) and np.array_equal(got, want[np.ix_(cols, cols)]), n_cols
        assert nd == distinct  # all nodes, not only the columns
    has_parent = sorted({c for ch in children for c in ch})
    inner = rng.permutation(has_parent)[:100]
    assert np.array_equal(idx.pair_counts(cols=inner), want[np.ix_(inner, inner)])
    for bad, word in ((None, "130 nodes"), ([0, 130], "outside"), ([-1], "outside"), ([5, 9, 5], "repeated"),
                      (list(range(129)), "n_cols"), ([], "n_cols")):
        with pytest.raises(capi.KshError) as e:
            idx.pair_counts(cols=bad)
        assert e.value.code == capi.KSH_INVALID_ARGUMENT and word in str(e.value), bad
    with pytest.raises(capi.KshError) as e:
        idx.pair_counts(flush_rows=-1)
    assert e.value.code == capi.KSH_INVALID_ARGUMENT
    assert np.array_equal(idx.pair_counts(cols=[7, 3]), want[np.ix_([7, 3], [7, 3])])  # still serving
    idx.close()

    idx = capi.KssIndex.from_nodes(ctx, comps[:128], [[c for c in ch if c < 128] for ch in children[:128]])
    want128, distinct128 = closure_table(node_sets[:128], [[c for c in ch if c < 128] for ch in children[:128]])
    got, nd = idx.pair_counts(with_distinct=True)
    assert got.shape == (128, 128) and np.array_equal(got, want128) and nd == distinct128
    idx.close()

    # nodes whose Get is empty: 1 (a leaf) and 3 (whose only child is 1)
    sets4 = [node_sets[1], np.zeros(0, dtype=np.uint64), node_sets[2], np.zeros(0, dtype=np.uint64)]
    comps4 = [capi.DeviceSpss.from_strings(g, kmer_strings(s, g.k), ctx.device) for s in sets4]
    ch4 = [[1, 2], [], [1], [1]]
    want4, _ = closure_table(sets4, ch4)
    idx = capi.KssIndex.from_nodes(ctx, comps4, ch4)
    got = idx.pair_counts()
    assert np.array_equal(got, want4)
    assert not got[1].any() and not got[:, 1].any() and not got[3].any() and not got[:, 3].any() and got[0, 2] > 0
    jac = idx.jaccard()
    assert jac[1, 3] == 1.0 and jac[1, 1] == 1.0 and jac[0, 1] == 0.0 and np.array_equal(jac, jaccard_of(want4))
    idx.close()


@pytest.mark.parametrize("flush_rows", [1, 64, 1000])
def test_flush(ctx, built, flush_rows):
    """A workgroup that flushes its counters after every tile, after 64 and after 1000 rows gives the default's
    table; the route bits say that it flushed, and that the default did not.  (A workgroup is started per 8192
    entries of the structure, so each holds well over 1000 rows in tiles of a few dozen.)"""
    dkss, gets, want, distinct = built(CASES[2])
    idx = capi.KssIndex.from_kss(dkss)
    one = idx.pair_counts()
    assert np.array_equal(one, want)
    assert not idx.routes() & capi.QROUTE_PAIR_FLUSH
    got, nd = idx.pair_counts(flush_rows=flush_rows, with_distinct=True)
    assert np.array_equal(got, one) and nd == distinct
    assert idx.routes() & capi.QROUTE_PAIR_FLUSH
    idx.close()


def test_wide_buckets(ctx):
    """(23, 18): 2^18 buckets, 4 sets of 2 * 10^4 k-mers: most buckets are empty and the workgroups stride over
    them."""
    sets, ocompacts, okss, dkss = build_both(ctx, 23, 18, 4, 4, 20000, 19)
    gets = [okss.get(i).kmers() for i in range(okss.size())]
    idx = capi.KssIndex.from_kss(dkss)
    got, nd = idx.pair_counts(with_distinct=True)
    assert np.array_equal(got, pair_table(gets))
    assert nd == np.unique(np.concatenate(gets)).size  # (Get(i) holds node i)
    idx.close()
    dkss.close()


def test_jaccard(ctx, built):
    """jaccard() is c_ab / (c_aa + c_bb - c_ab) of the oracle's counts (1.0 for two empty sets: test_columns)."""
    dkss, gets, want, distinct = built(CASES[1])
    idx = capi.KssIndex.from_kss(dkss)
    jac = idx.jaccard()
    assert jac.dtype == np.float64 and np.array_equal(jac, jaccard_of(want))
    assert np.all(np.diag(jac) == 1.0) and (jac < 1.0).any()
    cols = [2, 0]
    assert np.array_equal(idx.jaccard(cols), jaccard_of(want)[np.ix_(cols, cols)])
    idx.close()


def test_plans_stay_exact(ctx):
    """One victim of each plan group: plan, ksh_kss_pair_counts on a structure of the same context, then the write:
    served, and equal to a fresh plan + write (include/kmersets_hip.h, "Plans")."""
    k, n = 23, 14
    g = capi.geom(k, n)
    sets = synth.phylogeny_sets(k, 2, 20000, seed=17)
    a, b = (capi.DeviceSet.from_kmers(g, s, ctx.device) for s in sets)
    ca, cb = ctx.spss_encode(a, mode=0), ctx.spss_encode(b, mode=0)
    idx = capi.KssIndex.from_nodes(ctx, [ca, cb], [[1], []])
    both, nb = np.union1d(sets[0], sets[1]).size, np.asarray(sets[1]).size
    want = np.array([[both, nb], [nb, nb]], dtype=np.int64)

    def intrude():
        assert np.array_equal(idx.pair_counts(), want)
        got, nd = idx.pair_counts(cols=[1, 0], flush_rows=100, with_distinct=True)
        assert np.array_equal(got, want[::-1, ::-1]) and nd == both

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
