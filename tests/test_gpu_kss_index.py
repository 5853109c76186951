"""KmerSetSet membership index (ksh_kss_index_*, capi.KssIndex): for every query k-mer, the nodes i whose
Get(i) (lib/core/kmer_set_set.h:433-454) holds it, on both routes (per-query search, bucket join) and auto,
against the oracle's Get(i).Contains, numpy closures of fabricated DAGs, and Get(i) of the device structure."""
import numpy as np
import pytest
import torch

import oracle_lib as ol
from kmersets import capi, synth, synth_torch

pytestmark = pytest.mark.gpu

ROUTES = (1, 2, 0)


@pytest.fixture(scope="module")
def ctx(gpu):
    c = capi.Context(0)
    yield c
    c.close()


def build_both(ctx, k, n, kb, n_sets, size, seed, max_iterations=-1):
    sets = synth.phylogeny_sets(k, n_sets, size, seed=seed)
    osets = [ol.Set.from_kmers(k, n, kb, s) for s in sets]
    ocompacts = [s.compact() for s in osets]
    ids = synth.sample_bucket_ids(n, seed=seed + 1)
    okss = ol.KmerSetSet(ocompacts, ids, max_iterations=max_iterations)
    g = capi.geom(k, n)
    dcompacts = [capi.DeviceSpss.from_strings(g, c.strings(), ctx.device) for c in ocompacts]
    dkss = capi.DeviceKmerSetSet(ctx, dcompacts, ids, max_iterations=max_iterations)
    return sets, osets, okss, dkss


def queries(sets, k, seed, per_set=300):
    rng = np.random.default_rng(seed)
    mem = np.concatenate([rng.choice(s, size=min(per_set, s.size), replace=False) for s in sets]).astype(np.uint64)
    rc = synth.revcomp(mem, k).astype(np.uint64)
    rnd = rng.integers(0, 1 << (2 * k), size=per_set, dtype=np.uint64)
    top = np.uint64(1) << np.uint64(2 * k)
    out = (mem[:50] | top, rnd[:50] | (np.uint64(1) << np.uint64(63)))  # patterns with bits at or above 2K
    return np.concatenate([mem, rc, rnd, *out]).astype(np.uint64)


def expected_rows(gets, q, k, canonicalize):
    qq = synth.canonical(q, k).astype(np.uint64) if canonicalize else q
    rows = np.stack([np.isin(qq, s) for s in gets], axis=1)
    rows[(q >> np.uint64(2 * k)) != 0] = False
    return rows


def closure(n, children):
    anc = np.eye(n, dtype=bool)  # anc[j, i]: j reachable from i
    order, indeg = [], [0] * n
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


@pytest.mark.parametrize("case", [(9, 10, 1, 6, 3000, 11), (15, 14, 2, 8, 20000, 3),
                                  (23, 14, 4, 8, 30000, 5), (31, 14, 8, 4, 20000, 7)])
def test_index_vs_oracle(ctx, case):
    """Every node's column == the oracle's Get(i).Contains, canonicalised or as given, on routes 1, 2 and auto;
    the index built from the downloaded node strings and children (the Load path) gives the same rows."""
    k, n, kb, n_sets, size, seed = case
    sets, osets, okss, dkss = build_both(ctx, k, n, kb, n_sets, size, seed)
    n_nodes = okss.size()
    gets = [okss.get(i).kmers() for i in range(n_nodes)]
    q = queries(sets, k, seed)
    idx = capi.KssIndex.from_kss(dkss)
    assert idx.info()["n_nodes"] == n_nodes and idx.words == (n_nodes + 63) // 64
    for canon in (True, False):
        want = expected_rows(gets, q, k, canon)
        for route in ROUTES:
            got = idx.query(q, canonicalize=canon, route=route)
            assert got.shape == want.shape
            assert np.array_equal(got, want), (canon, route)
            bits = idx.routes()
            assert bits & (capi.QROUTE_SEARCH if route == 1 else capi.QROUTE_JOIN if route == 2 else 3)
    g = capi.geom(k, n)
    comps = [capi.DeviceSpss.from_strings(g, dkss.node_strings(i), ctx.device) for i in range(n_nodes)]
    idx2 = capi.KssIndex.from_nodes(ctx, comps, [dkss.children(i) for i in range(n_nodes)])
    for route in (1, 2):
        assert np.array_equal(idx2.query(q, route=route, packed=True), idx.query(q, route=route, packed=True))
    idx2.close()
    idx.close()
    dkss.close()


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


@pytest.mark.parametrize("n_nodes", [150, 700])
def test_wide_rows(ctx, n_nodes):
    """W = 3 and 11 words per row on fabricated DAGs (edges from lower to higher ids), against a numpy closure."""
    k = 15
    g, pool, node_sets, comps, children = fabricated(ctx, n_nodes, n_nodes, k=k, empty_every=37)
    idx = capi.KssIndex.from_nodes(ctx, comps, children)
    assert idx.words == (n_nodes + 63) // 64
    anc = closure(n_nodes, children)
    rng = np.random.default_rng(1)
    q = np.concatenate([pool, rng.integers(0, 1 << (2 * k), size=2000, dtype=np.uint64)]).astype(np.uint64)
    direct = np.stack([np.isin(q, s) for s in node_sets], axis=1)  # [query, j]
    want = (direct.astype(np.int32) @ anc.astype(np.int32)) > 0     # OR over j of anc[j]
    for route in ROUTES:
        assert np.array_equal(idx.query(q, canonicalize=False, route=route), want), route
    assert idx.query(np.zeros(0, dtype=np.uint64)).shape == (0, n_nodes)
    idx.close()


def test_refusals_and_small_shapes(ctx):
    g, pool, node_sets, comps, children = fabricated(ctx, 4, 5)
    for bad in ([[1], [2], [0], []], [[0], [], [], []], [[9], [], [], []]):
        with pytest.raises(capi.KshError) as e:
            capi.KssIndex.from_nodes(ctx, comps, bad)
        assert e.value.code == capi.KSH_INVALID_ARGUMENT
    one = capi.KssIndex.from_nodes(ctx, comps[:1], [[]])
    q = np.concatenate([pool, pool ^ np.uint64(5)]).astype(np.uint64)
    for route in ROUTES:
        assert np.array_equal(one.query(q, canonicalize=False, route=route)[:, 0], np.isin(q, node_sets[0]))
    one.close()
    empty = [capi.DeviceSpss.from_strings(g, [], ctx.device) for _ in range(3)]
    idx = capi.KssIndex.from_nodes(ctx, empty, [[1], [2], []])
    for route in ROUTES:
        assert not idx.query(q, route=route).any()
    assert idx.query(np.zeros(0, dtype=np.uint64), route=2).shape == (0, 3)
    idx.close()


def device_family(ctx, k, n, n_sets, size, seed):
    g = capi.geom(k, n)
    sets = synth_torch.phylogeny_sets(k, n_sets, size, seed, ctx.device)
    comps = [ctx.spss_encode(synth_torch.device_set(g, s), mode=0) for s in sets]
    return g, sets, comps


def check_family(ctx, g, sets, comps, children, n_queries, seed, routes=(1, 2)):
    idx = capi.KssIndex.from_nodes(ctx, comps, children)
    members = torch.cat(sets)
    gen = torch.Generator(device=ctx.device).manual_seed(seed)
    pick = torch.randint(0, members.numel(), (n_queries // 2,), device=ctx.device, generator=gen)
    rnd = torch.randint(0, 1 << (2 * g.k), (n_queries - n_queries // 2,), device=ctx.device, generator=gen)
    q = torch.cat([members[pick], rnd])
    n_nodes = len(comps)
    anc = torch.from_numpy(closure(n_nodes, children)).to(ctx.device)
    qc = torch.minimum(q, synth_torch.revcomp(q, g.k))  # what the index looks up (canonicalize=True)
    direct = torch.stack([torch.isin(qc, s) for s in sets], dim=1)
    want = (direct.to(torch.float32) @ anc.to(torch.float32)) > 0
    seen = 0
    for route in routes:
        got = idx.query(q, route=route, packed=True)
        bits = ((got[:, :1] >> torch.arange(n_nodes, device=ctx.device)) & 1).bool()
        assert torch.equal(bits, want), route
        seen |= idx.routes()
    idx.close()
    return seen


def test_oversize_slices(ctx):
    """(15, 4): about 6 * 10^4 keys per bucket, more than the join's LDS stage holds -> the HBM search fallback."""
    g, sets, comps = device_family(ctx, 15, 4, 3, 10 ** 6, 21)
    seen = check_family(ctx, g, sets, comps, [[1, 2], [2], []], 200000, 3)
    assert seen & capi.QROUTE_OVERSIZE and seen & capi.QROUTE_JOIN and seen & capi.QROUTE_SEARCH


def test_wide_buckets(ctx):
    """(23, 18, 4): 2^18 buckets, few keys per slice, both routes."""
    g, sets, comps = device_family(ctx, 23, 18, 3, 200000, 22)
    seen = check_family(ctx, g, sets, comps, [[2], [2], []], 300000, 4)
    assert not seen & capi.QROUTE_OVERSIZE


def test_join_two_chunks(ctx):
    """2 * 10^7 queries against a structure of 8 x 10^6 k-mers: the join takes two passes; auto gives the same rows
    (it searches: the keys fit the Infinity Cache).  Expected from dkss.get_kmers(i) and isin."""
    k, n = 23, 14
    g, sets, comps = device_family(ctx, k, n, 8, 10 ** 6, 23)
    ids = synth.sample_bucket_ids(n, seed=24)
    dkss = capi.DeviceKmerSetSet(ctx, comps, ids)
    n_nodes = dkss.size()
    idx = capi.KssIndex.from_kss(dkss)
    members = torch.cat(sets)
    gen = torch.Generator(device=ctx.device).manual_seed(5)
    nq = 2 * 10 ** 7
    pick = torch.randint(0, members.numel(), (nq // 2,), device=ctx.device, generator=gen)
    rnd = torch.randint(0, 1 << (2 * k), (nq - nq // 2,), device=ctx.device, generator=gen)
    q = torch.cat([members[pick], rnd])
    got = idx.query(q, route=2, packed=True)
    assert idx.routes() == capi.QROUTE_JOIN | capi.QROUTE_CHUNKED
    assert torch.equal(idx.query(q, route=0, packed=True), got)
    assert idx.routes() == capi.QROUTE_SEARCH
    qc = torch.minimum(q, synth_torch.revcomp(q, k))  # what the index looks up (canonicalize=True)
    for i in range(n_nodes):
        s = torch.from_numpy(dkss.get_kmers(i).view(np.int64)).to(ctx.device)
        col = ((got[:, i // 64] >> (i % 64)) & 1).bool()
        assert torch.equal(col, torch.isin(qc, s)), i
    del got
    idx.close()
    dkss.close()


def test_join_past_2e23_tiles(ctx):
    """N = 24: a pass of 1.6 x 10^7 queries touches more than 2^23 buckets, i.e. more join tiles than one
    workgroup each could launch (2^23 x 512 work-items pass 2^32); the join walks them on a capped grid.  Auto
    keeps the search here (under two queries per bucket)."""
    k, n = 23, 24
    g, sets, comps = device_family(ctx, k, n, 2, 200000, 25)
    children = [[1], []]
    idx = capi.KssIndex.from_nodes(ctx, comps, children)
    gen = torch.Generator(device=ctx.device).manual_seed(6)
    members = torch.cat(sets)
    nq = 16 * 10 ** 6
    pick = torch.randint(0, members.numel(), (nq // 8,), device=ctx.device, generator=gen)
    rnd = torch.randint(0, 1 << (2 * k), (nq - nq // 8,), device=ctx.device, generator=gen)
    q = torch.cat([members[pick], rnd])  # looked up as given (canonical k-mers crowd the lower buckets)
    assert torch.unique(q >> (2 * k - n)).numel() > 1 << 23
    want = torch.stack([torch.isin(q, sets[0]) | torch.isin(q, sets[1]), torch.isin(q, sets[1])], dim=1)
    for route in (2, 1, 0):
        got = idx.query(q, canonicalize=False, route=route, packed=True)
        bits = ((got[:, :1] >> torch.arange(2, device=ctx.device)) & 1).bool()
        assert torch.equal(bits, want), route
        assert idx.routes() == (capi.QROUTE_JOIN if route == 2 else capi.QROUTE_SEARCH)
        del got, bits
    idx.close()


def test_index_refuses_after_its_structure_closes(ctx):
    """from_kss borrows the structure's node sets: once the structure is closed the index refuses to query."""
    sets, osets, okss, dkss = build_both(ctx, 15, 14, 2, 3, 5000, 13)
    idx = capi.KssIndex.from_kss(dkss)
    q = np.asarray(sets[0][:100], dtype=np.uint64)
    assert idx.query(q)[:, 0].all()
    dkss.close()
    with pytest.raises(capi.KshError) as e:
        idx.query(q)
    assert e.value.code == capi.KSH_FAILED_PRECONDITION
    assert idx.h is None
