"""Selections on a KmerSetSet index (ksh_kss_select_count / ksh_kss_select_keys, capi.KssIndex.select / spectrum):
the k-mers q with min_count <= c(q) <= max_count, in every required and in no excluded Get, against the oracle's
Get(i) k-mers with np.unique(..., return_counts=True) and np.isin, numpy closures of fabricated DAGs and rank
arithmetic on the dense 9-mer space; split tiles, column words, wide buckets, empty selections, the write guard, and
pending plans of the context staying exact across the calls.  Every comparison is integer or array equality."""
import numpy as np
import pytest
import torch

import oracle_lib as ol
from kmersets import capi, synth

pytestmark = pytest.mark.gpu

CASES = [(9, 10, 1, 6, 3000, 11), (15, 14, 2, 8, 20000, 3), (23, 14, 4, 8, 30000, 5), (31, 14, 8, 4, 20000, 7)]
# spectrum[0 .. n] of the inputs of each case, from the oracle on the CPU: no class 1 .. n is empty
INPUT_SPECTRA = [[0, 386, 196, 49, 146, 299, 2462], [0, 4659, 2399, 306, 2308, 294, 2046, 3058, 13153],
                 [0, 11281, 5851, 875, 4596, 1107, 4618, 6091, 15016], [0, 5527, 4375, 3561, 13760]]


@pytest.fixture(scope="module")
def ctx(gpu):
    c = capi.Context(0)
    yield c
    c.close()


# ---- recipes of tests/test_gpu_pair_counts.py (copied: importing a test module would collect its tests twice) ----
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
EMPTY = np.zeros(0, dtype=np.uint64)


def closure_gets(node_sets, children):
    """Get(i) of a fabricated DAG: the union of the sets of the nodes reachable from i."""
    n = len(node_sets)
    anc = closure(n, children)
    return [np.unique(np.concatenate([EMPTY] + [node_sets[j] for j in range(n) if anc[j, i]])) for i in range(n)]


def want_selection(gets, cols, lo=1, hi=None, require=(), exclude=()):
    hi = len(cols) if hi is None else hi
    u, c = np.unique(np.concatenate([EMPTY] + [gets[i] for i in cols]), return_counts=True)
    keep = (c >= lo) & (c <= hi)
    for r in require:
        keep &= np.isin(u, gets[r])
    for x in exclude:
        keep &= ~np.isin(u, gets[x])
    return u[keep]


def want_spectrum(gets, n_distinct, cols):
    """spectrum[m] for m >= 1 from the Get(i) of the columns; spectrum[0] = the k-mers of the structure in none."""
    u, c = np.unique(np.concatenate([EMPTY] + [gets[i] for i in cols]), return_counts=True)
    spec = np.bincount(c, minlength=len(cols) + 1).astype(np.int64)
    spec[0] = n_distinct - u.size
    return spec


def check_selection(ctx, got, want, real_set=False):
    """`got` (a DeviceSet) holds exactly `want`, ascending; with real_set, the other calls take it for a set."""
    assert got.n_keys == want.size
    kmers = got.kmers()
    assert np.array_equal(kmers, want)
    assert np.all(kmers[1:] > kmers[:-1])
    off = got.offsets.cpu().numpy()
    assert off[0] == 0 and off[-1] == want.size and np.all(np.diff(off) >= 0)
    if real_set:
        assert ctx.set_hash(got) == int(np.bitwise_xor.reduce(want)) if want.size else ctx.set_hash(got) == 0
        assert np.array_equal(ctx.spss_decode(ctx.spss_encode(got, mode=0)).kmers(), want)


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
            made[case] = (dkss, gets, int(np.unique(np.concatenate(nodes)).size))
        return made[case]

    yield get
    for dkss, *_ in made.values():
        dkss.close()


@pytest.mark.parametrize("which", range(len(CASES)))
def test_select_vs_oracle(ctx, built, which):
    """The inputs as columns (and once internal nodes), on an index that borrows the structure's sets and on one that
    decodes the node containers: union, core, exactly one, accessory, private to input 0, in 0 and 1 but not in 2;
    the spectrum; the result as an argument of hash, encode and decode."""
    case = CASES[which]
    k, n, kb, n_sets = case[:4]
    dkss, gets, distinct = built(case)
    n_nodes = len(gets)
    inputs = list(range(n_sets))
    spec = want_spectrum(gets, distinct, inputs)
    print("expected spectrum of the inputs:", spec.tolist())
    assert spec.tolist() == INPUT_SPECTRA[which] and np.all(spec[1:] > 0)  # no wrong answer hides in an empty class
    inner = list(range(n_sets, n_nodes))[::-1][:5]
    assert len(inner) >= 2
    selections = [dict(cols=inputs), dict(cols=inputs, lo=n_sets), dict(cols=inputs, hi=1),
                  dict(cols=inputs, lo=2, hi=n_sets - 1), dict(cols=inputs, hi=1, require=[0]),
                  dict(cols=inputs, require=[0, 1], exclude=[2]), dict(cols=inner, lo=2),
                  dict(cols=inner[:2] + [1], hi=2, exclude=[inner[0]])]
    g = capi.geom(k, n)
    assert g.key_bytes == max(kb, 2)
    comps = [capi.DeviceSpss.from_strings(g, dkss.node_strings(i), ctx.device) for i in range(n_nodes)]
    owned = capi.KssIndex.from_nodes(ctx, comps, [dkss.children(i) for i in range(n_nodes)])
    borrowed = capi.KssIndex.from_kss(dkss)
    for idx in (borrowed, owned):
        sizes = []
        for s in selections:
            want = want_selection(gets, s["cols"], s.get("lo", 1), s.get("hi"), s.get("require", ()),
                                  s.get("exclude", ()))
            got = idx.select(s["cols"], s.get("lo", 1), s.get("hi"), s.get("require", ()), s.get("exclude", ()))
            check_selection(ctx, got, want, real_set=idx is borrowed)
            assert not idx.routes() & capi.QROUTE_PAIR_SPLIT  # these buckets fit one tile each
            sizes.append(want.size)
        print("selection sizes:", sizes)
        assert all(sizes[:6])
        got = idx.spectrum(inputs)
        assert got.dtype == np.int64 and np.array_equal(got, spec)
        table, nd = idx.pair_counts(cols=inputs, with_distinct=True)
        assert got.sum() == nd == distinct
        assert (np.arange(n_sets + 1) * got).sum() == np.trace(table)
        assert np.array_equal(idx.spectrum(inner), want_spectrum(gets, distinct, inner))
        assert np.array_equal(idx.spectrum(), want_spectrum(gets, distinct, range(n_nodes)))  # cols = NULL
        assert idx.select().n_keys == distinct  # the union of all nodes
    owned.close()
    borrowed.close()


def test_split_tiles(ctx):
    """(15, 4): 16 buckets of about 10^4 entries, a tile holds 512: every bucket is cut by key range many times, which
    is where the order of the tiles and the order inside a tile can go wrong.  The nodes are the oracle's containers of
    8 sets under a fabricated DAG; expected from the oracle sets' k-mers and a numpy closure."""
    k, n, kb, n_sets, size = 15, 4, 4, 8, 20000
    g = capi.geom(k, n)
    sets = synth.phylogeny_sets(k, n_sets, size, seed=31)
    osets = [ol.Set.from_kmers(k, n, kb, s) for s in sets]
    node_sets = [s.kmers() for s in osets]
    _, c = np.unique(np.concatenate(node_sets), return_counts=True)
    assert np.bincount(c, minlength=9).tolist() == [0, 4248, 2176, 369, 2389, 150, 1732, 3053, 13528]
    comps = [capi.DeviceSpss.from_strings(g, s.compact().strings(), ctx.device) for s in osets]
    children = [[1, 2], [3], [3, 4], [], [5], [], [7], []]
    gets = closure_gets(node_sets, children)
    distinct = int(np.unique(np.concatenate(node_sets)).size)
    cols = list(range(n_sets))
    idx = capi.KssIndex.from_nodes(ctx, comps, children)
    for lo, hi in ((n_sets, n_sets), (1, n_sets), (3, 3)):
        want = want_selection(gets, cols, lo, hi)
        assert want.size > 0
        got = idx.select(cols, lo, hi)
        assert idx.routes() & capi.QROUTE_PAIR_SPLIT
        check_selection(ctx, got, want, real_set=(lo == 3))
    want = want_selection(gets, [6, 0, 3], 1, 2, require=[3], exclude=[6])
    assert want.size > 0
    check_selection(ctx, idx.select([6, 0, 3], 1, 2, require=[3], exclude=[6]), want)
    assert np.array_equal(idx.spectrum(cols), want_spectrum(gets, distinct, cols))
    assert idx.routes() & capi.QROUTE_PAIR_SPLIT
    idx.close()


def test_dense_keys(ctx):
    """Every canonical 9-mer (131 072 of them; k = 9, N = 10: every bucket full, consecutive keys).  Node j holds the
    k-mers whose rank is divisible by m_j; every k-mer is in node 0.  Expected from the ranks."""
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
    count = member.sum(axis=0)
    idx = capi.KssIndex.from_nodes(ctx, comps, children)
    assert np.array_equal(idx.spectrum(), np.bincount(count, minlength=7))
    check_selection(ctx, idx.select(), every)
    for lo, hi in ((6, 6), (2, 2), (1, 1), (3, 5)):
        want = every[(count >= lo) & (count <= hi)]
        assert want.size > 0
        check_selection(ctx, idx.select(None, lo, hi), want)
    want = every[member[1] & member[3] & ~member[2]]
    assert want.size > 0
    check_selection(ctx, idx.select([3, 2, 1], require=[1, 3], exclude=[2]), want)
    idx.close()


def test_column_words(ctx):
    """130 fabricated nodes (every 7th holds nothing of its own) against a numpy closure: 1 to 128 columns in a
    shuffled order, so that the row takes one word, both, and the last bit of each; require and exclude ids on both
    sides of bit 64; the core of many columns may be empty: 0 keys and all-zero offsets.  The refusals that read the
    index, by their word, and the index serving after each."""
    g, pool, node_sets, comps, children = fabricated(ctx, 130, 130, per_node=12, empty_every=7)
    gets = closure_gets(node_sets, children)
    distinct = int(np.unique(np.concatenate(node_sets)).size)
    idx = capi.KssIndex.from_nodes(ctx, comps, children)
    rng = np.random.default_rng(4)
    sizes = []
    for n_cols in (1, 2, 63, 64, 65, 127, 128):
        cols = [int(c) for c in rng.permutation(130)[:n_cols]]
        want = want_selection(gets, cols, n_cols, n_cols)
        got = idx.select(cols, n_cols, n_cols)
        check_selection(ctx, got, want)
        if want.size == 0:
            assert got.n_keys == 0 and not got.offsets.cpu().numpy().any()
        check_selection(ctx, idx.select(cols), want_selection(gets, cols))
        assert np.array_equal(idx.spectrum(cols), want_spectrum(gets, distinct, cols)), n_cols
        # the columns ordered by |Get|: a large set required on one side of bit 64, a small one excluded on the other
        by_size = sorted(range(n_cols), key=lambda a: gets[cols[a]].size)
        low, high = [a for a in by_size if a < 64], [a for a in by_size if a >= 64]
        for req, exc in ((low[-1:], high[:1]), (high[-1:], low[:1]), (low[-1:] + high[-1:], low[:1] + high[:1])):
            req, exc = [cols[a] for a in req], [cols[a] for a in exc if cols[a] not in [cols[r] for r in req]]
            want = want_selection(gets, cols, require=req, exclude=exc)
            check_selection(ctx, idx.select(cols, require=req, exclude=exc), want)
            sizes.append((n_cols, len(req), len(exc), want.size))
    print("(n_cols, required, excluded, selected):", sizes)
    assert any(s[3] > 0 and s[1] and s[2] for s in sizes if s[0] >= 65)  # both words judged on a non-empty answer

    serve = want_selection(gets, [7, 3], require=[3])
    for bad, word in ((dict(cols=None), "130 nodes"), (dict(cols=[0, 130]), "outside"), (dict(cols=[-1]), "outside"),
                      (dict(cols=[5, 9, 5]), "repeated"), (dict(cols=list(range(129))), "n_cols"),
                      (dict(cols=[]), "n_cols"), (dict(cols=[5, 9], require=[130]), "outside"),
                      (dict(cols=[5, 9], require=[7]), "not in cols"), (dict(cols=[5, 9], exclude=[7]), "not in cols"),
                      (dict(cols=[5, 9], require=[9], exclude=[9]), "both"),
                      (dict(cols=[5, 9], max_count=3), "max_count"), (dict(cols=[5, 9], min_count=3), "min_count")):
        for call in (idx.select, idx.select_count):
            with pytest.raises(capi.KshError) as e:
                call(**bad)
            assert e.value.code == capi.KSH_INVALID_ARGUMENT and word in str(e.value), bad
        check_selection(ctx, idx.select([7, 3], require=[3]), serve)  # still serving
    with pytest.raises(capi.KshError) as e:
        idx.spectrum()
    assert e.value.code == capi.KSH_INVALID_ARGUMENT and "130 nodes" in str(e.value)
    idx.close()


def test_wide_buckets(ctx):
    """(23, 18): 2^18 buckets, 4 sets of 2 * 10^4 k-mers: most buckets are empty, the workgroups stride over them
    and the offsets come from the chained scan."""
    sets, ocompacts, okss, dkss = build_both(ctx, 23, 18, 4, 4, 20000, 19)
    gets = [okss.get(i).kmers() for i in range(okss.size())]
    distinct = int(np.unique(np.concatenate(gets)).size)  # (Get(i) holds node i)
    idx = capi.KssIndex.from_kss(dkss)
    for lo, hi in ((1, 4), (4, 4), (1, 1)):
        want = want_selection(gets, range(4), lo, hi)
        assert want.size > 0
        check_selection(ctx, idx.select(range(4), lo, hi), want, real_set=(lo == 4))
    assert np.array_equal(idx.spectrum(range(4)), want_spectrum(gets, distinct, range(4)))
    idx.close()
    dkss.close()


def test_empty_selection(ctx, built):
    """require {a}, exclude {b} with a reachable from b, so that Get(b) holds Get(a): nothing is selected on a
    structure that is far from empty; the write of nothing takes no key buffer."""
    dkss, gets, distinct = built(CASES[1])
    b = next(i for i in range(len(gets)) if dkss.children(i))
    a = dkss.children(b)[0]
    assert gets[a].size > 0 and np.isin(gets[a], gets[b]).all()
    idx = capi.KssIndex.from_kss(dkss)
    off, n, spec = idx.select_count([a, b], require=[a], exclude=[b], spectrum=True)
    assert n == 0 and not off.cpu().numpy().any()
    assert np.array_equal(spec, want_spectrum(gets, distinct, [a, b]))
    idx.select_write(off, 0, None, [a, b], require=[a], exclude=[b])  # KSH_OK
    got = idx.select([a, b], require=[a], exclude=[b])
    assert got.n_keys == 0 and got.kmers().size == 0
    idx.close()


def test_write_guard(ctx, built):
    """The offsets of the union with the request of the core: KSH_FAILED_PRECONDITION, and nothing written at or
    beyond the n_keys keys the call was given.  (The buffer holds every distinct k-mer of the structure, so even a
    wrong kernel stays inside it.)  A correct count + write on the same index is exact afterwards."""
    case = CASES[2]
    n_sets = case[3]
    dkss, gets, distinct = built(case)
    inputs = list(range(n_sets))
    idx = capi.KssIndex.from_kss(dkss)
    kb = idx.g.key_bytes
    off_union, n_union, _ = idx.select_count(inputs)
    off_core, n_core, _ = idx.select_count(inputs, n_sets)
    assert 0 < n_core < n_union <= distinct
    keys = torch.full((distinct * kb,), 0xA5, dtype=torch.uint8, device=ctx.device)
    with pytest.raises(capi.KshError) as e:
        idx.select_write(off_union, n_core, keys, inputs, n_sets)
    assert e.value.code == capi.KSH_FAILED_PRECONDITION and "ksh_kss_select_keys" in str(e.value)
    assert bool((keys[n_core * kb:] == 0xA5).all())
    with pytest.raises(capi.KshError) as e:  # the right offsets, too little room
        idx.select_write(off_core, n_core - 1, keys, inputs, n_sets)
    assert e.value.code == capi.KSH_FAILED_PRECONDITION
    assert bool((keys[n_core * kb:] == 0xA5).all())
    idx.select_write(off_core, n_core, keys, inputs, n_sets)
    assert bool((keys[n_core * kb:] == 0xA5).all())
    check_selection(ctx, capi.DeviceSet(idx.g, off_core, keys, n_core), want_selection(gets, inputs, n_sets))
    idx.close()


def test_plans_stay_exact(ctx):
    """One victim of each plan group: plan, a selection and a spectrum on a structure of the same context, then the
    write: served, and equal to a fresh plan + write (include/kmersets_hip.h, "Plans")."""
    k, n = 23, 14
    g = capi.geom(k, n)
    sets = synth.phylogeny_sets(k, 2, 20000, seed=17)
    a, b = (capi.DeviceSet.from_kmers(g, s, ctx.device) for s in sets)
    ca, cb = ctx.spss_encode(a, mode=0), ctx.spss_encode(b, mode=0)
    idx = capi.KssIndex.from_nodes(ctx, [ca, cb], [[1], []])
    only_a = np.setdiff1d(sets[0], sets[1])
    both, nb = np.union1d(sets[0], sets[1]).size, np.asarray(sets[1]).size
    assert only_a.size > 0

    def intrude():
        assert np.array_equal(idx.select(require=[0], exclude=[1]).kmers(), only_a)
        assert np.array_equal(idx.spectrum([1, 0]), [0, both - nb, nb])

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
