"""Sequences painted with colour classes (ksh_seq_class_runs, capi.KssIndex.class_runs / paint) against the numpy
reference of tests/paint_reference.py: oracle-built structures on a borrowed and an owned index, the coloured-graph
round trip, the edges of the run logic under every pass size, a class change at every position, both column words,
many nodes, the zero row and partial tables, the write guard, pending plans staying exact, and ksh_seq_hits giving
what it gave.  Every comparison is integer or array equality."""
import numpy as np
import pytest
import torch

import oracle_lib as ol
import paint_reference as pr
from paint_reference import with_zero_row
from index_reference import IndexReference, class_matrix, revcomp_string
from kmersets import capi, synth

pytestmark = pytest.mark.gpu

U = np.uint64
CASES = [(9, 10, 1, 6, 3000, 11), (15, 14, 2, 8, 20000, 3), (23, 14, 4, 8, 30000, 5), (31, 14, 8, 4, 20000, 7),
         (23, 18, 4, 4, 20000, 19)]  # those of test_gpu_class_ids.py, and its wide geometry
EMPTY = np.zeros(0, dtype=U)
ONES = (1 << 64) - 1
PATTERN = 0x5A5A5A5A


@pytest.fixture(scope="module")
def ctx(gpu):
    c = capi.Context(0)
    yield c
    c.close()


def build_both(ctx, k, n, kb, n_sets, size, seed):
    sets = synth.phylogeny_sets(k, n_sets, size, seed=seed)
    ocompacts = [ol.Set.from_kmers(k, n, kb, s).compact() for s in sets]
    ids = synth.sample_bucket_ids(n, seed=seed + 1)
    okss = ol.KmerSetSet(ocompacts, ids)
    g = capi.geom(k, n)
    dkss = capi.DeviceKmerSetSet(ctx, [capi.DeviceSpss.from_strings(g, c.strings(), ctx.device) for c in ocompacts], ids)
    return sets, ocompacts, okss, dkss


def kmer_strings(kmers, k):
    return ["".join("ACGT"[(int(x) >> (2 * (k - 1 - j))) & 3] for j in range(k)) for x in kmers]


def host(result):
    off, start, cls, missing = result
    assert off.dtype == torch.int64 and start.dtype == torch.int32 and cls.dtype == torch.int32 and off.is_cuda
    return off.cpu().numpy(), start.cpu().numpy(), cls.cpu().numpy(), missing


def same(got, want):
    return all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3])) and got[3] == want[3]


def positions(strings, k):
    return [len(s) - k + 1 for s in strings]


# ---- 1. oracle-built structures ---------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(len(CASES)))
def test_paint_vs_oracle(ctx, which):
    k, n, kb, n_sets, size, seed = CASES[which]
    sets, ocompacts, okss, dkss = build_both(ctx, k, n, kb, n_sets, size, seed)
    n_nodes = okss.size()
    # Get(i) of the oracle as column i: nodes without edges that hold their Get have that membership matrix
    ref = IndexReference(k, [okss.get(i).kmers() for i in range(n_nodes)], [[] for _ in range(n_nodes)])
    g = capi.geom(k, n)
    fwd = []
    for c in ocompacts[:2]:
        by_len = sorted(c.strings(), key=len)
        fwd += by_len[-12:] + by_len[:4]
    strings = fwd + [revcomp_string(s) for s in fwd]
    dseqs = capi.DeviceSpss.from_strings(g, strings, ctx.device)
    inner = list(range(n_sets, n_nodes))[::-1][:5]
    assert len(inner) >= 2
    column_sets = [list(range(n_sets)), [inner[0], 1, inner[1], 0]] + ([None] if n_nodes <= 128 else [])
    comps = [capi.DeviceSpss.from_strings(g, dkss.node_strings(i), ctx.device) for i in range(n_nodes)]
    owned = capi.KssIndex.from_nodes(ctx, comps, [dkss.children(i) for i in range(n_nodes)])
    borrowed = capi.KssIndex.from_kss(dkss)
    lengths = positions(strings, k)
    for cols in column_sets:
        table = with_zero_row(ref.color_classes(cols)[0])
        want = {canon: pr.class_runs(ref, strings, cols, table, canon) for canon in (True, False)}
        # the reference itself: a string and its reverse complement have mirrored runs when canonicalised, several
        # runs somewhere, and without canonicalising the mirrored strings read otherwise
        ids = pr.expand(*want[True][:3], lengths)
        half = len(fwd)
        assert all(np.array_equal(ids[j][::-1], ids[half + j]) for j in range(half))
        assert want[True][0][-1] > len(strings) and want[True][3] == 0
        assert not same(want[True], want[False])
        for idx in (borrowed, owned):
            for canon in (True, False):
                for route in (1, 2, 0):
                    got = host(idx.class_runs(dseqs, table, cols, canonicalize=canon, route=route))
                    assert same(got, want[canon]), (cols, canon, route)
                    bits = idx.routes()
                    assert bits & (capi.QROUTE_SEARCH if route == 1 else capi.QROUTE_JOIN if route == 2 else 3)
                    assert not bits & capi.QROUTE_SEQ_PASSES
            # paint makes the table itself; a k-mer of no node reads -1 unless the structure's table has the zero row
            off, start, cls, missing, rows, counts = idx.paint(dseqs, cols)
            assert np.array_equal(rows, ref.color_classes(cols)[0])
            assert same(host((off, start, cls, missing)), pr.class_runs(ref, strings, cols, rows, True))
    assert same(host(owned.class_runs(strings[:5], table, column_sets[-1])),
                pr.class_runs(ref, strings[:5], column_sets[-1], table, True))  # a list of str is uploaded
    owned.close()
    borrowed.close()
    dkss.close()


# ---- 2. the coloured-graph round trip ---------------------------------------------------------------------------
def test_colored_graph_round_trip(ctx):
    k, n, kb, n_sets, size, seed = CASES[2]
    sets, ocompacts, okss, dkss = build_both(ctx, k, n, kb, n_sets, size, seed)
    idx = capi.KssIndex.from_kss(dkss)
    cols = list(range(n_sets))
    ds, ids, rows, counts = idx.select_classes(cols)
    keys, ids = ds.kmers(), ids.cpu().numpy()
    spss = ctx.spss_encode(ds, mode=0)
    strings = spss.to_strings()
    for allow in (True, False):
        off, start, cls, missing = host(idx.class_runs(spss, rows, cols, allow_unmatched=allow))
        assert missing == (0 if allow else None)
        per_position = np.concatenate(pr.expand(off, start, cls, positions(strings, k)))
        x = synth.canonical(np.concatenate([synth.kmers_of_bases(synth.bases_of_string(s), k) for s in strings]), k)
        assert x.size == keys.size == per_position.size
        at = np.searchsorted(keys, x)
        assert np.array_equal(keys[at], x) and np.array_equal(ids[at], per_position)
    n_runs = int(off[-1])
    print("coloured graph: %d k-mers, %d strings, %d runs: %.4f runs per k-mer" % (keys.size, len(strings), n_runs,
                                                                                   n_runs / keys.size))
    assert len(strings) <= n_runs < keys.size
    idx.close()
    dkss.close()


# ---- 3. edges of the run logic ----------------------------------------------------------------------------------
PASSES = [1, 2, 63, 64, 65, 255, 256, 257, 4096, 0]


@pytest.fixture(scope="module")
def edges(ctx):
    """A genome of 8500 k-mer positions cut into consecutive sequences that overlap by K - 1 bases, so that the line
    of all positions IS the genome's k-mers in order; three columns whose membership changes at chosen positions, and
    a fourth node outside the columns whose membership flips every 7 positions: rows change where classes do not."""
    k, n, total = 15, 10, 8500
    g = capi.geom(k, n)
    genome = synth.random_genome(total + k - 1, 4242)
    x = synth.canonical(synth.kmers_of_bases(genome, k), k)
    assert np.unique(x).size == total  # a position's membership is its k-mer's
    changes = [10, 600, 640, 768, 819, 845, 1020, 1028, 1100, 2100, 2101, 2102, 2250, 4000, 4096, 4200, 8300]
    value = np.zeros(total, dtype=np.int64)
    for j, (a, b) in enumerate(zip([0] + changes, changes + [total])):
        value[a:b] = (1, 3, 0, 5, 7, 2, 6, 4)[j % 8]
    node_sets = [np.unique(x[(value >> c) & 1 == 1]) for c in range(3)] + [np.unique(x[(np.arange(total) // 7) % 2 == 1])]
    cuts = [0, 1260, 1280, 1300, 1530, 1536, 1542] + list(range(2000, 2301)) + [8192, total]
    text = synth.string_of_bases(genome)
    strings = [text[a:b + k - 1] for a, b in zip(cuts[:-1], cuts[1:])]
    assert sum(positions(strings, k)) == total and sum(len(s) == k for s in strings) >= 300
    ref = IndexReference(k, node_sets, [[], [], [], []])
    cols = [0, 1, 2]
    table = with_zero_row(ref.color_classes(cols)[0])
    want = pr.class_runs(ref, strings, cols, table, True)
    ids = np.concatenate(pr.expand(*want[:3], positions(strings, k)))
    assert np.array_equal(ids, np.searchsorted(table[:, 0], value.astype(U)))  # the classes are the chosen values
    comps = [capi.DeviceSpss.from_strings(g, kmer_strings(s, k), ctx.device) for s in node_sets]
    idx = capi.KssIndex.from_nodes(ctx, comps, [[], [], [], []])
    yield idx, ref, strings, cuts, cols, table, want, ids
    idx.close()


def test_edges_reference_has_the_cases(edges):
    idx, ref, strings, cuts, cols, table, want, ids = edges
    off, start, cls, missing = want
    flag = np.zeros(ids.size, dtype=bool)
    flag[np.array(cuts[:-1])] = True
    flag[1:] |= ids[1:] != ids[:-1]
    assert flag.sum() == off[-1] and missing == 0
    other = pr.position_ids(ref, strings[:1], [3], np.array([[0, 0], [1, 0]], dtype=U), True)[0]
    assert other[6] != other[7] and not flag[1:10].any()  # rows change inside a run: the classes decide
    for p in (4, 63, 64, 65, 126, 128, 130, 255, 256, 257, 512):  # a run spans wave, workgroup and pass edges
        assert not flag[p], p
    assert not flag[4160]
    for p in (640, 768, 819, 845, 1020, 1028, 4096):  # a class change exactly at a wave edge, a workgroup edge and at
        assert flag[p] and p not in cuts, p       # a cut of the passes of 64, 256, 63, 65, 255, 257 and 4096
    assert 640 % 64 == 0 and 768 % 256 == 0 and 819 % 63 == 0 and 845 % 65 == 0 and 1020 % 255 == 0 and 1028 % 257 == 0
    for p, pass_positions in ((1260, 63), (1280, 64), (1300, 65), (1530, 255), (1536, 256), (1542, 257), (8192, 4096)):
        assert p in cuts and p % pass_positions == 0 and ids[p] == ids[p - 1] and flag[p]  # a sequence starts a run
    assert 1300 % 64 != 0 and 1542 % 64 != 0  # ... and inside a wave
    assert flag[2000:2300].all() and (ids[2000:2100] == ids[2000]).all()  # every position a run, with equal classes
    assert max(positions(strings, ref.k)) > 4096  # one sequence longer than a pass


@pytest.mark.parametrize("pass_positions", PASSES)
def test_edges_every_pass(ctx, edges, pass_positions):
    idx, ref, strings, cuts, cols, table, want, ids = edges
    dseqs = capi.DeviceSpss.from_strings(idx.g, strings, ctx.device)
    for route in ((1,) if 0 < pass_positions < 63 else (1, 2)):  # (a pass of the join synchronises: not 8500 times)
        got = host(idx.class_runs(dseqs, table, cols, route=route, pass_positions=pass_positions))
        assert same(got, want), (pass_positions, route)
        assert bool(idx.routes() & capi.QROUTE_SEQ_PASSES) == (0 < pass_positions < ids.size)


# ---- 4. a class change at every position ------------------------------------------------------------------------
def test_many_classes(ctx):
    k, n, n_nodes = 15, 4, 20
    g = capi.geom(k, n)
    rng = np.random.default_rng(77)
    pool = np.unique(synth.canonical(rng.integers(0, 1 << 30, 30000), k))
    assert pool.size == 30000
    member = rng.random((n_nodes, 30000)) < 0.5
    node_sets = [pool[member[j]] for j in range(n_nodes)]
    comps = [ctx.spss_encode(capi.DeviceSet.from_kmers(g, s, ctx.device), mode=0) for s in node_sets]
    ref = IndexReference(k, node_sets, [[] for _ in range(n_nodes)])
    idx = capi.KssIndex.from_nodes(ctx, comps, [[] for _ in range(n_nodes)])
    cols = list(range(n_nodes))
    table = ref.color_classes(cols)[0]
    assert table.shape[0] == 29583
    singles = kmer_strings(pool, k)
    members = [int(c) for c in rng.integers(2, 40, size=300)]  # k-mers of the pool back to back, random joints
    longs = ["".join(singles[j] for j in rng.integers(0, 30000, size=c)) for c in members]
    for strings, least in ((singles, 30000), (longs, sum(members))):
        want = pr.class_runs(ref, strings, cols, table, True)
        assert want[0][-1] >= least and (want[0][-1] == least) == (strings is singles)
        assert np.unique(want[2]).size > least // 2  # (the joints read -1: the table has no zero row)
        dseqs = capi.DeviceSpss.from_strings(g, strings, ctx.device)
        off, start, cls, missing, rows, counts = idx.paint(dseqs, cols)  # the whole table, made by the call
        assert np.array_equal(rows, table) and same(host((off, start, cls, missing)), want)
        for route in (1, 2):
            assert same(host(idx.class_runs(dseqs, table.copy(), cols, route=route)), want)  # ... and the caller's
    idx.close()


# ---- 5. both column words ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_words(ctx):
    """The 131 fabricated nodes of tests/test_gpu_class_ids.py (its docstring says who reaches whom)."""
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
    idx = capi.KssIndex.from_nodes(ctx, comps, children)
    yield idx, IndexReference(k, node_sets, children), {j: own[s] for j, s in special.items()}
    idx.close()


@pytest.mark.parametrize("n_cols,present", [
    (128, [(ONES, 0, 63), (0, ONES, 127), (ONES, 1, 128), (ONES, ONES, 130)]),
    (64, [(ONES, 0, 63)]),
    (65, [(ONES, 0, 63), (ONES, 1, 128)])])
def test_both_column_words(two_words, n_cols, present):
    idx, ref, own = two_words
    k = ref.k
    cols = list(range(n_cols))
    table = ref.color_classes(cols)[0]
    have = {(int(r[0]), int(r[1])): c for c, r in enumerate(table)}
    nodes = [node for _, _, node in present] + [129]
    strings = [s for node in nodes for s in kmer_strings(own[node], k)]
    strings.append("".join(strings))  # ... and all of them in one sequence, random joints between them
    want = pr.class_runs(ref, strings, cols, table, True)
    for j, (r0, r1, node) in enumerate(present):
        assert (want[2][5 * j:5 * j + 5] == have[(r0, r1)]).all(), node
    assert (0, 0) in have and (want[2][5 * len(present):5 * len(present) + 5] == have[(0, 0)]).all()  # the root's own
    assert same(host(idx.class_runs(strings, table, cols)), want)
    assert same(host(idx.class_runs(strings, table, cols, route=2)), want)
    shuffled = [int(c) for c in np.random.default_rng(n_cols).permutation(128)[:n_cols]]
    table = ref.color_classes(shuffled)[0]
    want = pr.class_runs(ref, strings, shuffled, table, True)
    assert want[3] == 0 and same(host(idx.class_runs(strings, table, shuffled)), want)


# ---- 6. many nodes ----------------------------------------------------------------------------------------------
def test_many_nodes(ctx):
    k, n, n_nodes = 15, 10, 450
    g = capi.geom(k, n)
    rng = np.random.default_rng(450)
    pool = np.unique(synth.canonical(rng.integers(0, 1 << 30, 1200), k))
    node_sets = [EMPTY if j % 3 == 2 else np.unique(rng.choice(pool, size=3)) for j in range(n_nodes)]
    children = [[] for _ in range(n_nodes)]
    cols = list(range(6))
    for c in cols:
        children[c] = list(range(6 + 60 * c, 6 + 60 * c + 100))
    children[449] = [448]
    comps = [capi.DeviceSpss.from_strings(g, kmer_strings(s, k), ctx.device) for s in node_sets]
    ref = IndexReference(k, node_sets, children)
    idx = capi.KssIndex.from_nodes(ctx, comps, children)
    assert idx.words == 8
    picks = kmer_strings(pool, k)
    strings = picks[:100] + ["".join(picks[100:400]), "".join(picks[400:])]
    table = ref.color_classes(cols)[0]
    assert table.shape[0] > 8 and not table[0].any()
    for use in (cols, [449, 3, 200]):
        t = with_zero_row(ref.color_classes(use)[0])
        want = pr.class_runs(ref, strings, use, t, True)
        assert want[0][-1] > 200
        for route in (1, 2):
            assert same(host(idx.class_runs(strings, t, use, route=route)), want)
    with pytest.raises(capi.KshError) as e:  # cols = NULL on more than 128 nodes
        idx.class_runs(strings, table)
    assert e.value.code == capi.KSH_INVALID_ARGUMENT and "450 nodes" in str(e.value)
    assert same(host(idx.class_runs(strings, t, use)), want)  # still serving
    idx.close()


# ---- 7. the zero row and partial tables -------------------------------------------------------------------------
def test_zero_row_and_partial_tables(ctx):
    k, n = 15, 10
    g = capi.geom(k, n)
    rng = np.random.default_rng(7)
    pool = np.unique(synth.canonical(rng.integers(0, 1 << 30, 900), k))
    a, b, c, outside, nowhere = pool[:300], pool[200:500], pool[400:700], pool[700:800], pool[800:]
    node_sets = [np.unique(s) for s in (a, b, c, outside)]
    ref = IndexReference(k, node_sets, [[], [], [], []])
    comps = [capi.DeviceSpss.from_strings(g, kmer_strings(s, k), ctx.device) for s in node_sets]
    idx = capi.KssIndex.from_nodes(ctx, comps, [[], [], [], []])
    cols = [0, 1, 2]
    whole = ref.color_classes(cols)[0]
    assert not whole[0].any() and whole.shape[0] == 6  # (the k-mers of node 3 alone make the zero row a class)
    strings = kmer_strings(np.concatenate([nowhere[:3], outside[:3], a[:3], pool[250:253], nowhere[3:6]]), k)
    strings.append("".join(strings))
    want = pr.class_runs(ref, strings, cols, whole, True)
    assert (want[2][:6] == 0).all() and want[3] == 0  # in no node, and in a node outside cols: the same id
    assert same(host(idx.class_runs(strings, whole, cols)), want)
    strict = host(idx.class_runs(strings, whole, cols, allow_unmatched=False))
    assert strict[3] is None and same(strict[:3] + (0,), want)
    without = whole[1:]
    want = pr.class_runs(ref, strings, cols, without, True)
    assert (want[2][:6] == -1).all() and want[3] >= 12
    got = host(idx.class_runs(strings, without, cols))
    assert same(got, want) and np.array_equal(got[2].view(np.uint32) == capi.CLASS_NONE, want[2] < 0)
    one_bit = whole[[1, 2, 4]]
    assert [int(r) for r in one_bit[:, 0]] == [1, 2, 4]
    want = pr.class_runs(ref, strings, cols, one_bit, True)
    assert 0 < want[3] < sum(positions(strings, k))
    assert same(host(idx.class_runs(strings, one_bit, cols)), want)
    with pytest.raises(capi.KshError) as e:
        idx.class_runs(strings, one_bit, cols, allow_unmatched=False)
    assert e.value.code == capi.KSH_FAILED_PRECONDITION and "rows" in str(e.value) and str(want[3]) in str(e.value)
    assert same(host(idx.class_runs(strings, one_bit, cols)), want)  # still serving
    for bad in (np.array([[1, 0], [8, 0]], dtype=U), np.array([[1, 0], [1, 1]], dtype=U)):
        for allow in (False, True):
            with pytest.raises(capi.KshError) as e:
                idx.class_runs(strings, bad, cols, allow_unmatched=allow)
            assert e.value.code == capi.KSH_INVALID_ARGUMENT and "n_cols" in str(e.value) and "rows[1]" in str(e.value)
    for bad_cols, word in (([0, 4], "cols[1]"), ([1, 1], "repeated"), ([-1], "cols[0]")):
        with pytest.raises(capi.KshError) as e:
            idx.class_runs(strings, np.array([[1, 0]], dtype=U), bad_cols)
        assert e.value.code == capi.KSH_INVALID_ARGUMENT and word in str(e.value)
    assert same(host(idx.class_runs(strings, one_bit, cols, route=2)), want)
    idx.close()
    tiny = capi.geom(3, 5)  # K < 4
    idx = capi.KssIndex.from_nodes(ctx, [capi.DeviceSpss.from_strings(tiny, ["ACG"], ctx.device)], [[]])
    with pytest.raises(capi.KshError) as e:
        idx.class_runs(["ACGT"], np.array([[1, 0]], dtype=U), [0])
    assert e.value.code == capi.KSH_INVALID_ARGUMENT and "K >= 4" in str(e.value)
    idx.close()


# ---- 8. the write guard -----------------------------------------------------------------------------------------
def test_write_guard(ctx, edges):
    idx, ref, strings, cuts, cols, table, want, ids = edges
    dseqs = capi.DeviceSpss.from_strings(idx.g, strings, ctx.device)
    n_runs, n = int(want[0][-1]), len(strings)
    room = n_runs + 1000

    def fresh():
        return (torch.full((n + 1,), -5, dtype=torch.int64, device=ctx.device),
                torch.full((room,), PATTERN, dtype=torch.int32, device=ctx.device),
                torch.full((room,), PATTERN, dtype=torch.int32, device=ctx.device))

    for pass_positions in (0, 100):
        off, start, cls = fresh()
        rc, got, missing = idx.class_runs_raw(dseqs, table, n_runs - 1, off, start, cls, cols,
                                              pass_positions=pass_positions)
        assert rc == capi.KSH_FAILED_PRECONDITION and got == n_runs
        message = capi.lib().ksh_last_error().decode()
        assert "capacity" in message and str(n_runs) in message
        assert bool((start[n_runs - 1:] == PATTERN).all()) and bool((cls[n_runs - 1:] == PATTERN).all())
        off, start, cls = fresh()
        rc, got, missing = idx.class_runs_raw(dseqs, table, n_runs, off, start, cls, cols,
                                              pass_positions=pass_positions)
        assert rc == capi.KSH_OK and got == n_runs and missing == 0
        assert bool((start[n_runs:] == PATTERN).all()) and bool((cls[n_runs:] == PATTERN).all())
        assert same((off.cpu().numpy(), start[:n_runs].cpu().numpy(), cls[:n_runs].cpu().numpy(), 0), want)
        off, start, cls = fresh()
        rc, got, missing = idx.class_runs_raw(dseqs, table, 0, off, None, None, cols, pass_positions=pass_positions)
        assert rc == capi.KSH_OK and got == n_runs and np.array_equal(off.cpu().numpy(), want[0])
        rc, got, missing = idx.class_runs_raw(dseqs, table, 0, None, None, None, cols, pass_positions=pass_positions)
        assert rc == capi.KSH_OK and got == n_runs  # the count alone
    # no strings
    nothing = capi.DeviceSpss.from_strings(idx.g, [], ctx.device)
    off, start, cls = fresh()
    rc, got, missing = idx.class_runs_raw(nothing, table, 10, off, start, cls, cols)
    assert rc == capi.KSH_OK and got == 0 and missing == 0 and int(off[0]) == 0 and int(off[1]) == -5
    assert bool((start == PATTERN).all()) and bool((cls == PATTERN).all())
    o, s, c, missing = idx.class_runs([], table, cols)
    assert o.cpu().numpy().tolist() == [0] and s.numel() == 0 and c.numel() == 0 and missing == 0
    # malformed containers: refused, nothing written
    lens = dseqs.lens.clone()
    lens[3] = -1  # UINT32_MAX
    for bad, word in ((capi.DeviceSpss(idx.g, dseqs.words, dseqs.lens, n, dseqs.n_bases + 1), "n_bases"),
                      (capi.DeviceSpss(idx.g, dseqs.words, dseqs.lens, n, dseqs.n_bases - 1), "n_bases"),
                      (capi.DeviceSpss(idx.g, dseqs.words, lens, n, dseqs.n_bases), "lens[3]")):
        off, start, cls = fresh()
        with pytest.raises(capi.KshError) as e:
            idx.class_runs_raw(bad, table, room, off, start, cls, cols)
        assert e.value.code == capi.KSH_INVALID_ARGUMENT and word in str(e.value)
        assert bool((off == -5).all()) and bool((start == PATTERN).all()) and bool((cls == PATTERN).all())
    assert same(host(idx.class_runs(dseqs, table, cols)), want)  # still serving


# ---- 9. plans stay exact ----------------------------------------------------------------------------------------
def test_plans_stay_exact(ctx):
    """One victim of each plan group: plan, a painting on an index of the same context, then the write: served, and
    equal to a fresh plan + write (include/kmersets_hip.h, "Plans")."""
    k, n = 23, 14
    g = capi.geom(k, n)
    sets = synth.phylogeny_sets(k, 2, 20000, seed=17)
    a, b = (capi.DeviceSet.from_kmers(g, s, ctx.device) for s in sets)
    ca, cb = ctx.spss_encode(a, mode=0), ctx.spss_encode(b, mode=0)
    idx = capi.KssIndex.from_nodes(ctx, [ca, cb], [[1], []])
    ref = IndexReference(k, [np.sort(sets[0]), np.sort(sets[1])], [[1], []])
    table = np.array([[0, 0], [1, 0], [3, 0]], dtype=U)  # Get(0) holds Get(1): a alone has bit 0, b both bits
    strings = ca.to_strings() + cb.to_strings()[:30]
    want = pr.class_runs(ref, strings, [0, 1], table, True)
    assert want[3] == 0 and len(set(want[2].tolist())) >= 2

    def intrude():
        for route in (1, 2):
            assert same(host(idx.class_runs(strings, table, [0, 1], route=route, pass_positions=5000)), want)

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


# ---- 10. seq_hits is unchanged ----------------------------------------------------------------------------------
def test_seq_hits_unchanged_and_equal_to_the_runs_summed(ctx):
    k, n, kb, n_sets, size, seed = CASES[1]
    sets, ocompacts, okss, dkss = build_both(ctx, k, n, kb, n_sets, size, seed)
    n_nodes = okss.size()
    ref = IndexReference(k, [okss.get(i).kmers() for i in range(n_nodes)], [[] for _ in range(n_nodes)])
    strings = []
    for c in ocompacts[:3]:
        by_len = sorted(c.strings(), key=len)
        strings += by_len[-20:] + by_len[:5]
    strings += [revcomp_string(s) for s in strings[::3]]
    idx = capi.KssIndex.from_kss(dkss)
    dseqs = capi.DeviceSpss.from_strings(idx.g, strings, ctx.device)
    want_hits = ref.seq_hits(strings, True)
    before = idx.seq_hits(dseqs)
    assert np.array_equal(before, want_hits) and before.any()
    cols = [n_nodes - 1, 0, 2, 5]
    off, start, cls, missing, rows, counts = idx.paint(dseqs, cols)
    off, start, cls = off.cpu().numpy(), start.cpu().numpy(), cls.cpu().numpy()
    for route in (1, 2, 0):
        assert np.array_equal(idx.seq_hits(dseqs, route=route), before)
    # the run lengths summed per column (a position without a class is in no column: the zero row, if it is missing)
    bits = np.concatenate([class_matrix(rows, len(cols)), np.zeros((1, len(cols)), dtype=bool)]).astype(np.int64)
    hits = np.zeros((len(strings), len(cols)), dtype=np.int64)
    for s, n_pos in enumerate(positions(strings, k)):
        a, b = off[s], off[s + 1]
        ends = np.concatenate([start[a + 1:b], [n_pos]])
        hits[s] = ((ends - start[a:b])[:, None] * bits[cls[a:b]]).sum(axis=0)
    assert np.array_equal(hits, before[:, cols].astype(np.int64))
    idx.close()
    dkss.close()
